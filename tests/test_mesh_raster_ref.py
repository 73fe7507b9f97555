"""CPU tests of the mesh visibility rasterizer's contract (include/gsr_mesh.h) on its numpy
restatement tests/mesh_raster_ref.py: hand-computed answers, the edge / tie / cull rules, and the
float32 evaluation (what the kernel computes, bit for bit: test_gpu_mesh_raster.py) judged against
float64 on the template mesh.

The integer-coordinate scenes use z = 2 with tanfov = 0.5 (mesh_raster_cases.py): there
den = z + 1e-7f rounds to z in float32, so pixel coordinates are exact integers.  (With z = 1 and
tanfov = 1, 1 + 1e-7f rounds to 1 + 2^-23 and no vertex lands on an integer.)"""
import functools
import os
import re

import numpy as np
import pytest

import mesh_raster_cases as cs
import mesh_raster_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.float32, np.float64)


def _run(verts, faces, W, H, dtype):
    return ref.rasterize(verts, faces, cs.EYE, cs.TANFOV_EXACT, cs.TANFOV_EXACT, W, H, dtype)


def test_one_triangle_hand_computed(dtype=np.float32):
    """Pixel-space vertices (1,1), (5,1), (1,5) with z = 2, 2, 4 at 8x8: area = -16, the strictly
    interior centres are (2,2), (3,2), (2,3).  At (2,2): w = (1/2, 1/4, 1/4), t = (4, 2, 1), d = 7,
    b = (4/7, 2/7, 1/7), pz = 16/7.  At (3,2): w = (1/4, 1/2, 1/4) -> t = (2, 4, 1), pz = 16/7;
    at (2,3): w = (1/4, 1/4, 1/2) -> t = (2, 2, 2), d = 6, b = 1/3 each, pz = 8/3.  float32 only: in
    float64 den = z + 1e-7 moves the vertices off the integers and the centres on the hypotenuse in."""
    T = dtype
    v = cs.pixel_verts([(1, 1, 2), (5, 1, 2), (1, 5, 4)], 8, 8)
    r = _run(v, np.array([[0, 1, 2]], np.int32), 8, 8, dtype)
    want = np.full((8, 8), -1, np.int32)
    want[2, 2] = want[2, 3] = want[3, 2] = 0  # [yi, xi]
    assert np.array_equal(r["pix_to_face"], want)
    assert r["stats"] == (0, 1, 0, 3) and r["face_visible"].tolist() == [1]  # (a 5x5 box: the wide path)
    for (xi, yi), t in (((2, 2), (4, 2, 1)), ((3, 2), (2, 4, 1)), ((2, 3), (2, 2, 2))):
        b = np.array([T(x) / T(sum(t)) for x in t], T)
        pz = (b[0] * T(2) + b[1] * T(2)) + b[2] * T(4)
        assert np.array_equal(r["bary"][yi, xi], b), (xi, yi)  # exact coordinates: the very bits
        assert r["zbuf"][yi, xi] == pz
        exact = (2 * t[0] + 2 * t[1] + 4 * t[2]) / sum(t)
        assert abs(float(pz) - exact) <= 2 * np.spacing(T(exact))
    assert (r["zbuf"][want < 0] == -1).all() and (r["bary"][want < 0] == -1).all()


def test_constant_depth_triangle_coverage(dtype=np.float32):
    """(1,1), (7,1), (1,7) at z = 2: the ten centres with xi > 1, yi > 1, xi + yi < 8; pz = 2 and
    b_i = w_i = (8 - xi - yi, xi - 1, yi - 1) / 6 up to rounding."""
    v = cs.pixel_verts([(1, 1, 2), (7, 1, 2), (1, 7, 2)], 8, 8)
    r = _run(v, np.array([[0, 1, 2]], np.int32), 8, 8, dtype)
    yi, xi = np.mgrid[0:8, 0:8]
    inside = (xi > 1) & (yi > 1) & (xi + yi < 8)
    assert inside.sum() == 10 and np.array_equal(r["pix_to_face"] >= 0, inside)
    assert np.abs(r["zbuf"][inside] - 2.0).max() < 1e-6
    want = np.stack([8 - xi - yi, xi - 1, yi - 1], -1)[inside] / 6.0
    assert np.abs(r["bary"][inside] - want).max() < 1e-6


@pytest.mark.parametrize("W,H", [(8, 8), (32, 24)])
def test_edge_rule(W, H):
    """Integer pixel coordinates (float32: asserted): a centre on the shared diagonal, on an outer edge
    or on a vertex has some w_i == 0 exactly and belongs to no face (strict > 0, as PyTorch3D)."""
    v, f = cs.edge_scene(W, H)
    lo, hi = 1, cs.EDGE_HI[H]
    px, py, zv = ref._project(v, cs.EYE, cs.TANFOV_EXACT, cs.TANFOV_EXACT, W, H, np.float32)
    assert px.tolist() == [lo, hi, hi, lo] and py.tolist() == [lo, lo, hi, hi] and zv.tolist() == [2] * 4
    r = _run(v, f, W, H, np.float32)
    yi, xi = np.mgrid[0:H, 0:W]
    box = (xi > lo) & (xi < hi) & (yi > lo) & (yi < hi)
    want = np.full((H, W), -1, np.int32)
    want[box & (xi > yi)] = 0  # (A,B,C): the side of the diagonal with the larger x
    want[box & (xi < yi)] = 1
    assert np.array_equal(r["pix_to_face"], want)
    for p in range(lo, hi + 1):
        assert r["pix_to_face"][p, p] == -1  # the diagonal, both end vertices included
        assert r["pix_to_face"][lo, p] == -1 and r["pix_to_face"][p, hi] == -1  # outer edges of face 0
    assert (np.abs(r["zbuf"][want >= 0] - 2) <= 2 * np.spacing(np.float32(2))).all()
    assert (r["min_w"][want >= 0] >= 0.99 / (hi - lo)).all()  # w_i are multiples of 1/(hi - lo), rounded


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicate_face_lowest_index_wins(dtype):
    v = cs.pixel_verts([(0.3, 0.4, 3.0), (7.6, 0.7, 2.5), (3.1, 7.4, 3.5)], 8, 8)
    r = _run(v, np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2]], np.int32), 8, 8, dtype)
    assert (r["pix_to_face"] >= 0).sum() > 10
    assert set(np.unique(r["pix_to_face"])) == {-1, 0}
    assert r["face_visible"].tolist() == [1, 0, 0]
    assert (r["z_gap"][r["pix_to_face"] >= 0] == 0).all()  # the runner-up is the copy


@pytest.mark.parametrize("dtype", DTYPES)
def test_culled_faces_never_appear(dtype):
    """Zero area, behind the camera, off-screen, a vertex index out of range: no pixel, not visible."""
    pts = [(1, 1, 3), (6, 1.5, 3), (2, 6, 3),           # 0: a visible face
           (2, 3, 2.2), (4, 5, 2.2), (3, 4, 2.2),       # 1: zero area (collinear), in front
           (2, 2, -3), (6, 2.5, -3), (3, 6, -3),        # 2: behind the camera
           (50, 52, 2), (60, 53, 2), (55, 61, 2)]       # 3: off-screen
    v = cs.pixel_verts(pts, 8, 8)
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 1, 99], [4, 4, 5]], np.int32)
    r = _run(v, f, 8, 8, dtype)
    assert set(np.unique(r["pix_to_face"])) == {-1, 0}
    assert r["face_visible"].tolist() == [1, 0, 0, 0, 0, 0]
    n_lane, n_wide, n_cull, covered = r["stats"]
    assert n_cull == 4 and n_lane + n_wide == 2 and covered == (r["pix_to_face"] == 0).sum()


def test_interpenetrating_triangles_switch_winner():
    """hand_scene's two big triangles have opposite depth slopes: both win pixels, and the winner is
    the nearer of the two wherever both cover (the per-pixel depth test, not a per-face order)."""
    v, f = cs.hand_scene(32, 24)
    a, b = cs.HAND_FACES.index("big_a"), cs.HAND_FACES.index("big_b")
    both = _run(v, f[[a, b]], 32, 24, np.float32)
    ra, rb = _run(v, f[[a]], 32, 24, np.float32), _run(v, f[[b]], 32, 24, np.float32)
    overlap = (ra["pix_to_face"] >= 0) & (rb["pix_to_face"] >= 0)
    assert overlap.sum() > 50
    nearer = np.where(ra["zbuf"] <= rb["zbuf"], 0, 1)
    assert np.array_equal(both["pix_to_face"][overlap], nearer[overlap])
    assert 10 < (nearer[overlap] == 0).sum() < overlap.sum() - 10
    assert np.array_equal(both["zbuf"][overlap], np.minimum(ra["zbuf"], rb["zbuf"])[overlap])


def test_hand_scene_paths():
    """The scene the GPU test renders takes every path: lane and wide faces, two culled faces (zero
    area, behind; the off-screen face passes the culls with an empty box), the sub-pixel face covering
    nothing, the huge face filling what nothing nearer covers."""
    for W, H in ((8, 8), (32, 24)):
        v, f = cs.hand_scene(W, H)
        r = _run(v, f, W, H, np.float32)
        n_lane, n_wide, n_cull, covered = r["stats"]
        assert n_cull == 2 and n_wide >= 3 and n_lane >= 1 and covered == W * H
        vis = dict(zip(cs.HAND_FACES, r["face_visible"]))
        assert vis["dup_0"] == 1 and vis["huge"] == 1 and vis["big_a"] == 1 and vis["big_b"] == 1
        for name in ("dup_1", "zero_area", "behind", "offscreen", "subpixel"):
            assert vis[name] == 0, name


@functools.lru_cache(maxsize=None)
def _pair(i):
    W, H, yaw, dist = cs.F32_F64_INPUTS[i]
    v, f = cs.template()
    tx, ty = cs.template_fov(W, H)
    M = cs.template_camera(yaw, dist)
    return tuple(ref.rasterize(v, f, M, tx, ty, W, H, dt) for dt in DTYPES)


BARY_C = 1178  # twice the smallest integer (589) the float32 restatement meets on F32_F64_INPUTS


@pytest.mark.parametrize("i", range(len(cs.F32_F64_INPUTS)))
def test_float32_against_float64_on_template(i):
    """Template mesh (V = 10,475, F = 20,908) under F32_F64_INPUTS.  A pixel is flagged when its
    float64 winner has min|w_i| < 1e-4 or a z gap below 1e-5.  Every pixel where float32 and float64
    pick different faces is flagged; flagged pixels are at most 0.5 % of the covered ones; the visible
    face sets are equal; on unflagged pixels |z32 - z64| <= 16 ulp(z) and each barycentric is within
    c * 2^-24 * S/|area| of float64 (S: the sum of the absolute values of the winner's six
    edge-function products, in float64).

    Measured (float32 restatement, the five inputs in order): differing pixels 0 everywhere; flagged
    0, 0, 1, 3, 5 of 682, 628, 2,559, 2,318, 11,066 covered; visible faces 678, 627, 2,055, 567,
    4,009; worst z error 2.2, 1.9, 2.5, 3.1, 2.8 ulp; worst barycentric error 1.4e-4 absolute, in
    units of 2^-24 * S/|area|: 283.2, 498.2, 301.9, 50.2, 588.7.  The smallest integer c that holds is
    589; the bound asserted is its double, 1178."""
    a, b = _pair(i)
    cov = b["pix_to_face"] >= 0
    flag = cov & ((b["min_w"] < 1e-4) | (b["z_gap"] < 1e-5))
    differ = a["pix_to_face"] != b["pix_to_face"]
    print(cs.F32_F64_INPUTS[i], "covered", int(cov.sum()), "flagged", int(flag.sum()), "differ", int(differ.sum()),
          "visible", int(b["face_visible"].sum()))
    assert cov.sum() > 500 and b["face_visible"].sum() > 500  # not vacuous
    assert not (differ & ~flag).any()
    assert flag.sum() <= 0.005 * cov.sum()
    assert np.array_equal(a["face_visible"], b["face_visible"])
    ok = cov & ~flag & ~differ
    z64 = b["zbuf"][ok]
    zerr = np.abs(a["zbuf"][ok].astype(np.float64) - z64) / np.spacing(z64.astype(np.float32)).astype(np.float64)
    berr = np.abs(a["bary"][ok].astype(np.float64) - b["bary"][ok]).max(1)
    unit = 2.0 ** -24 * b["cond"][ok]
    print("z ulp", zerr.max(), "bary abs", berr.max(), "bary c", (berr / unit).max())
    assert zerr.max() <= 16
    assert (berr <= BARY_C * unit).all()


def test_restatement_is_quick():
    """A 256^2 frame of the template stays well under a second (the GPU tests lean on it)."""
    import time
    v, f = cs.template()
    tx, ty = cs.template_fov(256, 256)
    t = time.perf_counter()
    ref.rasterize(v, f, cs.template_camera(0.0, 22.0), tx, ty, 256, 256, np.float32)
    assert time.perf_counter() - t < 1.0


def test_header_and_exports():
    from guava_renderer_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gsr_mesh.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\*?\s+\**(gsr_[a-z_0-9]+)\s*\(", hdr, re.M))
    assert declared == {"gsr_mesh_raster_workspace_bytes", "gsr_mesh_raster", "gsr_mesh_visible_texels",
                        "gsr_mesh_raster_stats"}
    assert declared <= set(_lib.EXPORTS)
    assert "mesh_raster.hip" in build.SOURCES
    L = _lib.load()
    for s in declared:
        assert hasattr(L, s), s
    assert L.gsr_mesh_raster_workspace_bytes(2, 100, 50, 64, 48) > 2 * 64 * 48 * 8
    assert L.gsr_mesh_raster_workspace_bytes(0, 100, 50, 64, 48) == 0
    # bad arguments fail on the host before any launch (the pointers are never dereferenced)
    assert L.gsr_mesh_raster(1, 3, 1, 8, 8, None, 256, 256, 256, 256, 0, None, None, None, None, 256, None) == -1
    assert b"null" in L.gsr_last_error()
    assert L.gsr_mesh_raster(1, 3, 0, 8, 8, 256, 256, 256, 256, 256, 0, None, None, None, None, 256, None) == -1
    assert L.gsr_mesh_raster(65536, 3, 65536, 8, 8, 256, 256, 256, 256, 256, 1, None, None, None, None, 256,
                             None) == -1  # B*F >= 2^31
    assert L.gsr_mesh_visible_texels(1, 4, 4, None, 256, 256, None) == -1


def test_python_surface():
    """The module's names and the CPU-side refusals (no GPU needed: the checks come first)."""
    import torch
    from guava_renderer_amd import mesh_raster as mr
    assert mr.MeshFragments._fields == ("pix_to_face", "zbuf", "bary_coords", "face_visible", "texel_visible")
    assert mr.Fragments._fields == ("pix_to_face", "zbuf", "bary_coords", "dists")
    with pytest.raises(RuntimeError, match="GPU only"):
        mr.MeshRasterizer(torch.zeros((4, 3), dtype=torch.int32), 8, 8, 1, device="cpu")
    # visible_uv_mask is plain torch: the reference's isin / unique recipe on a small example
    F, B = 6, 2
    p2f = torch.tensor([[0, 3, -1, 3], [F + 5, -1, F + 1, F + 1]]).reshape(B, 2, 2, 1)
    idx = torch.tensor([[0, 1, 2], [3, 4, 5], [5, 0, 3]])
    mask = torch.tensor([[1.0, 1, 1], [1, 1, 0], [1, 0, 1]])
    all_faces = torch.arange(F)[None].repeat(B, 1) + (torch.arange(B) * F)[:, None]
    want = torch.isin(all_faces, torch.unique(p2f))[:, idx] * mask
    assert torch.equal(mr.visible_uv_mask(p2f, F, idx, mask), want)
