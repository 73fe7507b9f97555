"""GPU tests of the mesh visibility rasterizer (include/gsr_mesh.h, csrc/mesh_raster.hip,
guava_renderer_amd/mesh_raster.py).

Reference of every comparison: the float32 evaluation of tests/mesh_raster_ref.py, which states the
kernel's arithmetic op for op; equality means np.array_equal on pix_to_face, the bits of zbuf and
bary, and face_visible (test_mesh_raster_ref.py judges that float32 evaluation against float64).

Calls through the C ABI (_abi) poison every output buffer and the whole workspace first and check
afterwards that no output element kept its poison.  (Of the workspace only the counters are checked:
the worklist behind its length and the slabs' padding are legitimately never written.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_raster_cases as cs
import mesh_raster_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON_I32 = 0x5A5A5A5A
POISON_U8 = 0xA5


def _ptr(t):
    return None if t is None else t.data_ptr()


def _abi(verts, faces, w2c, tx, ty, W, H, packed=False, ws_batch=None):
    """gsr_mesh_raster on poisoned buffers -> dict of numpy results + stats."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    B, V = verts.shape[:2]
    F = faces.shape[0]
    tx = np.broadcast_to(np.asarray(tx, np.float32), (B,)).copy()
    ty = np.broadcast_to(np.asarray(ty, np.float32), (B,)).copy()
    d = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    dv, df, dm, dtx, dty = d(verts), d(faces), d(w2c), d(tx), d(ty)
    n_ws = L.gsr_mesh_raster_workspace_bytes(ws_batch or B, V, F, W, H)
    assert n_ws > 0
    ws = torch.full((n_ws,), POISON_U8, dtype=torch.uint8, device=DEV)
    p2f = torch.full((B, H, W), POISON_I32, dtype=torch.int32, device=DEV)
    zbuf = torch.full((B, H, W), float("nan"), device=DEV)
    bary = torch.full((B, H, W, 3), float("nan"), device=DEV)
    vis = torch.full((B, F), POISON_U8, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.gsr_mesh_raster(B, V, F, W, H, _ptr(dv), _ptr(df), _ptr(dm), _ptr(dtx), _ptr(dty), int(packed),
                                 _ptr(p2f), _ptr(zbuf), _ptr(bary), _ptr(vis), _ptr(ws), stream), "gsr_mesh_raster")
    torch.cuda.synchronize()
    st = (ctypes.c_int64 * 4)()
    _lib.check(L.gsr_mesh_raster_stats(_ptr(ws), st), "gsr_mesh_raster_stats")
    out = dict(pix_to_face=p2f.cpu().numpy(), zbuf=zbuf.cpu().numpy(), bary=bary.cpu().numpy(),
               face_visible=vis.cpu().numpy(), stats=tuple(int(x) for x in st))
    assert (out["pix_to_face"] != POISON_I32).all()
    assert not np.isnan(out["zbuf"]).any() and not np.isnan(out["bary"]).any()
    assert (out["face_visible"] <= 1).all()
    assert sum(out["stats"][:3]) == B * F and out["stats"][3] <= B * H * W  # (the poison would be 0xA5A5A5A5)
    return out


def _assert_equal(got, want, packed_F=None):
    p = want["pix_to_face"]
    if packed_F:
        off = (np.arange(p.shape[0], dtype=np.int32) * packed_F).reshape(-1, 1, 1)
        p = np.where(p >= 0, p + off, -1).astype(np.int32)
    assert np.array_equal(got["pix_to_face"], p)
    assert np.array_equal(got["zbuf"].view(np.uint32), want["zbuf"].astype(np.float32).view(np.uint32))
    assert np.array_equal(got["bary"].view(np.uint32), want["bary"].astype(np.float32).view(np.uint32))
    assert np.array_equal(got["face_visible"], want["face_visible"])
    if "stats" in got and "stats" in want:
        assert got["stats"] == want["stats"]


TEMPLATE_CAMS = ((0.0, 22.0), (2.5, 22.0), (0.3, 4.0))


@functools.lru_cache(maxsize=None)
def _template_case(W, H):
    """(verts, faces, w2c, tx, ty, float32 reference) of the B = 3 template batch, made once."""
    verts, w2c = cs.posed_batch(TEMPLATE_CAMS, seed=3)
    _, faces = cs.template()
    tx, ty = cs.template_fov(W, H)
    tx = np.float32(tx) * np.array([1.0, 1.05, 1.0], np.float32)  # per-frame values
    ty = np.float32(ty) * np.array([1.0, 1.0, 0.95], np.float32)
    want = ref.rasterize_batch(verts, faces, w2c, tx, ty, W, H)
    for a in (verts, w2c, tx, ty):
        a.setflags(write=False)
    return verts, faces, w2c, tx, ty, want


@pytest.mark.parametrize("W,H", [(96, 64), (128, 128)])
def test_template_batch(W, H):
    """Template mesh, B = 3, per-frame posed vertices and cameras; 96x64 with unequal tanfovx/tanfovy.
    The counters equal the restatement's, whose per-frame split shows the distance-4 frame on the wide
    path and the distance-22 frames on the per-lane path."""
    verts, faces, w2c, tx, ty, want = _template_case(W, H)
    assert tx[0] != ty[0] or W == H
    fs = want["frame_stats"]
    assert fs[2][1] > 0 and fs[0][0] > 20000 and fs[1][0] > 20000 and fs[0][3] > 500 and fs[1][3] > 500
    got = _abi(verts, faces, w2c, tx, ty, W, H)
    print("stats", got["stats"], "per frame", fs)
    _assert_equal(got, want)
    assert got["stats"][1] >= fs[2][1] > 0 and got["stats"][0] > 40000


@pytest.mark.parametrize("W,H", [(32, 24), (8, 8)])
def test_hand_scene(W, H):
    """cs.hand_scene (edge rule on exact integer coordinates, interpenetrating triangles, duplicate,
    culled faces, a triangle larger than the image, a sub-pixel triangle), plus a shifted second frame."""
    v, f = cs.hand_scene(W, H)
    verts = np.stack([v, v + np.array([0.013, -0.007, 0.05], np.float32)]).astype(np.float32)
    w2c = np.stack([cs.EYE, cs.EYE])
    want = ref.rasterize_batch(verts, f, w2c, cs.TANFOV_EXACT, cs.TANFOV_EXACT, W, H)
    got = _abi(verts, f, w2c, cs.TANFOV_EXACT, cs.TANFOV_EXACT, W, H)
    _assert_equal(got, want)
    n_lane, n_wide, n_cull, covered = got["stats"]
    assert n_wide >= 6 and n_cull >= 3 and n_lane >= 2 and covered == 2 * W * H
    vis = dict(zip(cs.HAND_FACES, got["face_visible"][0]))
    assert vis["dup_0"] == 1 and vis["dup_1"] == 0 and vis["subpixel"] == 0 and vis["huge"] == 1
    # frame 0: the shared diagonal's centres show a face behind, never the edge pair
    hi = cs.EDGE_HI[H]
    for p in range(1, hi + 1):
        assert got["pix_to_face"][0, p, p] not in (0, 1)


def test_frame_behind_camera():
    """B = 4 with frame 2 entirely behind its camera: all -1 and nothing visible there; the other
    frames equal the single-frame calls on the same inputs."""
    W = H = 64
    cams = ((0.0, 22.0), (0.7, 22.0), (0.0, 22.0), (2.5, 22.0))
    verts, w2c = cs.posed_batch(cams, seed=5)
    w2c = w2c.copy()
    w2c[2, 2] = -w2c[2, 2]  # zv < 0 for every vertex
    _, faces = cs.template()
    tx, ty = cs.template_fov(W, H)
    got = _abi(verts, faces, w2c, tx, ty, W, H)
    assert (got["pix_to_face"][2] == -1).all() and (got["zbuf"][2] == -1).all() and (got["bary"][2] == -1).all()
    assert not got["face_visible"][2].any()
    covered = 0
    for b in (0, 1, 3):
        one = _abi(verts[b:b + 1], faces, w2c[b:b + 1], tx, ty, W, H)
        for k in ("pix_to_face", "zbuf", "bary", "face_visible"):
            assert np.array_equal(got[k][b].view(np.uint8), one[k][0].view(np.uint8)), (b, k)
        assert one["stats"][3] > 500
        covered += one["stats"][3]
    assert got["stats"][3] == covered and got["stats"][2] >= faces.shape[0]
    _assert_equal(got, ref.rasterize_batch(verts, faces, w2c, tx, ty, W, H))


def _frag_bytes(fr):
    return [t.cpu().numpy().view(np.uint8).copy() for t in fr[:4]]


def test_repeatable_and_workspace_reuse():
    """Two calls are bit-equal; so is a rasterizer with max_batch > B, and a call after one at another
    B and after the workspace was overwritten (no state survives a call)."""
    from guava_renderer_amd.mesh_raster import MeshRasterizer
    W, H = 96, 64
    verts, faces, w2c, tx, ty, want = _template_case(W, H)
    dv, dm = torch.from_numpy(np.array(verts)).to(DEV), torch.from_numpy(np.array(w2c)).to(DEV)
    dtx, dty = torch.from_numpy(np.array(tx)).to(DEV), torch.from_numpy(np.array(ty)).to(DEV)
    r3, r7 = MeshRasterizer(faces, W, H, 3, DEV), MeshRasterizer(faces, W, H, 7, DEV)
    first = _frag_bytes(r3(dv, dm, dtx, dty))
    assert r3.stats() == dict(zip(("lane_faces", "wide_faces", "culled_faces", "covered_pixels"), want["stats"]))
    second = _frag_bytes(r3(dv, dm, dtx, dty))
    wide = _frag_bytes(r7(dv, dm, dtx, dty))
    r7(dv[:1], dm[:1], dtx[:1], dty[:1])  # another B on the same workspace
    r7._ws.fill_(POISON_U8)
    again = _frag_bytes(r7(dv, dm, dtx, dty))
    for other in (second, wide, again):
        for a, b in zip(first, other):
            assert np.array_equal(a, b)
    assert np.array_equal(first[0].view(np.int32).reshape(3, H, W), want["pix_to_face"])


@functools.lru_cache(maxsize=None)
def _mirror_case():
    verts, w2c = cs.posed_batch(((0.0, 22.0), (0.7, 22.0)), seed=7)
    _, faces = cs.template()
    want = ref.rasterize_batch(verts, faces, w2c, 1.0 / 24.0, 1.0 / 24.0, 64, 64)
    return verts, faces, w2c, want


def test_render_fragments_mirror():
    """BaseMeshRenderer.render_fragments: the reference's shapes, dtypes and packed indices f + b*F;
    dists is None; reverse_camera=False equals the call with rows 0 and 1 negated; a [B,3,4] matrix is
    accepted; a batch beyond max_batch grows the rasterizer as the reference takes any batch."""
    from guava_renderer_amd.mesh_raster import BaseMeshRenderer, MeshRasterizer
    verts, faces, w2c, want = _mirror_case()
    B, F = 2, faces.shape[0]
    dv, dm = torch.from_numpy(verts).to(DEV), torch.from_numpy(w2c).to(DEV)
    rend = BaseMeshRenderer(faces, image_size=64, focal_length=24, max_batch=1, device=DEV)
    p2f, frag = rend.render_fragments(dv, transform_matrix=dm)
    assert p2f.shape == (B, 64, 64, 1) and p2f.dtype == torch.int64 and frag.pix_to_face is p2f
    assert frag.zbuf.shape == (B, 64, 64, 1) and frag.zbuf.dtype == torch.float32
    assert frag.bary_coords.shape == (B, 64, 64, 1, 3) and frag.dists is None
    got = dict(pix_to_face=p2f[..., 0].cpu().numpy().astype(np.int32), zbuf=frag.zbuf[..., 0].cpu().numpy(),
               bary=frag.bary_coords[:, :, :, 0].cpu().numpy(), face_visible=want["face_visible"])
    _assert_equal(got, want, packed_F=F)
    assert got["pix_to_face"][1].max() >= F  # frame 1 really carries its offset
    p34, _ = rend.render_fragments(dv, transform_matrix=dm[:, :3])
    assert torch.equal(p34, p2f)
    # reverse_camera=False
    neg = dm.clone()
    neg[:, :2] = -neg[:, :2]
    pf, ff = rend.render_fragments(dv, transform_matrix=dm, reverse_camera=False)
    direct = MeshRasterizer(faces, 64, 64, B, DEV)(dv, neg, 1.0 / 24.0, 1.0 / 24.0, packed=True)
    assert torch.equal(pf[..., 0], direct.pix_to_face.long()) and torch.equal(ff.zbuf[..., 0], direct.zbuf)
    assert torch.equal(ff.bary_coords[:, :, :, 0], direct.bary_coords)
    wneg = ref.rasterize_batch(verts, faces, neg.cpu().numpy(), 1.0 / 24.0, 1.0 / 24.0, 64, 64)
    assert np.array_equal(direct.face_visible.cpu().numpy(), wneg["face_visible"]) and wneg["stats"][3] > 500
    assert not torch.equal(pf, p2f)
    # a non-square image: the shorter side spans NDC [-1, 1]
    r2 = BaseMeshRenderer(faces, image_size=(48, 64), focal_length=24, max_batch=B, device=DEV)
    assert r2.tanfovx == pytest.approx((64 / 48) / 24) and r2.tanfovy == pytest.approx(1 / 24)
    p, _ = r2.render_fragments(dv, transform_matrix=dm)
    w2 = ref.rasterize_batch(verts, faces, w2c, r2.tanfovx, r2.tanfovy, 64, 48)
    assert p.shape == (B, 48, 64, 1) and np.array_equal(p[0, :, :, 0].cpu().numpy(), w2["pix_to_face"][0])


def test_visible_uv_mask_and_texels():
    """visible_uv_mask equals the reference's isin / unique recipe (ubody_gaussian.py:102-111) on a
    synthetic 64^2 uvmap_f_idx; texel_visible equals face_visible[:, binding_face] for the avatar
    assets' binding_face."""
    from guava_renderer_amd import avatar
    from guava_renderer_amd.mesh_raster import BaseMeshRenderer, MeshRasterizer, visible_uv_mask
    verts, faces, w2c, want = _mirror_case()
    B, F = 2, faces.shape[0]
    dv, dm = torch.from_numpy(verts).to(DEV), torch.from_numpy(w2c).to(DEV)
    rend = BaseMeshRenderer(faces, image_size=64, focal_length=24, max_batch=B, device=DEV)
    p2f, _ = rend.render_fragments(dv, transform_matrix=dm)
    g = torch.Generator().manual_seed(0)
    # half of the texels on faces that frame 0 sees, so the mask is neither empty nor full
    seen = torch.from_numpy(np.nonzero(want["face_visible"][0])[0])
    idx = torch.where(torch.rand((64, 64), generator=g) < 0.5, seen[torch.randint(0, len(seen), (64, 64), generator=g)],
                      torch.randint(0, F, (64, 64), generator=g)).to(DEV)
    mask = (torch.rand((64, 64), generator=g) < 0.8).float().to(DEV)
    all_faces = torch.arange(F, device=DEV, dtype=torch.int32)[None].repeat(B, 1)
    all_faces = all_faces + (torch.arange(B, device=DEV, dtype=torch.int32) * F)[:, None]
    recipe = torch.isin(all_faces, torch.unique(p2f))[:, idx] * mask
    got = visible_uv_mask(p2f, F, idx, mask)
    assert got.shape == (B, 64, 64) and torch.equal(got, recipe)
    assert 0.2 < got.mean().item() < 0.8
    tv, tf, tc = avatar.template_mesh()
    bind = avatar.gaussians(tv, tf, tc, P=30000, seed=0)["binding_face"]
    fr = MeshRasterizer(faces, 64, 64, B, DEV)(dv, dm, 1.0 / 24.0, 1.0 / 24.0,
                                                 binding_face=torch.from_numpy(bind).to(DEV))
    assert fr.texel_visible.shape == (B, bind.shape[0]) and fr.texel_visible.dtype == torch.uint8
    assert np.array_equal(fr.face_visible.cpu().numpy(), want["face_visible"])
    assert np.array_equal(fr.texel_visible.cpu().numpy(), want["face_visible"][:, bind])
    assert 0 < fr.texel_visible.sum().item() < fr.texel_visible.numel()


def test_arguments():
    from guava_renderer_amd import _lib
    from guava_renderer_amd.mesh_raster import BaseMeshRenderer, MeshRasterizer
    verts, faces, w2c, _ = _mirror_case()
    dv, dm = torch.from_numpy(verts).to(DEV), torch.from_numpy(w2c).to(DEV)
    r = MeshRasterizer(faces, 16, 16, 1, DEV)
    with pytest.raises(RuntimeError, match="GPU only"):
        r(torch.from_numpy(verts[:1]), dm[:1], 0.1, 0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        r(dv[:1], torch.from_numpy(w2c[:1]), 0.1, 0.1)
    with pytest.raises(RuntimeError, match="num_faces, 3"):
        MeshRasterizer(faces.reshape(-1, 4), 16, 16, 1, DEV)
    with pytest.raises(RuntimeError, match="outside this rasterizer"):
        r(dv, dm, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="num_verts, 3"):
        r(dv[:1, :, :2], dm[:1], 0.1, 0.1)
    with pytest.raises(RuntimeError, match="vertices"):
        r(dv[:1, :100], dm[:1], 0.1, 0.1)
    with pytest.raises(RuntimeError, match="one value per frame"):
        r(dv[:1], dm[:1], [0.1, 0.2], 0.1)
    with pytest.raises(NotImplementedError, match="cameras"):
        BaseMeshRenderer(faces, 16, 24, 1, DEV).render_fragments(dv[:1], cameras=object(), transform_matrix=dm[:1])
    # the C entry: a null vertex pointer is refused before any launch -- the outputs keep their poison
    L = _lib.load()
    F, V = faces.shape[0], verts.shape[1]
    ws = torch.full((L.gsr_mesh_raster_workspace_bytes(1, V, F, 16, 16),), POISON_U8, dtype=torch.uint8, device=DEV)
    p2f = torch.full((1, 16, 16), POISON_I32, dtype=torch.int32, device=DEV)
    vis = torch.full((1, F), POISON_U8, dtype=torch.uint8, device=DEV)
    df = torch.from_numpy(np.array(faces)).to(DEV)
    fov = torch.full((1,), 0.1, device=DEV)
    rc = L.gsr_mesh_raster(1, V, F, 16, 16, None, df.data_ptr(), dm.data_ptr(), fov.data_ptr(), fov.data_ptr(), 0,
                           p2f.data_ptr(), None, None, vis.data_ptr(), ws.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"null" in L.gsr_last_error()
    assert (p2f == POISON_I32).all() and (vis == POISON_U8).all() and (ws == POISON_U8).all()
    assert L.gsr_mesh_raster(1, V, F, 0, 16, dv.data_ptr(), df.data_ptr(), dm.data_ptr(), fov.data_ptr(),
                             fov.data_ptr(), 0, p2f.data_ptr(), None, None, None, ws.data_ptr(), None) == -1
    assert (p2f == POISON_I32).all()


def test_full_size():
    """Template mesh at 512^2, B = 2: equality with the float32 restatement."""
    W = H = 512
    verts, w2c = cs.posed_batch(((0.0, 22.0), (0.7, 22.0)), seed=11)
    _, faces = cs.template()
    want = ref.rasterize_batch(verts, faces, w2c, 1.0 / 24.0, 1.0 / 24.0, W, H)
    got = _abi(verts, faces, w2c, 1.0 / 24.0, 1.0 / 24.0, W, H, packed=True)
    print("stats", got["stats"])
    _assert_equal(got, want, packed_F=faces.shape[0])
    assert got["stats"][3] > 40000
