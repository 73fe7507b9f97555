"""CPU tests of the feature lifting's numpy restatement (tests/feature_lift_ref.py), the reference of
every GPU comparison in test_gpu_feature_lift.py, against torch:

 (a) sampling: the float32 restatement, evaluated at its own float32 pixel coordinates, against torch's
     float64 grid_sample fed those coordinates, in both padding modes.  Bound 8 * 2^-24 * max|feat|: an
     output takes at most six roundings that matter (two weight factors, the weight product, the tap
     product, and the adds), each relative to a value of at most max|feat|.
 (b) recipe: the reference's recipe (ubody_gaussian.py:75-114: homogeneous einsum, invtanfov, gathers
     through the permuted vertex tensor, grid_sample, mask, isin / unique over packed face ids) in
     float64, against the restatement: the bound of (a) plus (|d ix| + |d iy|) * (largest difference
     between the four taps), d the float32-against-float64 coordinate difference computed here
     (bilinear interpolation is continuous and its slope is bounded by the tap differences).
 (c) an affine map a*x + b*y + c is reproduced at interior samples.
 (d) the backward restatement (in float64) agrees with torch float64 autograd of the recipe.
 (e) the header's symbols are bound and built.
"""
import os
import re

import numpy as np
import torch

import feature_lift_cases as cs
import feature_lift_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
CASES = [c for c in cs.CASES if c[2] <= 35]  # (the C = 128 case has the geometry of the C = 1 case)


def _grid(ix, iy, W, H):
    """float64 grid_sample coordinates of pixel coordinates (align_corners=False)."""
    gx = (2.0 * ix.astype(np.float64) + 1.0) / W - 1.0
    gy = (2.0 * iy.astype(np.float64) + 1.0) / H - 1.0
    return torch.from_numpy(np.stack([gx, gy], -1))


def _grid_sample(feat, grid, mode):
    """feat [B,C,H,W] f64, grid [B,N,2] -> [B,N,C]."""
    out = torch.nn.functional.grid_sample(feat, grid[:, None], mode="bilinear", padding_mode=mode, align_corners=False)
    return out[:, :, 0].permute(0, 2, 1)


def _tap_span(feat_b, tp):
    """[N,C]: max - min over the four taps' values (0 for a tap outside the image)."""
    C, H, W = feat_b.shape
    flat = feat_b.reshape(C, H * W).astype(np.float64)
    vals = []
    for k in range(4):
        pix = np.where(tp["mask"][:, k], tp["ty"][:, k] * W + tp["tx"][:, k], 0)
        vals.append(np.where(tp["mask"][:, k][:, None], flat[:, pix].T, 0.0))
    vals = np.stack(vals)
    return vals.max(0) - vals.min(0)


def _case(W, H, C, U, cams):
    g = cs.geometry(W, H, U, cams)
    return g, cs.features(3, C, H, W, seed=W + C)


# ---- (a) ----

def test_sampling_against_grid_sample():
    worst = 0.0
    for W, H, C, U, cams in CASES:
        g, feat = _case(W, H, C, U, cams)
        f64 = torch.from_numpy(feat.astype(np.float64))
        bound = 8 * U24 * float(np.abs(feat).max())
        v = ref.lift_vertices(g["verts"], g["w2c"], g["tx"], g["ty"], feat)
        grid = torch.stack([_grid(t["ix"], t["iy"], W, H) for t in v["taps"]])
        err = np.abs(v["out"].astype(np.float64) - _grid_sample(f64, grid, "border").numpy())
        assert err.max() <= bound, (W, H, C, "border", err.max() / U24)
        worst = max(worst, err.max() / (U24 * np.abs(feat).max()))
        for vis in (None, g["face_visible"]):
            u = ref.lift_uv(g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], g["tx"], g["ty"], feat, vis)
            grid = torch.stack([_grid(t["ix"], t["iy"], W, H) for t in u["taps"]])
            want = _grid_sample(f64, grid, "zeros").numpy()
            for b in range(3):  # the zero rules of the UV path are not grid_sample's
                _, live = ref.uv_points(g["verts"][b], g["faces"], g["texel_face"], g["texel_bary"],
                                        None if vis is None else vis[b])
                want[b] *= live[:, None]
            err = np.abs(u["out"].astype(np.float64) - want.transpose(0, 2, 1))
            assert err.max() <= bound, (W, H, C, "zeros", err.max() / U24)
            worst = max(worst, err.max() / (U24 * np.abs(feat).max()))
    print("worst error / (2^-24 max|feat|):", worst)


# ---- (b) the reference recipe in float64 torch ----

def recipe_vertices(vertices, feature_map, w2c_cam, invtan):
    """sample_prj_feature (:75-83); invtan [B,2] = 1/tanfov per frame and axis (cfg.invtanfov in the
    reference, one number)."""
    homo = torch.cat([vertices, torch.ones_like(vertices[:, :, :1])], dim=-1)
    cam = torch.einsum("bij,bnj->bni", w2c_cam, homo)[:, :, :3]
    img = cam[:, :, :2] * invtan[:, None, :] / (cam[:, :, 2:] + 1e-7)
    s = torch.nn.functional.grid_sample(feature_map, img[:, None, :, :2], mode="bilinear", padding_mode="border",
                                        align_corners=False)
    return s.squeeze(-2).permute(0, 2, 1).contiguous(), img


def recipe_uv(img_features, deformed_vertices, w2c_cam, invtan, faces, uvmap_f_idx, uvmap_f_bary, uvmap_mask,
              visble_faces=None):
    """convert_pixel_feature_to_uv (:85-114)."""
    B = img_features.shape[0]
    bary = uvmap_f_bary[None].expand(B, -1, -1, -1)
    uv_vertex_id = faces[uvmap_f_idx]  # H W k
    uv_vertex = deformed_vertices.permute(1, 2, 0).contiguous()[uv_vertex_id]  # H W k 3 B
    uv_vertex = uv_vertex.permute(4, 0, 1, 2, 3).contiguous()  # B H W k 3
    uv_vertex = torch.einsum("bhwk,bhwkn->bhwn", bary, uv_vertex)
    homo = torch.cat([uv_vertex, torch.ones_like(uv_vertex[:, :, :, :1])], dim=-1)
    cam = torch.einsum("bij,bhwj->bhwi", w2c_cam, homo)[:, :, :, :3]
    img = cam[..., :2] * invtan[:, None, None, :] / (cam[..., 2:] + 1e-7)
    uv = torch.nn.functional.grid_sample(img_features, img, mode="bilinear", padding_mode="zeros", align_corners=False)
    mask = uvmap_mask.clone()[None].repeat(B, 1, 1)
    if visble_faces is not None:
        F = faces.shape[0]
        off = torch.arange(B, dtype=torch.int32) * F
        all_faces = torch.arange(0, F, dtype=torch.int32)[None].repeat(B, 1) + off[:, None]
        visible = torch.isin(all_faces, torch.unique(visble_faces))
        mask = mask * visible[:, uvmap_f_idx]
    return uv * mask[:, None], img


def _packed_visible(face_visible):
    """A stand-in for render_fragments' packed pix_to_face: b*F + f of every visible face, and -1."""
    B, F = face_visible.shape
    b, f = np.nonzero(face_visible)
    return torch.from_numpy(np.concatenate([[-1], b * F + f, [-1]]).astype(np.int64))


def _recipe_inputs(g, feat, U):
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))  # noqa: E731
    invtan = torch.stack([1.0 / t(g["tx"]), 1.0 / t(g["ty"])], 1)
    f_idx = torch.from_numpy(np.maximum(g["texel_face"], 0).astype(np.int64)).reshape(U, U)
    return dict(verts=t(g["verts"]), feat=t(feat), w2c=t(g["w2c"]), invtan=invtan,
                faces=torch.from_numpy(g["faces"].astype(np.int64)), f_idx=f_idx,
                bary=t(g["texel_bary"]).reshape(U, U, 3), mask=t(g["uvmap_mask"]).reshape(U, U))


def _pix(img, W, H):
    x = ((img[..., 0] + 1.0) * W - 1.0) * 0.5
    y = ((img[..., 1] + 1.0) * H - 1.0) * 0.5
    return x.numpy(), y.numpy()


def test_recipe_agrees_with_restatement():
    for W, H, C, U, cams in CASES:
        g, feat = _case(W, H, C, U, cams)
        r = _recipe_inputs(g, feat, U)
        base = 8 * U24 * float(np.abs(feat).max())
        # vertices
        want, img = recipe_vertices(r["verts"], r["feat"], r["w2c"], r["invtan"])
        got = ref.lift_vertices(g["verts"], g["w2c"], g["tx"], g["ty"], feat)
        x64, y64 = _pix(img, W, H)
        assert np.abs(got["ndc"].astype(np.float64) - img.numpy()).max() < 1e-4
        for b in range(3):
            tp = got["taps"][b]
            # border mode clamps: the clamped coordinates differ by no more than the raw ones
            dx = np.abs(np.clip(tp["ix"].astype(np.float64), 0, W - 1) - np.clip(x64[b], 0, W - 1))
            dy = np.abs(np.clip(tp["iy"].astype(np.float64), 0, H - 1) - np.clip(y64[b], 0, H - 1))
            t64 = ref.taps(x64[b], y64[b], W, H, True)
            span = np.maximum(_tap_span(feat[b], tp), _tap_span(feat[b], t64))
            err = np.abs(got["out"][b].astype(np.float64) - want[b].numpy())
            assert (err <= base + (dx + dy)[:, None] * span).all(), (W, H, C, "vertices", b, err.max())
        # UV, without and with the visibility term
        for vis in (None, g["face_visible"]):
            want, img = recipe_uv(r["feat"], r["verts"], r["w2c"], r["invtan"], r["faces"], r["f_idx"], r["bary"],
                                  r["mask"], None if vis is None else _packed_visible(vis))
            got = ref.lift_uv(g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], g["tx"], g["ty"],
                              feat, vis)
            x64, y64 = _pix(img.reshape(3, U * U, 2), W, H)
            want = want.reshape(3, C, U * U).numpy()
            kept = 0
            for b in range(3):
                tp = got["taps"][b]
                _, live = ref.uv_points(g["verts"][b], g["faces"], g["texel_face"], g["texel_bary"],
                                        None if vis is None else vis[b])
                dx = np.abs(tp["ix"].astype(np.float64) - x64[b])
                dy = np.abs(tp["iy"].astype(np.float64) - y64[b])
                t64 = ref.taps(x64[b], y64[b], W, H, False, live)
                span = np.maximum(_tap_span(feat[b], tp), _tap_span(feat[b], t64))
                err = np.abs(got["out"][b].T.astype(np.float64) - want[b].T)
                assert (err <= base + (dx + dy)[:, None] * span).all(), (W, H, C, "uv", b, err.max())
                assert (want[b].T[~live] == 0).all() and (got["out"][b].T[~live] == 0).all()
                kept += live.sum()
            assert kept > 0


# ---- (c) ----

def test_affine_map_is_reproduced():
    W, H, C, U, cams = cs.CASES[0]
    g = cs.geometry(W, H, U, cams)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    coef = np.array([[0.5, -0.25, 3.0], [-1.0, 0.125, 0.0], [0.0, 2.0, -7.0]], np.float32)
    feat = np.stack([a * x + b * y + c for a, b, c in coef])[None].repeat(3, 0).astype(np.float32)
    bound = 8 * U24 * float(np.abs(feat).max())
    got = ref.lift_uv(g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], g["tx"], g["ty"], feat)
    n = 0
    for b in range(3):
        tp = got["taps"][b]
        inner = tp["mask"].all(1)
        ix, iy = tp["ix"][inner].astype(np.float64), tp["iy"][inner].astype(np.float64)
        for c, (a, bb, cc) in enumerate(coef.astype(np.float64)):
            assert np.abs(got["out"][b, c][inner] - (a * ix + bb * iy + cc)).max() <= bound
        n += inner.sum()
    assert n > 500
    v = ref.lift_vertices(g["verts"], g["w2c"], g["tx"], g["ty"], feat)
    for b in range(3):
        tp = v["taps"][b]
        ix, iy = tp["ix"].astype(np.float64), tp["iy"].astype(np.float64)
        inner = (ix > 0) & (ix < W - 1) & (iy > 0) & (iy < H - 1)
        assert inner.sum() > 1000
        for c, (a, bb, cc) in enumerate(coef.astype(np.float64)):
            assert np.abs(v["out"][b][inner, c] - (a * ix + bb * iy + cc)[inner]).max() <= bound


# ---- (d) ----

def test_backward_against_autograd():
    for W, H, C, U, cams in CASES[:2]:
        g, feat = _case(W, H, C, U, cams)
        r = _recipe_inputs(g, feat, U)
        V = g["verts"].shape[1]
        fm = r["feat"].clone().requires_grad_(True)
        dv = cs.gradient((3, V, C), 1).astype(np.float64)
        out, _ = recipe_vertices(r["verts"], fm, r["w2c"], r["invtan"])
        out.backward(torch.from_numpy(dv))
        got = ref.lift_vertices_backward(g["verts"], g["w2c"], g["tx"], g["ty"], dv, C, W, H, dtype=np.float64)
        scale = np.abs(fm.grad.numpy()).max()
        assert scale > 0 and np.abs(got["dfeat"] - fm.grad.numpy()).max() <= 1e-9 * scale
        assert got["n"].sum() == sum(t["mask"].sum() for t in
                                     [f[0] for f in ref.vertex_taps(g["verts"], g["w2c"], g["tx"], g["ty"], W, H, np.float64)])
        for vis in (None, g["face_visible"]):
            fm = r["feat"].clone().requires_grad_(True)
            du = cs.gradient((3, C, U * U), 2).astype(np.float64)
            out, _ = recipe_uv(fm, r["verts"], r["w2c"], r["invtan"], r["faces"], r["f_idx"], r["bary"], r["mask"],
                               None if vis is None else _packed_visible(vis))
            out.backward(torch.from_numpy(du).reshape(3, C, U, U))
            got = ref.lift_uv_backward(g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], g["tx"], g["ty"],
                                       du, W, H, vis, dtype=np.float64)
            scale = np.abs(fm.grad.numpy()).max()
            assert scale > 0 and np.abs(got["dfeat"] - fm.grad.numpy()).max() <= 1e-9 * scale
            assert (got["S"] >= np.abs(got["dfeat"]) - 1e-12).all() and (got["n"] >= 0).all()


# ---- (e) ----

def test_lift_symbols_are_bound_and_built():
    """Every symbol include/gsr_lift.h declares is in _lib.EXPORTS with argtypes, and lift.hip is built."""
    from guava_renderer_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gsr_lift.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\*?\s+\**(gsr_[a-z_0-9]+)\s*\(", hdr, re.M))
    assert declared == {"gsr_lift_vertices", "gsr_lift_uv", "gsr_lift_backward_workspace_bytes",
                        "gsr_lift_vertices_backward", "gsr_lift_uv_backward"}
    assert declared <= set(_lib.EXPORTS)
    assert "lift.hip" in build.SOURCES
    L = _lib.load()
    for sym in declared:
        assert getattr(L, sym).argtypes is not None, sym
    # sizes: the scratch is one channels-last copy of the map; bad sizes give 0 / GSR_ERR_ARG without a device
    assert L.gsr_lift_backward_workspace_bytes(2, 35, 512, 512) >= 2 * 35 * 512 * 512 * 4
    assert L.gsr_lift_backward_workspace_bytes(1, 1, 16385, 4) == 0
    assert L.gsr_lift_backward_workspace_bytes(64, 128, 512, 512) == 0  # B*C*H*W >= 2^31
    assert L.gsr_lift_vertices(1, 4, 3, 8, 8, None, None, None, None, None, None, None, None) == -1
    assert b"null" in L.gsr_last_error()
    assert L.gsr_lift_uv(1, 4, 2, 0, 3, 8, 8, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"bad sizes" in L.gsr_last_error()


def test_no_cpu_path():
    import pytest
    from guava_renderer_amd.feature_lift import FeatureLifter
    with pytest.raises(RuntimeError, match="GPU only"):
        FeatureLifter(np.zeros((1, 3), np.int32), np.zeros((2, 2), np.int64), np.zeros((2, 2, 3), np.float32),
                      np.ones((2, 2), np.float32), device="cpu")
