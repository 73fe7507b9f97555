"""GPU tests of the feature lifting (include/gsr_lift.h, csrc/lift.hip, guava_renderer_amd/feature_lift.py).

Reference of every comparison: the float32 evaluation of tests/feature_lift_ref.py, which states the
kernels' arithmetic op for op (test_feature_lift_ref.py judges it against torch in float64).
  forward   np.array_equal on the bits, for both entries and for ndc.
  backward  float atomic sums have no fixed order, so per feature-map pixel and channel
            |dfeat - float64 sum| <= (n + 2) * 2^-24 * S,  n the taps on the pixel, S the sum of
            |w*dout| over them: any order of n float32 adds stays within (n - 1) * 2^-24 * S of the exact
            sum of the float32 products, and the rest covers the final rounding.  A pixel that no tap
            reaches must be exactly 0.

Calls through the C ABI (_abi_*) poison every output (a NaN with its own payload) and the whole
workspace first and check afterwards that no output element kept the poison's bits.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import feature_lift_cases as cs
import feature_lift_ref as ref
import mesh_raster_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON_F32 = 0x7FC5A5A5  # a quiet NaN no computation produces
POISON_U8 = 0xA5
U24 = 2.0 ** -24


def _d(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _poisoned(shape):
    return torch.full(shape, POISON_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def _clean(t):
    a = t.cpu().numpy()
    assert not (a.view(np.uint32) == POISON_F32).any(), "an output element kept its poison"
    return a


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fov(t, B):
    return _d(np.broadcast_to(np.asarray(t, np.float32), (B,)).copy())


def _abi_vertices(verts, w2c, tx, ty, feat, want_ndc=True):
    from guava_renderer_amd import _lib
    L = _lib.load()
    B, V = verts.shape[:2]
    C, H, W = feat.shape[1:]
    out, ndc = _poisoned((B, V, C)), (_poisoned((B, V, 2)) if want_ndc else None)
    t = [_d(verts), _d(w2c), _fov(tx, B), _fov(ty, B), _d(feat)]
    _lib.check(L.gsr_lift_vertices(B, V, C, W, H, *[_ptr(x) for x in t], _ptr(out), _ptr(ndc), _stream()),
               "gsr_lift_vertices")
    torch.cuda.synchronize()
    return _clean(out), (_clean(ndc) if want_ndc else None)


def _abi_uv(g, tx, ty, feat, vis):
    from guava_renderer_amd import _lib
    L = _lib.load()
    B, V = g["verts"].shape[:2]
    C, H, W = feat.shape[1:]
    F, T = g["faces"].shape[0], g["texel_face"].shape[0]
    out = _poisoned((B, C, T))
    t = [_d(g["verts"]), _d(g["faces"]), _d(g["texel_face"]), _d(g["texel_bary"]), _d(g["w2c"]), _fov(tx, B), _fov(ty, B),
         _d(feat), None if vis is None else _d(vis)]
    _lib.check(L.gsr_lift_uv(B, V, F, T, C, W, H, *[_ptr(x) for x in t], _ptr(out), _stream()), "gsr_lift_uv")
    torch.cuda.synchronize()
    return _clean(out)


def _ws(B, C, W, H):
    from guava_renderer_amd import _lib
    n = _lib.load().gsr_lift_backward_workspace_bytes(B, C, W, H)
    assert n >= B * C * W * H * 4
    return torch.full((n,), POISON_U8, dtype=torch.uint8, device=DEV)


def _abi_vertices_bwd(verts, w2c, tx, ty, dout, W, H, ws=None):
    from guava_renderer_amd import _lib
    L = _lib.load()
    B, V, C = dout.shape
    ws = _ws(B, C, W, H) if ws is None else ws
    dfeat = _poisoned((B, C, H, W))
    t = [_d(verts), _d(w2c), _fov(tx, B), _fov(ty, B), _d(dout)]
    _lib.check(L.gsr_lift_vertices_backward(B, V, C, W, H, *[_ptr(x) for x in t], _ptr(dfeat), _ptr(ws), _stream()),
               "gsr_lift_vertices_backward")
    torch.cuda.synchronize()
    return _clean(dfeat)


def _abi_uv_bwd(g, tx, ty, dout, W, H, vis, ws=None):
    from guava_renderer_amd import _lib
    L = _lib.load()
    B, V = g["verts"].shape[:2]
    C = dout.shape[1]
    F, T = g["faces"].shape[0], g["texel_face"].shape[0]
    ws = _ws(B, C, W, H) if ws is None else ws
    dfeat = _poisoned((B, C, H, W))
    t = [_d(g["verts"]), _d(g["faces"]), _d(g["texel_face"]), _d(g["texel_bary"]), _d(g["w2c"]), _fov(tx, B), _fov(ty, B),
         None if vis is None else _d(vis), _d(dout)]
    _lib.check(L.gsr_lift_uv_backward(B, V, F, T, C, W, H, *[_ptr(x) for x in t], _ptr(dfeat), _ptr(ws), _stream()),
               "gsr_lift_uv_backward")
    torch.cuda.synchronize()
    return _clean(dfeat)


def _bits_equal(got, want):
    want = np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _assert_backward(got, want, what):
    """want: feature_lift_ref.scatter()'s dict."""
    bound = (want["n"][:, None].astype(np.float64) + 2.0) * U24 * want["S"]
    err = np.abs(got.astype(np.float64) - want["dfeat"])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(what, "worst error / bound:", worst, "max taps", int(want["n"].max()))
    assert (err <= bound).all(), (what, worst)
    assert (got[np.broadcast_to(want["n"][:, None] == 0, got.shape)] == 0).all()


@functools.lru_cache(maxsize=None)
def _seeded(i):
    """Inputs and float32 reference of seeded case i, made once and left unchanged."""
    W, H, C, U, cams = cs.CASES[i]
    g = cs.geometry(W, H, U, cams)
    B, V = g["verts"].shape[:2]
    feat = cs.features(B, C, H, W, seed=10 + i)
    dv, du = cs.gradient((B, V, C), 20 + i), cs.gradient((B, C, U * U), 30 + i)
    a = (g["verts"], g["w2c"], g["tx"], g["ty"])
    uv = (g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], g["tx"], g["ty"])
    want = dict(vert=ref.lift_vertices(*a, feat), uv=ref.lift_uv(*uv, feat, g["face_visible"]),
                uv_all=ref.lift_uv(*uv, feat, None),
                vert_bwd=ref.lift_vertices_backward(*a, dv, C, W, H),
                uv_bwd=ref.lift_uv_backward(*uv, du, W, H, g["face_visible"]))
    for x in (feat, dv, du):
        x.setflags(write=False)
    return g, feat, dv, du, want


@pytest.mark.parametrize("i", range(len(cs.CASES)), ids=[f"{c[0]}x{c[1]}-C{c[2]}-U{c[3]}" for c in cs.CASES])
def test_seeded_case(i):
    """B = 3, per-frame vertices, cameras and tanfov (unequal tanfovx / tanfovy at 96x64)."""
    W, H, C, U, cams = cs.CASES[i]
    g, feat, dv, du, want = _seeded(i)
    # what the case must contain, on the restatement alone
    s = cs.shares(g, W, H)
    print(s)
    assert g["verts"].shape[0] == 3 and len(set(g["tx"])) > 1 and len(set(g["ty"])) > 1
    assert s["masked"] >= 0.20 and 0.20 <= s["visible"] <= 0.80
    assert s["uv_outside"] >= 0.02 and s["vertex_outside"] >= 0.02 and s["partial"] >= 0.002 and s["max_taps"] >= 6
    assert W == H or g["tx"][0] != g["ty"][0]
    assert want["uv"]["out"].any() and not np.array_equal(want["uv"]["out"], want["uv_all"]["out"])
    # forward
    out, ndc = _abi_vertices(g["verts"], g["w2c"], g["tx"], g["ty"], feat)
    assert _bits_equal(out, want["vert"]["out"]) and _bits_equal(ndc, want["vert"]["ndc"])
    assert _bits_equal(_abi_uv(g, g["tx"], g["ty"], feat, g["face_visible"]), want["uv"]["out"])
    assert _bits_equal(_abi_uv(g, g["tx"], g["ty"], feat, None), want["uv_all"]["out"])
    # backward
    _assert_backward(_abi_vertices_bwd(g["verts"], g["w2c"], g["tx"], g["ty"], dv, W, H), want["vert_bwd"], "vertices")
    _assert_backward(_abi_uv_bwd(g, g["tx"], g["ty"], du, W, H, g["face_visible"]), want["uv_bwd"], "uv")


def _hand(W=16, H=8):
    """Samples on exact pixel coordinates (w2c = I, tanfov = 0.5, z = 2: mesh_raster_cases.pixel_verts):
    pixel centres, ix = -1, -0.5, W-1, W-0.5, W, the four corners and two points beyond a corner, plus
    one NaN vertex.  UV path: face i = (i, i, i) with barycentrics (1, 0, 0) is vertex i exactly; then
    a face with a vertex index >= V, and texels bound to face F, INT_MAX, -1 and -5."""
    pts = [(3, 2), (5, 6), (-1, 2), (-0.5, 2), (W - 1, 3), (W - 0.5, 3), (W, 3), (0, 0), (W - 1, 0), (0, H - 1),
           (W - 1, H - 1), (-0.5, -0.5), (W - 0.5, H - 0.5), (6.5, 1.5), (2, -1), (2, H)]
    v = mc.pixel_verts([(x, y, 2.0) for x, y in pts], W, H)
    v = np.concatenate([v, np.array([[np.nan, 0.1, 2.0]], np.float32)])
    V = v.shape[0]
    faces = np.array([[i, i, i] for i in range(V)] + [[0, 1, V], [0, -1, 1]], np.int32)
    F = faces.shape[0]
    tf = np.array(list(range(F)) + [F, 2 ** 31 - 1, -1, -5], np.int32)
    tb = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (tf.shape[0], 1))
    g = dict(verts=np.stack([v, v]), faces=faces, texel_face=tf, texel_bary=tb, w2c=np.stack([mc.EYE, mc.EYE]))
    return g, pts, V, F


def test_hand_case():
    W, H, C = 16, 8, 3
    g, pts, V, F = _hand(W, H)
    fov = mc.TANFOV_EXACT
    feat = cs.features(2, C, H, W, seed=5) + 2.0
    a = (g["verts"], g["w2c"], fov, fov)
    uvargs = (g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], fov, fov)
    wv, wu = ref.lift_vertices(*a, feat), ref.lift_uv(*uvargs, feat)
    # the restatement is where the docstring says it is
    tp = wv["taps"][0]
    assert np.array_equal(tp["ix"][:len(pts)], np.array([p[0] for p in pts], np.float32))
    assert np.array_equal(tp["iy"][:len(pts)], np.array([p[1] for p in pts], np.float32))
    f0 = feat[0]
    border, zeros = wv["out"][0], wu["out"][0].T
    assert np.array_equal(border[0], f0[:, 2, 3]) and np.array_equal(zeros[0], f0[:, 2, 3])  # a pixel centre
    assert np.array_equal(border[2], f0[:, 2, 0]) and not zeros[2].any()                      # ix = -1
    assert np.array_equal(border[3], f0[:, 2, 0]) and np.array_equal(zeros[3], np.float32(0.5) * f0[:, 2, 0])
    assert np.array_equal(zeros[4], f0[:, 3, W - 1])                                          # ix = W - 1
    assert np.array_equal(zeros[5], np.float32(0.5) * f0[:, 3, W - 1]) and not zeros[6].any()  # W - 0.5, W
    assert np.array_equal(zeros[10], f0[:, H - 1, W - 1])                                     # a corner
    assert np.array_equal(zeros[11], np.float32(0.25) * f0[:, 0, 0])                          # beyond a corner
    assert np.array_equal(border[12], f0[:, H - 1, W - 1]) and not zeros[14].any() and not zeros[15].any()
    nanv = V - 1
    assert not border[nanv].any() and not zeros[nanv].any()           # the NaN vertex
    assert not zeros[F - 2].any() and not zeros[F - 1].any()          # a vertex index >= V, and one < 0
    assert not zeros[F:].any()                                        # faces F, INT_MAX, -1, -5
    # the GPU
    out, ndc = _abi_vertices(*a, feat)
    assert _bits_equal(out, wv["out"])
    nn = ~np.isnan(wv["ndc"])  # (the NaN vertex's ndc is NaN on both sides; a NaN's bits are not pinned)
    assert np.array_equal(np.isnan(ndc), ~nn) and np.array_equal(ndc[nn].view(np.uint32), wv["ndc"][nn].view(np.uint32))
    gu = _abi_uv(g, fov, fov, feat, None)
    assert _bits_equal(gu, wu["out"])
    ones = np.ones((2, F), np.uint8)
    assert _bits_equal(_abi_uv(g, fov, fov, feat, ones), wu["out"])
    some = ones.copy()
    some[1, :5] = 0
    assert _bits_equal(_abi_uv(g, fov, fov, feat, some), ref.lift_uv(*uvargs, feat, some)["out"])
    # backward at the same samples
    dv, du = cs.gradient((2, V, C), 1), cs.gradient((2, C, g["texel_face"].shape[0]), 2)
    _assert_backward(_abi_vertices_bwd(*a, dv, W, H), ref.lift_vertices_backward(*a, dv, C, W, H), "hand vertices")
    _assert_backward(_abi_uv_bwd(g, fov, fov, du, W, H, None), ref.lift_uv_backward(*uvargs, du, W, H), "hand uv")
    _assert_backward(_abi_uv_bwd(g, fov, fov, du, W, H, some), ref.lift_uv_backward(*uvargs, du, W, H, some),
                     "hand uv, visibility")


def test_frame_independence():
    """A frame's result equals the single-frame call on that frame."""
    W, H, C, U, cams = cs.CASES[0]
    g, feat, dv, du, want = _seeded(0)
    for b in range(3):
        one = dict(g, verts=g["verts"][b:b + 1], w2c=g["w2c"][b:b + 1])
        tx, ty = g["tx"][b:b + 1], g["ty"][b:b + 1]
        out, ndc = _abi_vertices(one["verts"], one["w2c"], tx, ty, feat[b:b + 1])
        assert _bits_equal(out[0], want["vert"]["out"][b]) and _bits_equal(ndc[0], want["vert"]["ndc"][b])
        assert _bits_equal(_abi_uv(one, tx, ty, feat[b:b + 1], g["face_visible"][b:b + 1])[0], want["uv"]["out"][b])
        got = _abi_uv_bwd(one, tx, ty, du[b:b + 1], W, H, g["face_visible"][b:b + 1])
        _assert_backward(got, {k: v[b:b + 1] for k, v in want["uv_bwd"].items()}, f"uv frame {b}")
        got = _abi_vertices_bwd(one["verts"], one["w2c"], tx, ty, dv[b:b + 1], W, H)
        _assert_backward(got, {k: v[b:b + 1] for k, v in want["vert_bwd"].items()}, f"vertices frame {b}")


def test_repeatable_and_workspace_reuse():
    """Forward calls are bit-equal.  The backward keeps no state in its workspace: a call on a workspace
    that another call (other sizes) used and that was then overwritten stays within the bound, and equals
    the first call bit for bit wherever at most two taps meet (a + b has one order)."""
    W, H, C, U, cams = cs.CASES[1]
    g, feat, dv, du, want = _seeded(1)
    a = (g["verts"], g["w2c"], g["tx"], g["ty"])
    o1, n1 = _abi_vertices(*a, feat)
    o2, n2 = _abi_vertices(*a, feat, want_ndc=True)
    o3, _ = _abi_vertices(*a, feat, want_ndc=False)
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and np.array_equal(n1.view(np.uint32), n2.view(np.uint32))
    assert np.array_equal(o1.view(np.uint32), o3.view(np.uint32))
    u1, u2 = (_abi_uv(g, g["tx"], g["ty"], feat, g["face_visible"]) for _ in range(2))
    assert np.array_equal(u1.view(np.uint32), u2.view(np.uint32))
    ws = _ws(3, C, W, H)
    first = _abi_uv_bwd(g, g["tx"], g["ty"], du, W, H, g["face_visible"], ws=ws)
    _abi_vertices_bwd(g["verts"][:1], g["w2c"][:1], g["tx"][:1], g["ty"][:1], dv[:1], W, H, ws=ws)
    ws.fill_(POISON_U8)
    again = _abi_uv_bwd(g, g["tx"], g["ty"], du, W, H, g["face_visible"], ws=ws)
    _assert_backward(first, want["uv_bwd"], "first")
    _assert_backward(again, want["uv_bwd"], "after the workspace was overwritten")
    few = np.broadcast_to(want["uv_bwd"]["n"][:, None] <= 2, first.shape)
    assert few.sum() > 1000 and np.array_equal(first[few].view(np.uint32), again[few].view(np.uint32))


def _lifter(g, W, H, U):
    from guava_renderer_amd.feature_lift import FeatureLifter
    focal = 24.0
    return FeatureLifter(g["faces"], np.maximum(g["texel_face"], 0).reshape(U, U), g["texel_bary"].reshape(U, U, 3),
                         g["uvmap_mask"].reshape(U, U), image_size=(H, W), focal_length=focal, device=DEV)


def test_feature_lifter():
    """The Python surface: the reference's shapes and dtypes, the packed visble_faces path against the
    face_visible path, autograd against the ABI backward's reference, and the refusals."""
    from guava_renderer_amd.feature_lift import FeatureLifter
    W, H, C, U, cams = cs.CASES[1]
    g, feat, dv, du, _ = _seeded(1)
    B, V = g["verts"].shape[:2]
    F = g["faces"].shape[0]
    lf = _lifter(g, W, H, U)
    assert lf.tanfovx == pytest.approx((W / H) / 24.0) and lf.tanfovy == pytest.approx(1 / 24.0)
    assert np.array_equal(lf.texel_face.cpu().numpy(), g["texel_face"])
    tx, ty = np.float32(lf.tanfovx), np.float32(lf.tanfovy)
    verts, w2c, vis = _d(g["verts"]), _d(g["w2c"]), _d(g["face_visible"])
    fm = _d(feat).requires_grad_(True)
    out, img = lf.sample_prj_feature(verts, fm, w2c)
    assert out.shape == (B, V, C) and out.dtype == torch.float32 and img.shape == (B, V, 2) and not img.requires_grad
    wv = ref.lift_vertices(g["verts"], g["w2c"], tx, ty, feat)
    assert _bits_equal(out.detach().cpu().numpy(), wv["out"]) and _bits_equal(img.cpu().numpy(), wv["ndc"])
    out.backward(_d(dv))
    _assert_backward(fm.grad.cpu().numpy(), ref.lift_vertices_backward(g["verts"], g["w2c"], tx, ty, dv, C, W, H),
                     "autograd vertices")
    # UV: face_visible, the packed pix_to_face, and neither
    uvargs = (g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], tx, ty)
    fm2 = _d(feat).requires_grad_(True)
    uv = lf.convert_pixel_feature_to_uv(fm2, verts, w2c, face_visible=vis)
    assert uv.shape == (B, C, U, U) and uv.dtype == torch.float32
    assert _bits_equal(uv.detach().cpu().numpy().reshape(B, C, U * U), ref.lift_uv(*uvargs, feat, g["face_visible"])["out"])
    b_idx, f_idx = np.nonzero(g["face_visible"])
    packed = np.full((B, 40, 50, 1), -1, np.int64)  # a stand-in for render_fragments' pix_to_face
    for b in range(B):
        ids = b * F + f_idx[b_idx == b]
        packed[b].reshape(-1)[:ids.size] = ids
    uv_p = lf.convert_pixel_feature_to_uv(_d(feat), verts, w2c, visble_faces=_d(packed))
    assert torch.equal(uv_p, uv.detach())
    uv_n = lf.convert_pixel_feature_to_uv(_d(feat), verts, w2c)
    assert _bits_equal(uv_n.cpu().numpy().reshape(B, C, U * U), ref.lift_uv(*uvargs, feat, None)["out"])
    uv.backward(_d(du).reshape(B, C, U, U))
    _assert_backward(fm2.grad.cpu().numpy(), ref.lift_uv_backward(*uvargs, du, W, H, g["face_visible"]), "autograd uv")
    # refusals
    with pytest.raises(RuntimeError, match="not both"):
        lf.convert_pixel_feature_to_uv(_d(feat), verts, w2c, visble_faces=_d(packed), face_visible=vis)
    with pytest.raises(NotImplementedError, match="no gradient"):
        lf.sample_prj_feature(verts.clone().requires_grad_(True), _d(feat), w2c)
    with pytest.raises(NotImplementedError, match="no gradient"):
        lf.convert_pixel_feature_to_uv(_d(feat), verts, w2c.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="GPU only"):
        lf.sample_prj_feature(torch.from_numpy(np.array(g["verts"])), _d(feat), w2c)
    with pytest.raises(RuntimeError, match="GPU only"):
        lf.convert_pixel_feature_to_uv(torch.from_numpy(feat.copy()), verts, w2c)
    with pytest.raises(RuntimeError, match="only 0 and 1"):
        FeatureLifter(g["faces"], np.zeros((U, U), np.int64), g["texel_bary"].reshape(U, U, 3),
                      2 * g["uvmap_mask"].reshape(U, U), image_size=(H, W), device=DEV)
    with pytest.raises(RuntimeError, match="was built for"):
        lf.sample_prj_feature(verts, _d(feat)[:, :, :, :W - 1], w2c)


def test_argument_errors_leave_the_poison():
    """GSR_ERR_ARG launches nothing: outputs and workspace keep their poison."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    W, H, C, U, cams = cs.CASES[0]
    g, feat, dv, du, _ = _seeded(0)
    B, V = g["verts"].shape[:2]
    F, T = g["faces"].shape[0], U * U
    t = dict(verts=_d(g["verts"]), faces=_d(g["faces"]), tf=_d(g["texel_face"]), tb=_d(g["texel_bary"]), w2c=_d(g["w2c"]),
             tx=_fov(g["tx"], B), ty=_fov(g["ty"], B), feat=_d(feat), dv=_d(dv), du=_d(du))
    p = {k: v.data_ptr() for k, v in t.items()}
    out_v, out_u, dfeat, ws = _poisoned((B, V, C)), _poisoned((B, C, T)), _poisoned((B, C, H, W)), _ws(B, C, W, H)
    o_v, o_u, o_d, o_w = out_v.data_ptr(), out_u.data_ptr(), dfeat.data_ptr(), ws.data_ptr()
    calls = [
        L.gsr_lift_vertices(B, V, C, W, H, None, p["w2c"], p["tx"], p["ty"], p["feat"], o_v, None, None),
        L.gsr_lift_vertices(B, V, C, W, H, p["verts"], p["w2c"], p["tx"], p["ty"], None, o_v, None, None),
        L.gsr_lift_vertices(B, V, 0, W, H, p["verts"], p["w2c"], p["tx"], p["ty"], p["feat"], o_v, None, None),
        L.gsr_lift_vertices(B, V, C, 16385, H, p["verts"], p["w2c"], p["tx"], p["ty"], p["feat"], o_v, None, None),
        L.gsr_lift_vertices(B, V, 1 << 20, W, H, p["verts"], p["w2c"], p["tx"], p["ty"], p["feat"], o_v, None, None),
        L.gsr_lift_uv(B, V, F, T, C, W, H, p["verts"], p["faces"], None, p["tb"], p["w2c"], p["tx"], p["ty"], p["feat"],
                      None, o_u, None),
        L.gsr_lift_uv(B, V, F, -1, C, W, H, p["verts"], p["faces"], p["tf"], p["tb"], p["w2c"], p["tx"], p["ty"], p["feat"],
                      None, o_u, None),
        L.gsr_lift_uv(B, V, F, T, C, W, 0, p["verts"], p["faces"], p["tf"], p["tb"], p["w2c"], p["tx"], p["ty"], p["feat"],
                      None, o_u, None),
        L.gsr_lift_vertices_backward(B, V, C, W, H, p["verts"], p["w2c"], p["tx"], p["ty"], p["dv"], o_d, None, None),
        L.gsr_lift_vertices_backward(B, 0, C, W, H, p["verts"], p["w2c"], p["tx"], p["ty"], p["dv"], o_d, o_w, None),
        L.gsr_lift_uv_backward(B, V, F, T, C, W, H, p["verts"], p["faces"], p["tf"], p["tb"], p["w2c"], p["tx"], p["ty"],
                               None, None, o_d, o_w, None),
        L.gsr_lift_uv_backward(B, V, F, T, C, W, 20000, p["verts"], p["faces"], p["tf"], p["tb"], p["w2c"], p["tx"],
                               p["ty"], None, p["du"], o_d, o_w, None),
    ]
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls)
    assert L.gsr_lift_backward_workspace_bytes(B, C, 0, H) == 0
    for buf in (out_v, out_u, dfeat):
        assert (buf.view(torch.int32) == POISON_F32).all()
    assert (ws == POISON_U8).all()


def test_full_size():
    """512^2, U = 512, C = 35, B = 2 on the UV path, and the vertex path at C = 128: forward bit-equal to
    the restatement, backward within the bound."""
    W = H = U = 512
    cams = ((0.0, 22.0), (0.7, 22.0))
    g = cs.geometry(W, H, U, cams, seed=11)
    B, V = g["verts"].shape[:2]
    uvargs = (g["verts"], g["faces"], g["texel_face"], g["texel_bary"], g["w2c"], g["tx"], g["ty"])
    feat = cs.features(B, 35, H, W, seed=1)
    assert _bits_equal(_abi_uv(g, g["tx"], g["ty"], feat, g["face_visible"]),
                       ref.lift_uv(*uvargs, feat, g["face_visible"])["out"])
    du = cs.gradient((B, 35, U * U), 2)
    _assert_backward(_abi_uv_bwd(g, g["tx"], g["ty"], du, W, H, g["face_visible"]),
                     ref.lift_uv_backward(*uvargs, du, W, H, g["face_visible"]), "full-size uv")
    a = (g["verts"], g["w2c"], g["tx"], g["ty"])
    feat = cs.features(B, 128, H, W, seed=3)
    want = ref.lift_vertices(*a, feat)
    out, ndc = _abi_vertices(*a, feat)
    assert _bits_equal(out, want["out"]) and _bits_equal(ndc, want["ndc"])
    dv = cs.gradient((B, V, 128), 4)
    _assert_backward(_abi_vertices_bwd(*a, dv, W, H), ref.lift_vertices_backward(*a, dv, 128, W, H), "full-size vertices")
