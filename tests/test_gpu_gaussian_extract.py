"""GPU tests of the UV Gaussian extraction (include/gsr_extract.h, csrc/extract.hip,
guava_renderer_amd/gaussian_extract.py).

Reference of every comparison: the float32 evaluation of tests/gaussian_extract_ref.py, which states
the kernels' arithmetic op for op (test_gaussian_extract_ref.py judges it against torch in float64).
Forward and backward are compared on the bits (np.array_equal on the uint32 views; where the inputs
hold NaN, NaN against NaN and the bits elsewhere).  Calls through the C ABI (_abi_*) poison every
output (a NaN with its own payload) first and check afterwards that no element kept the poison's bits.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gaussian_extract_cases as cs
import gaussian_extract_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON_F32 = 0x7FC5A5A5  # a quiet NaN no computation produces
POISON_I32 = 0x5A5A5A5A
KEYS = ref.KEYS


def _d(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _poisoned(shape):
    return torch.full(shape, POISON_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def _clean(t):
    a = t.cpu().numpy()
    assert not (a.view(np.uint32) == (POISON_F32 if a.dtype == np.float32 else POISON_I32)).any(), "poison kept"
    return a


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _set(tensors):
    from guava_renderer_amd import _lib
    return _lib.ExtractSet(*[_ptr(t) for t in tensors])


def _bits_equal(got, want, nan_ok=False):
    want = np.ascontiguousarray(want, got.dtype)
    if got.shape != want.shape:
        return False
    if got.dtype != np.float32:
        return np.array_equal(got, want)
    if nan_ok:
        n = np.isnan(want)
        return np.array_equal(np.isnan(got), n) and np.array_equal(got[~n].view(np.uint32), want[~n].view(np.uint32))
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _widths(C):
    return (C, 1, 3, 4, 3)


def _abi_prepare(mask, opacities=None, layout=0, threshold=0.0):
    from guava_renderer_amd import _lib
    L = _lib.load()
    T = mask.shape[0]
    nt = L.gsr_extract_tiles(T)
    assert nt == (T + 63) // 64
    base = torch.full((nt + 1,), POISON_I32, dtype=torch.int32, device=DEV)
    m = _d(mask)
    if opacities is None:
        _lib.check(L.gsr_extract_prepare(T, _ptr(m), _ptr(base), _stream()), "gsr_extract_prepare")
    else:
        _lib.check(L.gsr_extract_prepare_pruned(T, layout, _ptr(m), _ptr(opacities), float(threshold), _ptr(base),
                                                _stream()), "gsr_extract_prepare_pruned")
    torch.cuda.synchronize()
    return m, base


def _abi_forward(maps, mask, C, raw, rgb, binding=None, threshold=None):
    """-> (dict of tables, binding_face, face_bary as numpy, tile_base as numpy)."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    T, N = mask.shape[0], int(mask.sum())
    B = maps["colors"].shape[0]
    layout = 0 if raw else 1
    dm = [_d(maps[k]) for k in KEYS]
    m, base = _abi_prepare(mask)
    want_base = ref.tile_bases(mask != 0)
    assert np.array_equal(_clean(base), want_base)
    tables = [_poisoned((B, N, k)) for k in _widths(C)]
    tf = tb = bf = fb = None
    if binding is not None:
        tf, tb = _d(binding[0]), _d(binding[1])
        bf = torch.full((N,), POISON_I32, dtype=torch.int32, device=DEV)
        fb = _poisoned((N, 3))
    if threshold is None:
        rc = L.gsr_extract_forward(B, T, N, C, layout, int(rgb), _ptr(m), _ptr(base), ctypes.byref(_set(dm)),
                                   ctypes.byref(_set(tables)), _ptr(tf), _ptr(tb), _ptr(bf), _ptr(fb), _stream())
        pbase = base
    else:
        _, pbase = _abi_prepare(mask, dm[1], layout, threshold)
        rc = L.gsr_extract_forward_pruned(T, N, C, layout, int(rgb), float(threshold), _ptr(m), _ptr(base), _ptr(pbase),
                                          ctypes.byref(_set(dm)), ctypes.byref(_set(tables)), _ptr(tf), _ptr(tb),
                                          _ptr(bf), _ptr(fb), _stream())
    _lib.check(rc, "gsr_extract_forward")
    torch.cuda.synchronize()
    out = {k: _clean(t) for k, t in zip(KEYS, tables)}
    return out, (None if bf is None else _clean(bf)), (None if fb is None else _clean(fb)), _clean(pbase)


def _abi_backward(maps, mask, grads, C, raw, rgb, wanted=KEYS):
    from guava_renderer_amd import _lib
    L = _lib.load()
    T, N = mask.shape[0], int(mask.sum())
    B = maps["colors"].shape[0]
    dm = [_d(maps[k]) for k in KEYS]
    dg = [_d(grads[k]) for k in KEYS]
    m, base = _abi_prepare(mask)
    outs = [_poisoned(tuple(maps[k].shape)) if k in wanted else None for k in KEYS]
    _lib.check(L.gsr_extract_backward(B, T, N, C, 0 if raw else 1, int(rgb), _ptr(m), _ptr(base), ctypes.byref(_set(dm)),
                                      ctypes.byref(_set(dg)), ctypes.byref(_set(outs)), _stream()), "gsr_extract_backward")
    torch.cuda.synchronize()
    return {k: _clean(o) for k, o in zip(KEYS, outs) if o is not None}


CASES = ([(32, 3, 32, k) for k in cs.MASKS] + [(32, 1, 5, "random")] + [(8, 1, 5, k) for k in cs.MASKS] +
         [(8, 3, 32, "last"), (48, 3, 5, "full"), (48, 1, 32, "stripes"), (48, 3, 32, "random"), (48, 1, 5, "last")])


@functools.lru_cache(maxsize=None)
def _want(U, B, C, kind, raw, rgb):
    """The restatement's forward and backward of one case, made once and left unchanged."""
    c = cs.case(U, B, C, kind)
    maps = c["raw"] if raw else c["rows"]
    grads = cs.gradients(B, c["N"], C, seed=11)
    fwd = ref.extract(maps, c["mask"], raw, rgb, texel_face=c["texel_face"], texel_bary=c["texel_bary"])
    bwd = ref.extract_backward(maps, c["mask"], grads, raw, rgb)
    for a in list(grads.values()) + [v for v in fwd.values() if isinstance(v, np.ndarray)] + list(bwd.values()):
        a.setflags(write=False)
    return c, maps, grads, fwd, bwd


@pytest.mark.parametrize("raw", (True, False), ids=("planar-raw", "rows-activated"))
@pytest.mark.parametrize("U,B,C,kind", CASES, ids=[f"U{u}-B{b}-C{c}-{k}" for u, b, c, k in CASES])
def test_seeded_case(U, B, C, kind, raw):
    for rgb in (True, False):
        c, maps, grads, fwd, bwd = _want(U, B, C, kind, raw, rgb)
        N, T = c["N"], U * U
        assert {"empty": N == 0, "full": N == T, "last": N == 1}.get(kind, 0 < N < T)
        assert kind != "random" or U != 32 or N == 769
        got, bf, fb, _ = _abi_forward(maps, c["mask"], C, raw, rgb, binding=(c["texel_face"], c["texel_bary"]))
        for k in KEYS:
            assert _bits_equal(got[k], fwd[k]), k
        assert _bits_equal(bf, fwd["binding_face"]) and _bits_equal(fb, fwd["face_bary"])
        again, _, _, _ = _abi_forward(maps, c["mask"], C, raw, rgb)
        assert all(_bits_equal(again[k], got[k]) for k in KEYS)
        if not raw and not rgb:  # torch's own gather on the device
            sel = _d(c["mask"] != 0)
            for k in KEYS:
                w = _d(maps[k]).reshape(B, T, -1)[:, sel]
                assert _bits_equal(got[k], w.cpu().numpy()), k
        back = _abi_backward(maps, c["mask"], grads, C, raw, rgb)
        outside = np.broadcast_to((c["mask"] == 0).reshape(U, U), (B, U, U))
        for k in KEYS:
            assert _bits_equal(back[k], bwd[k]), k
            z = back[k][outside] if not raw else np.moveaxis(back[k], 1, -1)[outside]
            assert not z.view(np.uint32).any(), k  # the bit pattern of +0
        back2 = _abi_backward(maps, c["mask"], grads, C, raw, rgb)
        assert all(_bits_equal(back2[k], back[k]) for k in KEYS)
        # only some gradients wanted: the others are not written, the wanted ones unchanged
        some = _abi_backward(maps, c["mask"], grads, C, raw, rgb, wanted=("scales", "colors"))
        assert set(some) == {"scales", "colors"} and all(_bits_equal(some[k], back[k]) for k in some)


@pytest.mark.parametrize("raw", (True, False), ids=("planar-raw", "rows-activated"))
def test_abi_texel_count_that_is_no_square_or_tile_multiple(raw):
    """T = 1000: the last tile holds 40 texels."""
    T, B, C = 1000, 3, 5
    rng = np.random.default_rng(4)
    raw_maps = {k: rng.standard_normal((B, w, T)).astype(np.float32) for k, w in zip(KEYS, _widths(C))}
    maps = raw_maps if raw else {k: np.ascontiguousarray(v)
                                 for k, v in ref.activate(ref.to_rows(raw_maps, True), True, False).items()}
    for kind in ("stripes", "last", "full"):
        mask = cs.mask(kind, T)
        N = int(mask.sum())
        grads = cs.gradients(B, N, C, seed=2)
        tf, tb = cs.binding(T, 9)
        fwd = ref.extract(maps, mask, raw, True, texel_face=tf, texel_bary=tb)
        got, bf, fb, _ = _abi_forward(maps, mask, C, raw, True, binding=(tf, tb))
        assert all(_bits_equal(got[k], fwd[k]) for k in KEYS)
        assert _bits_equal(bf, fwd["binding_face"]) and _bits_equal(fb, fwd["face_bary"])
        bwd = ref.extract_backward(maps, mask, grads, raw, True)
        back = _abi_backward(maps, mask, grads, C, raw, True)
        assert all(_bits_equal(back[k], bwd[k]) for k in KEYS)


def test_special_values():
    """NaN / inf / +-200 / +-0 / subnormal logits and zero, subnormal, huge, NaN and inf quaternions:
    the call succeeds and the values are the restatement's."""
    U, C = 8, 5
    maps = cs.special_maps(U, C)
    mask = cs.mask("full", U * U)
    fwd = ref.extract(maps, mask, True, True)
    assert np.isnan(fwd["opacities"]).any() and np.isinf(fwd["scales"]).any() and not fwd["rotations"][0, 0].any()
    got, _, _, _ = _abi_forward(maps, mask, C, True, True)
    for k in KEYS:
        assert _bits_equal(got[k], fwd[k], nan_ok=True), k
    grads = cs.gradients(1, U * U, C, seed=6)
    with np.errstate(all="ignore"):
        bwd = ref.extract_backward(maps, mask, grads, True, True)
    back = _abi_backward(maps, mask, grads, C, True, True)
    for k in KEYS:
        assert _bits_equal(back[k], bwd[k], nan_ok=True), k
    # copied channels keep every bit, the special ones included
    assert np.array_equal(got["colors"][0, :, 3].view(np.uint32), maps["colors"][0, 3].reshape(-1).view(np.uint32))


@pytest.mark.parametrize("raw", (True, False), ids=("planar-raw", "rows-activated"))
def test_pruning(raw):
    U, C = 32, 32
    c = cs.case(U, 1, C, "random")
    maps = c["raw"] if raw else c["rows"]
    N = c["N"]
    opacity = ref.activate(ref.to_rows(maps, raw), raw, True)["opacities"][0, :, 0]
    thresholds = cs.prune_thresholds(opacity, c["mask"])
    full = ref.extract(maps, c["mask"], raw, True, texel_face=c["texel_face"], texel_bary=c["texel_bary"])
    for name, (thr, kept) in thresholds.items():
        want = ref.extract(maps, c["mask"], raw, True, threshold=thr, texel_face=c["texel_face"], texel_bary=c["texel_bary"])
        assert want["count"] == kept
        got, bf, fb, pbase = _abi_forward(maps, c["mask"], C, raw, True, binding=(c["texel_face"], c["texel_bary"]),
                                          threshold=thr)
        assert int(pbase[-1]) == kept, name  # the count word
        sel = np.nonzero(full["opacities"][0, :, 0] > thr)[0]
        assert sel.size == kept
        for k in KEYS:
            assert _bits_equal(got[k], want[k]), (name, k)
            assert _bits_equal(got[k][:, :kept], full[k][:, sel]) and not got[k][:, kept:].view(np.uint32).any(), (name, k)
        assert _bits_equal(bf, want["binding_face"]) and _bits_equal(fb, want["face_bary"])
        assert np.array_equal(bf[:kept], full["binding_face"][sel]) and not bf[kept:].any()
        assert not fb[kept:].view(np.uint32).any()


def _extractor(c, C):
    from guava_renderer_amd.gaussian_extract import UVGaussianExtractor
    U = c["U"]
    return UVGaussianExtractor(c["mask"].reshape(U, U).astype(np.float32), c["texel_face"].reshape(U, U).astype(np.int64),
                               c["texel_bary"].reshape(U, U, 3), color_dim=C, device=DEV)


def test_extractor_surface():
    """The Python surface: the reference's dict, both layouts, pruning, and the refusals."""
    import guava_renderer_amd
    from guava_renderer_amd.gaussian_extract import UVGaussianExtractor
    assert guava_renderer_amd.UVGaussianExtractor is UVGaussianExtractor
    U, B, C = 32, 3, 32
    c, maps, grads, fwd, bwd = _want(U, B, C, "random", True, True)
    ex = _extractor(c, C)
    N = c["N"]
    assert ex.N == N and np.array_equal(ex.tile_base.cpu().numpy(), ref.tile_bases(c["mask"] != 0))
    d = ex.extract(*[_d(maps[k]) for k in KEYS])
    assert set(d) == set(KEYS) | {"binding_face", "face_bary"}
    assert d["binding_face"].shape == (1, N, 1) and d["binding_face"].dtype == torch.int64
    assert d["face_bary"].shape == (1, N, 3) and d["colors"].shape == (B, N, C) and d["opacities"].shape == (B, N, 1)
    for k in KEYS:
        assert _bits_equal(d[k].cpu().numpy(), fwd[k]), k
    assert np.array_equal(d["binding_face"].cpu().numpy().reshape(-1), fwd["binding_face"])
    assert _bits_equal(d["face_bary"].cpu().numpy()[0], fwd["face_bary"])
    # rows layout, flag off: the reference's own dict
    rows = cs.case(U, B, C, "random")["rows"]
    d2 = ex.extract(*[_d(rows[k]) for k in KEYS], raw=False, rgb_sigmoid=False)
    w2 = ref.extract(rows, c["mask"], False, False)
    assert all(_bits_equal(d2[k].cpu().numpy(), w2[k]) for k in KEYS)
    # pruning at B = 1
    c1 = cs.case(U, 1, C, "random")
    op = ref.activate(ref.to_rows(c1["raw"], True), True, True)["opacities"][0, :, 0]
    thr, kept = cs.prune_thresholds(op, c1["mask"])["half"]
    ex1 = _extractor(c1, C)
    with torch.no_grad():
        p = ex1.extract_pruned(*[_d(c1["raw"][k]) for k in KEYS], opacity_threshold=float(thr))
    w = ref.extract(c1["raw"], c1["mask"], True, True, threshold=thr, texel_face=c1["texel_face"],
                    texel_bary=c1["texel_bary"])
    assert p["colors"].shape == (1, kept, C) and p["binding_face"].shape == (1, kept, 1)
    assert all(_bits_equal(p[k].cpu().numpy(), w[k][:, :kept]) for k in KEYS)
    assert np.array_equal(p["binding_face"].cpu().numpy().reshape(-1), w["binding_face"][:kept])
    assert _bits_equal(p["face_bary"].cpu().numpy()[0], w["face_bary"][:kept])
    # an empty mask: empty tables, zero gradients
    e = cs.case(8, 1, 5, "empty")
    exe = _extractor(e, 5)
    leaves = [_d(e["raw"][k]).requires_grad_(True) for k in KEYS]
    de = exe.extract(*leaves)
    assert exe.N == 0 and de["colors"].shape == (1, 0, 5) and de["binding_face"].shape == (1, 0, 1)
    sum(de[k].sum() for k in KEYS).backward()
    assert all(l.grad.shape == l.shape and not l.grad.cpu().numpy().view(np.uint32).any() for l in leaves)
    # refusals
    good = [_d(maps[k]) for k in KEYS]
    with pytest.raises(RuntimeError, match="GPU only"):
        ex.extract(torch.from_numpy(np.array(maps["colors"])), *good[1:])
    with pytest.raises(RuntimeError, match=r"scales must have dimensions \(B, 3, 32, 32\)"):
        ex.extract(good[0], good[1], good[2][:, :2], good[3], good[4])
    with pytest.raises(RuntimeError, match=r"colors must have dimensions \(B, 32, 32, 32\)"):
        ex.extract(good[0][:, :5], *good[1:], raw=False)
    with pytest.raises(RuntimeError, match="with B = 3"):
        ex.extract(good[0], good[1][:1], *good[2:])
    with pytest.raises(RuntimeError, match="B = 1"):
        ex.extract_pruned(*good)
    with pytest.raises(RuntimeError, match="no gradient"):
        ex1.extract_pruned(*[_d(c1["raw"][k]).requires_grad_(k == "scales") for k in KEYS])
    with pytest.raises(RuntimeError, match="only 0 and 1"):
        UVGaussianExtractor(2 * c["mask"].reshape(U, U).astype(np.float32), c["texel_face"].reshape(U, U),
                            c["texel_bary"].reshape(U, U, 3), device=DEV)
    with pytest.raises(RuntimeError, match=r"\[3, 64\]"):
        UVGaussianExtractor(c["mask"].reshape(U, U), c["texel_face"].reshape(U, U), c["texel_bary"].reshape(U, U, 3),
                            color_dim=65, device=DEV)


def test_autograd_through_deform_gaussians():
    """extract -> deform_gaussians -> a random linear loss on the template's topology at U = 32: the map
    gradients are gsr_deform_gaussians_backward's table gradients pushed through the restatement's
    backward, bit for bit; a map that does not require grad gets None."""
    from guava_renderer_amd import _lib, deform
    import mesh_raster_cases as mc
    U, B, C = 32, 2, 32
    c = cs.case(U, B, C, "random")
    N = c["N"]
    verts_np, _ = mc.posed_batch(((0.0, 22.0), (0.7, 22.0)), seed=1)
    _, faces_np = mc.template()
    V, F = verts_np.shape[1], faces_np.shape[0]
    assert int(c["texel_face"].max()) < F
    rng = np.random.default_rng(8)
    Tm = np.broadcast_to(np.eye(4, dtype=np.float32), (B, V, 4, 4)).copy()
    Tm[..., :3, :3] += rng.normal(scale=0.1, size=(B, V, 3, 3)).astype(np.float32)
    vr = rng.standard_normal((V, 4)).astype(np.float32)
    vs = rng.uniform(0.005, 0.03, (V, 3)).astype(np.float32)
    P = V + N
    g_xyz, g_rot, g_scl = (rng.standard_normal((B, P, k)).astype(np.float32) for k in (3, 4, 3))
    g_col, g_op = rng.standard_normal((B, N, C)).astype(np.float32), rng.standard_normal((B, N, 1)).astype(np.float32)
    verts, T, faces = _d(verts_np), _d(Tm), _d(np.array(faces_np, np.int32))
    ex = _extractor(c, C)
    leaves = {k: _d(c["raw"][k]).requires_grad_(k != "colors") for k in KEYS}
    d = ex.extract(*[leaves[k] for k in KEYS])
    xyz, rot, scl = deform.deform_gaussians(verts, T, faces, d["binding_face"], d["face_bary"], _d(vr), _d(vs),
                                            d["local_pos"], d["rotations"], d["scales"])
    loss = ((xyz * _d(g_xyz)).sum() + (rot * _d(g_rot)).sum() + (scl * _d(g_scl)).sum() +
            (d["colors"] * _d(g_col)).sum() + (d["opacities"] * _d(g_op)).sum())
    loss.backward()
    torch.cuda.synchronize()
    assert leaves["colors"].grad is None
    # the table gradients, straight from the deform's backward entry
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    bind = d["binding_face"].reshape(-1).to(torch.int32).contiguous()
    bary = d["face_bary"].reshape(-1, 3).contiguous()
    attrs = [_d(vr), _d(vs), d["local_pos"].detach(), d["rotations"].detach(), d["scales"].detach()]
    di, keep = deform.deform_inputs(B, verts, T, faces, bind, bary, attrs, bad)
    outs = [None, None] + [torch.zeros((B, N, k), dtype=torch.float32, device=DEV) for k in (3, 4, 3)]
    dgr = _lib.DeformGrads(*[None if o is None else o.data_ptr() for o in outs])
    ups = [_d(g_xyz), _d(g_rot), _d(g_scl)]
    _lib.check(_lib.load().gsr_deform_gaussians_backward(B, ctypes.byref(di), ups[0].data_ptr(), ups[1].data_ptr(),
                                                         ups[2].data_ptr(), ctypes.byref(dgr), _stream()),
               "gsr_deform_gaussians_backward")
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    tg = dict(colors=g_col, opacities=g_op, local_pos=outs[2].cpu().numpy(), rotations=outs[3].cpu().numpy(),
              scales=outs[4].cpu().numpy())
    assert all(np.abs(tg[k]).max() > 0 for k in KEYS)
    want = ref.extract_backward(c["raw"], c["mask"], tg, True, True)
    for k in KEYS:
        if k != "colors":
            assert _bits_equal(leaves[k].grad.cpu().numpy(), want[k]), k


def test_argument_errors_leave_the_poison():
    """GSR_ERR_ARG launches nothing: the outputs keep their poison."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    U, B, C = 8, 1, 5
    c = cs.case(U, B, C, "stripes")
    T, N = U * U, c["N"]
    dm = [_d(c["raw"][k]) for k in KEYS]
    m, base = _abi_prepare(c["mask"])
    tables = [_poisoned((B, N, k)) for k in _widths(C)]
    dmaps = [_poisoned(tuple(c["raw"][k].shape)) for k in KEYS]
    pb = torch.full_like(base, POISON_I32)
    S, St, Sd = _set(dm), _set(tables), _set(dmaps)
    none5 = _lib.ExtractSet(None, None, None, None, None)
    half = _lib.ExtractSet(tables[0].data_ptr(), None, None, None, None)
    r = ctypes.byref
    n4 = (None, None, None, None)
    calls = [
        L.gsr_extract_forward(B, T, N, C, 0, 1, None, _ptr(base), r(S), r(St), *n4, None),
        L.gsr_extract_forward(B, T, N, C, 0, 1, _ptr(m), None, r(S), r(St), *n4, None),
        L.gsr_extract_forward(B, T, N, C, 0, 1, _ptr(m), _ptr(base), r(S), r(half), *n4, None),
        L.gsr_extract_forward(B, T, N, C, 0, 1, _ptr(m), _ptr(base), r(none5), r(St), *n4, None),
        L.gsr_extract_forward(B, T, N, C, 0, 1, _ptr(m), _ptr(base), r(S), None, *n4, None),
        L.gsr_extract_forward(B, T, N, 2, 0, 1, _ptr(m), _ptr(base), r(S), r(St), *n4, None),
        L.gsr_extract_forward(B, T, N, 65, 0, 1, _ptr(m), _ptr(base), r(S), r(St), *n4, None),
        L.gsr_extract_forward(0, T, N, C, 0, 1, _ptr(m), _ptr(base), r(S), r(St), *n4, None),
        L.gsr_extract_forward(B, T, T + 1, C, 0, 1, _ptr(m), _ptr(base), r(S), r(St), *n4, None),
        L.gsr_extract_forward(B, T, N, C, 7, 1, _ptr(m), _ptr(base), r(S), r(St), *n4, None),
        L.gsr_extract_forward(1 << 16, 1 << 14, N, C, 0, 1, _ptr(m), _ptr(base), r(S), r(St), *n4, None),
        L.gsr_extract_forward(B, T, N, C, 0, 1, _ptr(m), _ptr(base), r(S), r(St), _ptr(m), None, None, None, None),
        L.gsr_extract_forward_pruned(T, N, C, 0, 1, 0.5, _ptr(m), _ptr(base), None, r(S), r(St), *n4, None),
        L.gsr_extract_backward(B, T, N, C, 0, 1, _ptr(m), _ptr(base), r(none5), r(St), r(Sd), None),
        L.gsr_extract_backward(B, T, N, C, 0, 1, _ptr(m), _ptr(base), r(S), r(St), None, None),
        L.gsr_extract_backward(B, -1, N, C, 0, 1, _ptr(m), _ptr(base), r(S), r(St), r(Sd), None),
        L.gsr_extract_prepare(T, _ptr(m), None, None),
        L.gsr_extract_prepare(-5, _ptr(m), _ptr(pb), None),
        L.gsr_extract_prepare_pruned(T, 3, _ptr(m), _ptr(dm[1]), 0.5, _ptr(pb), None),
        L.gsr_extract_prepare_pruned(T, 0, _ptr(m), None, 0.5, _ptr(pb), None),
    ]
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls)
    for buf in tables + dmaps:
        assert (buf.view(torch.int32) == POISON_F32).all()
    assert (pb == POISON_I32).all()
    # N = 0 in the data sense launches nothing and succeeds
    assert L.gsr_extract_forward(B, T, 0, C, 0, 1, _ptr(m), _ptr(base), r(none5), r(none5), *n4, None) == 0
    torch.cuda.synchronize()
    assert all((buf.view(torch.int32) == POISON_F32).all() for buf in tables)
