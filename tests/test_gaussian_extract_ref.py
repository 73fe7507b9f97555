"""CPU tests of the UV Gaussian extraction's numpy restatement (tests/gaussian_extract_ref.py), the
reference of every GPU comparison in test_gpu_gaussian_extract.py, against torch in float64.

 (a) ex_exp against float64 exp over the whole finite range and the special values:
     |err| <= 2 * 2^-23 * |y| wherever the exact result is a normal float (measured 0.68 * 2^-23), at most
     one subnormal step below, +inf above the overflow point, 0 below the underflow point, NaN for NaN.
     The sigmoid built from it: |err| <= 3 * 2^-23 * y wherever the exact sigmoid is normal (measured 1.24).
 (b) rotation: |y_k - exact| <= 2 * 2^-24 * |exact| per component.  The plain float32 evaluation
     sqrtf(((x0*x0 + x1*x1) + x2*x2) + x3*x3) takes seven roundings under the root and would leave the
     quotient up to 4 * 2^-24 off (measured 3.05 * 2^-24), so the norm is refined to the correctly rounded
     one from the operations' rounding errors and one Newton step (include/gsr_extract.h): one rounding
     for the norm and one for the divide, each below 2^-24.  Measured 1.96 to 1.99 * 2^-24 over 2 * 10^6
     normal quaternions at scales 0.01, 1 and 300; the norm itself within 2^-24.
 (c) recipe: the reference's literal recipe, written out here from feature_decoder.py:120-135 (sigmoid,
     exp, F.normalize, permute(0,2,3,1).contiguous()), ubody_gaussian.py:150-156 (reshape and boolean
     gather, binding_face / face_bary), :186-187 (RGB sigmoid) and :229-243 (prune), in torch float64:
     placement and every copied channel exactly equal, activated channels within the bars of (a) and (b).
 (d) backward against torch float64 autograd of the recipe, within 1e-5 relative.  Relative to the
     largest term of each element's expression, because a float32 difference of near-equal terms has no
     per-element relative bound (sigmoid's 1 - y at y -> 1, the normalisation's g_k - y_k*s):
       sigmoid   1e-5 * |g| * y          exp  1e-5 * |dx|          copy  exact
       rotation  1e-5 * max_k|g_k| / d   (each of g_k/d and y_k*s/d is at most 2 max|g| / d)
 (e) the tile / slot arithmetic, and that the header's symbols are bound and built.
"""
import os
import re

import numpy as np
import pytest
import torch

import gaussian_extract_cases as cs
import gaussian_extract_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U23, U24 = 2.0 ** -23, 2.0 ** -24
TINY = 2.0 ** -126


# ---- (a) ----

def _all_finite_floats(step):
    """Every step-th float32 bit pattern, both signs, finite."""
    u = np.arange(0, 0x7F800000, step, dtype=np.uint32)
    x = u.view(np.float32)
    return np.concatenate([x, -x])


def test_ex_exp_accuracy_and_specials():
    x = np.concatenate([_all_finite_floats(1021), np.linspace(-104, 89, 2000001).astype(np.float32)])
    y = ref.ex_exp(x).astype(np.float64)
    with np.errstate(over="ignore"):
        e = np.exp(x.astype(np.float64))
    normal = (e >= TINY) & (e <= 3.4028234663852886e38)
    worst = (np.abs(y[normal] - e[normal]) / e[normal]).max() / U23
    print("ex_exp worst relative error where normal:", worst, "* 2^-23")
    assert worst <= 2.0
    sub = e < TINY
    assert (np.abs(y[sub] - e[sub]) <= 2.0 ** -149).all() and (y[sub] < TINY * (1 + 2 * U23)).all()
    assert np.isinf(y[e > 3.4028235677973366e38]).all() and (y[x < -104.0] == 0).all() and (y[x > 88.73] == np.inf).all()
    s = ref.ex_exp(np.array([np.nan, np.inf, -np.inf, 200.0, -200.0, 0.0, -0.0, 1e-45, -1e-45], np.float32))
    assert np.isnan(s[0]) and s[1] == np.inf and s[2] == 0 and s[3] == np.inf and s[4] == 0 and (s[5:] == 1).all()


def test_ex_sigmoid_accuracy_and_specials():
    x = np.concatenate([_all_finite_floats(1021), np.linspace(-90, 90, 2000001).astype(np.float32)])
    y = ref.ex_sigmoid(x).astype(np.float64)
    with np.errstate(over="ignore"):
        e = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    normal = e >= TINY
    worst = (np.abs(y - e)[normal] / e[normal]).max() / U23
    print("ex_sigmoid worst relative error where normal:", worst, "* 2^-23")
    assert worst <= 3.0
    assert (y[~normal] >= 0).all() and (y[~normal] <= TINY).all()  # 0 or a subnormal below
    s = ref.ex_sigmoid(np.array([np.nan, np.inf, -np.inf, 200.0, -200.0, 0.0, -0.0], np.float32))
    assert np.isnan(s[0]) and s[1] == 1 and s[2] == 0 and s[3] == 1 and s[4] == 0 and s[5] == 0.5 and s[6] == 0.5


# ---- (b) ----

def _rotation_error():
    x = np.random.default_rng(0).standard_normal((2000000, 4)).astype(np.float32)
    y = ref.rot_forward(x).astype(np.float64)
    x64 = x.astype(np.float64)
    y64 = x64 / np.sqrt((x64 * x64).sum(1, keepdims=True))
    return (np.abs(y - y64) / np.abs(y64)).max() / U24


def test_rotation_within_two_half_ulps():
    """2 * 2^-24 relative per component (module docstring (b))."""
    worst = _rotation_error()
    print("rotation worst relative error:", worst, "* 2^-24")
    assert worst <= 2.0


def test_rotation_norm_and_special_rows():
    """The refined norm is within 2^-24 of the exact one at three scales; outside the refinement's range
    the plain evaluation holds: zero, subnormal, below the clamp, overflow, NaN."""
    for seed, scale in ((1, 1.0), (2, 0.01), (3, 300.0)):
        x = (np.random.default_rng(seed).standard_normal((200000, 4)) * scale).astype(np.float32)
        n, d = ref.rot_norm(x)
        exact = np.sqrt((x.astype(np.float64) ** 2).sum(1))
        assert np.array_equal(n, d) and (np.abs(n - exact) <= U24 * exact).all()
    q = np.array([[0, 0, 0, 0], [1e-45, 0, 0, 0], [1e19, -1e19, 1e19, 1e19], [3e-13, 0, 0, 0], [0, 2, 0, 0],
                  [1e15, 0, 0, 0], [1e-12, 0, 0, 0]], np.float32)
    y = ref.rot_forward(q)
    assert not y[0].any() and not np.signbit(y[0]).any()
    assert y[1, 0] == np.float32(1e-45) / np.float32(1e-12) and not y[2].any()   # n = inf: x / inf
    assert y[3, 0] == np.float32(3e-13) / np.float32(1e-12) and np.array_equal(y[4], [0, 1, 0, 0])
    assert y[5, 0] == 1 and y[6, 0] == 1
    with np.errstate(all="ignore"):
        bad = ref.rot_forward(np.array([[np.nan, 1, 0, 0]], np.float32))[0]
    assert np.isnan(bad[0]) and bad[1] == np.float32(1) / np.float32(1e-12)       # fmaxf drops the NaN norm


# ---- (c), (d): the reference's recipe in torch float64 ----

def recipe(maps64, mask, raw, rgb_sigmoid, f_idx=None, f_bary=None, threshold=None):
    """maps64: dict of float64 tensors, planar raw heads [B,k,U,U] (raw) or the decoder's [B,U,U,k]."""
    r = dict(maps64)
    if raw:
        r["opacities"] = torch.sigmoid(r["opacities"])                      # feature_decoder.py:123
        r["scales"] = torch.exp(r["scales"])                                # :126
        r["rotations"] = torch.nn.functional.normalize(r["rotations"])      # :129
        for key in r:
            r[key] = r[key].permute(0, 2, 3, 1).contiguous()                # :135
    B, U = r["colors"].shape[0], r["colors"].shape[1]
    uv_mask_flat = torch.from_numpy(np.asarray(mask).reshape(-1) != 0)
    out = {}
    for key in r:                                                           # ubody_gaussian.py:150-152
        out[key] = r[key].reshape(B, U * U, -1)[:, uv_mask_flat, :]
    if f_idx is not None:
        out["binding_face"] = torch.from_numpy(np.array(f_idx)).reshape(1, U * U, -1)[:, uv_mask_flat, :]  # :153-154
        out["face_bary"] = torch.from_numpy(np.array(f_bary)).reshape(1, U * U, -1)[:, uv_mask_flat, :]    # :155-156
    if rgb_sigmoid:                                                         # :186-187 (out of place: autograd)
        out["colors"] = torch.cat([torch.sigmoid(out["colors"][..., :3]), out["colors"][..., 3:]], -1)
    if threshold is not None:                                               # :229-243
        assert out["opacities"].shape[0] == 1
        m = (out["opacities"] > threshold).squeeze(-1)[0].bool()
        for key in ref.KEYS:
            out[key] = out[key][:, m]
        if f_idx is not None:
            out["binding_face"] = out["binding_face"][0].squeeze(-1)[m]
            out["face_bary"] = out["face_bary"][0][m]
    return out


def _t64(maps, grad=False):
    return {k: torch.from_numpy(np.array(v, np.float64)).requires_grad_(grad) for k, v in maps.items()}


def _assert_forward(got, want, raw, rgb, C):
    """got: the restatement's tables (float32), want: the recipe's (float64 tensors)."""
    w = {k: v.detach().numpy() for k, v in want.items()}
    for key in ref.KEYS:
        assert got[key].shape == w[key].shape, key
    copied = [("local_pos", slice(None))] + ([] if raw else [("opacities", slice(None)), ("scales", slice(None)),
                                                             ("rotations", slice(None))])
    copied.append(("colors", slice(3 if rgb else 0, None)))
    for key, sl in copied:
        assert np.array_equal(got[key][..., sl].astype(np.float64), w[key][..., sl]), key
    if rgb:
        e = w["colors"][..., :3]
        assert (np.abs(got["colors"][..., :3] - e) <= 3 * U23 * e).all()
    if raw:
        assert (np.abs(got["opacities"] - w["opacities"]) <= 3 * U23 * w["opacities"]).all()
        assert (np.abs(got["scales"] - w["scales"]) <= 2 * U23 * w["scales"]).all()
        assert (np.abs(got["rotations"] - w["rotations"]) <= 2 * U24 * np.abs(w["rotations"])).all()


@pytest.mark.parametrize("kind", cs.MASKS)
@pytest.mark.parametrize("raw", (True, False), ids=("planar-raw", "rows-activated"))
def test_forward_against_recipe(kind, raw):
    for U, B, C in ((32, 3, 32), (8, 1, 5)):
        c = cs.case(U, B, C, kind)
        maps = c["raw"] if raw else c["rows"]
        for rgb in (True, False):
            got = ref.extract(maps, c["mask"], raw, rgb, texel_face=c["texel_face"], texel_bary=c["texel_bary"])
            want = recipe(_t64(maps), c["mask"], raw, rgb, c["texel_face"], c["texel_bary"].astype(np.float64))
            assert got["count"] == c["N"] and got["colors"].shape == (B, c["N"], C)
            _assert_forward(got, want, raw, rgb, C)
            assert np.array_equal(got["binding_face"], want["binding_face"].numpy().reshape(-1))
            assert np.array_equal(got["face_bary"].astype(np.float64), want["face_bary"].numpy().reshape(-1, 3))


@pytest.mark.parametrize("raw", (True, False), ids=("planar-raw", "rows-activated"))
def test_prune_against_recipe(raw):
    c = cs.case(32, 1, 32, "random")
    maps = c["raw"] if raw else c["rows"]
    opacity = ref.activate(ref.to_rows(maps, raw), raw, True)["opacities"][0, :, 0]
    thresholds = cs.prune_thresholds(opacity, c["mask"])
    assert sorted(k for _, k in thresholds.values()) == [0, 1, c["N"] - c["N"] // 2, c["N"]]
    for name, (thr, kept) in thresholds.items():
        got = ref.extract(maps, c["mask"], raw, True, threshold=thr, texel_face=c["texel_face"], texel_bary=c["texel_bary"])
        want = recipe(_t64(maps), c["mask"], raw, True, c["texel_face"], c["texel_bary"].astype(np.float64),
                      threshold=float(thr))
        assert got["count"] == kept == want["opacities"].shape[1], name
        head = {k: got[k][:, :kept] for k in ref.KEYS}
        _assert_forward(head, want, raw, True, 32)
        assert np.array_equal(got["binding_face"][:kept], want["binding_face"].numpy())
        assert np.array_equal(got["face_bary"][:kept].astype(np.float64), want["face_bary"].numpy())
        for k in ref.KEYS + ("binding_face", "face_bary"):
            tail = got[k][kept:] if k in ("binding_face", "face_bary") else got[k][:, kept:]
            assert not tail.any(), (name, k)
        # the kept rows are the unpruned rows selected in order
        full = ref.extract(maps, c["mask"], raw, True)
        sel = np.nonzero(full["opacities"][0, :, 0] > thr)[0]
        assert all(np.array_equal(head[k], full[k][:, sel]) for k in ref.KEYS)


@pytest.mark.parametrize("raw", (True, False), ids=("planar-raw", "rows-activated"))
@pytest.mark.parametrize("rgb", (True, False), ids=("rgb", "no-rgb"))
def test_backward_against_autograd(raw, rgb):
    for U, B, C, kind in ((32, 3, 32, "random"), (8, 1, 5, "stripes"), (8, 1, 5, "empty")):
        c = cs.case(U, B, C, kind)
        maps = c["raw"] if raw else c["rows"]
        grads = cs.gradients(B, c["N"], C, seed=3)
        t = _t64(maps, grad=True)
        out = recipe(t, c["mask"], raw, rgb)
        sum((out[k] * torch.from_numpy(grads[k].astype(np.float64))).sum() for k in ref.KEYS).backward()
        got = ref.extract_backward(maps, c["mask"], grads, raw, rgb)
        sel = np.nonzero(c["mask"])[0]
        rows_in = ref.to_rows(maps, raw)
        for key in ref.KEYS:
            want = t[key].grad.numpy()
            assert got[key].shape == want.shape and got[key].dtype == np.float32
            g_rows = ref.to_rows({k: got[k] for k in ref.KEYS}, raw)[key].astype(np.float64)
            w_rows = ref.to_rows({k: (t[k].grad.numpy()) for k in ref.KEYS}, raw)[key].astype(np.float64)
            outside = np.ones(U * U, bool)
            outside[sel] = False
            z = g_rows[:, outside]
            assert not z.any() and not np.signbit(z).any() and not w_rows[:, outside].any()
            err = np.abs(g_rows[:, sel] - w_rows[:, sel])
            g = np.abs(grads[key].astype(np.float64))
            x = rows_in[key][:, sel].astype(np.float64)
            if key == "local_pos" or (not raw and key != "colors"):
                bound = np.zeros_like(err)
            elif key == "colors":
                bound = np.zeros_like(err)
                if rgb:
                    bound[..., :3] = 1e-5 * g[..., :3] / (1.0 + np.exp(-x[..., :3]))
            elif key == "opacities":
                bound = 1e-5 * g / (1.0 + np.exp(-x))
            elif key == "scales":
                bound = 1e-5 * np.abs(w_rows[:, sel])
            else:
                d = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
                bound = np.broadcast_to(1e-5 * g.max(-1, keepdims=True) / d, err.shape)
            assert (err <= bound).all(), (key, float((err - bound).max()))


def test_rotation_backward_clamp_branch():
    """F.normalize's autograd at n = 0, n = 3e-13 (the clamp branch) and a generic row."""
    q = np.array([[0, 0, 0, 0], [3e-13, 0, 0, 0], [0.3, -1.2, 0.5, 2.0]], np.float32)
    g = np.array([[1, 2, 3, 4], [1, -2, 0.5, 4], [0.7, 0.1, -2, 1]], np.float32)
    t = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)
    (torch.nn.functional.normalize(t, dim=-1) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    got = ref.rot_backward(q, g).astype(np.float64)
    want = t.grad.numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max() and (np.abs(got[:2] - want[:2]) <= 1e-6 * np.abs(want[:2])).all()


# ---- (e) ----

def test_tile_and_slot_arithmetic():
    for T in (1, 63, 64, 65, 1000, 2304):
        for kind in ("full", "empty", "first", "last", "random", "stripes"):
            m = cs.mask(kind, T, seed=T)
            base, s = ref.tile_bases(m != 0), ref.slots(m != 0)
            assert base.shape == ((T + 63) // 64 + 1,) and base[0] == 0 and base[-1] == m.sum()
            assert np.array_equal(s[m != 0], np.arange(int(m.sum()))) and (s[m == 0] == -1).all()


def test_extract_symbols_are_bound_and_built():
    """Every symbol include/gsr_extract.h declares is in _lib.EXPORTS with argtypes, extract.hip is
    built, and bad arguments are refused without a device."""
    from guava_renderer_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gsr_extract.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\*?\s+\**(gsr_[a-z_0-9]+)\s*\(", hdr, re.M))
    assert declared == {"gsr_extract_tiles", "gsr_extract_prepare", "gsr_extract_prepare_pruned", "gsr_extract_forward",
                        "gsr_extract_forward_pruned", "gsr_extract_backward"}
    assert declared <= set(_lib.EXPORTS)
    assert "extract.hip" in build.SOURCES
    L = _lib.load()
    for sym in declared:
        assert getattr(L, sym).argtypes is not None, sym
    assert L.gsr_extract_tiles(1000) == 16 and L.gsr_extract_tiles(2304) == 36 and L.gsr_extract_tiles(0) == 0
    assert L.gsr_extract_prepare(64, None, None, None) == -1 and b"null" in L.gsr_last_error()
    assert L.gsr_extract_prepare(0, None, None, None) == -1 and b"bad sizes" in L.gsr_last_error()
    assert L.gsr_extract_forward(1, 64, 8, 2, 0, 0, *([None] * 9)) == -1 and b"bad sizes" in L.gsr_last_error()
    assert L.gsr_extract_forward(1, 64, 8, 65, 0, 0, *([None] * 9)) == -1
    assert L.gsr_extract_forward(1, 64, 65, 32, 0, 0, *([None] * 9)) == -1        # N > T
    assert L.gsr_extract_forward(1, 64, 8, 32, 2, 0, *([None] * 9)) == -1         # layout
    assert L.gsr_extract_forward(64, 1 << 20, 8, 32, 0, 0, *([None] * 9)) == -1   # B*T*(C+11) >= 2^31
    assert L.gsr_extract_forward(1, 64, 8, 32, 0, 0, *([None] * 9)) == -1 and b"null" in L.gsr_last_error()
    assert L.gsr_extract_backward(1, 64, 8, 32, 0, 0, *([None] * 6)) == -1 and b"null" in L.gsr_last_error()
    assert L.gsr_extract_forward_pruned(64, 8, 32, 0, 0, 0.5, *([None] * 10)) == -1


def test_no_cpu_path_and_export():
    import guava_renderer_amd
    from guava_renderer_amd.gaussian_extract import UVGaussianExtractor
    assert guava_renderer_amd.UVGaussianExtractor is UVGaussianExtractor
    with pytest.raises(RuntimeError, match="GPU only"):
        UVGaussianExtractor(np.ones((2, 2), np.float32), np.zeros((2, 2), np.int64), np.zeros((2, 2, 3), np.float32),
                            device="cpu")
