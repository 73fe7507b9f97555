"""A numpy restatement of the refiner decoder's four backward passes (include/gsr_refiner.h, second half;
guava_renderer_amd/csrc/refiner_dev.h and refiner_bwd.hip).

Where the header states an order -- the elementwise outputs, up2T, the sums over o and over b -- the
restatement is float32 as written and the GPU must agree bit for bit.  Where it states a tree only (the
sums over the pixels of a plane) the restatement forms the same float32 terms and adds them in float64,
and returns the sum of their magnitudes for the header's bound (D + k) * 2^-24 * sum|term|.

Every function takes dtype=np.float32 (the kernels' arithmetic) or np.float64 (the same expressions in
double, with the exact sqrt(2): what tests/test_refiner_bwd_ref.py holds against float64 autograd).
"""
import functools
import os

import numpy as np

import refiner_cases as rc

F32 = np.float32
U = 2.0 ** -24
CHUNK_QUADS = 256  # kRfChunkQuads
GRAD_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refiner_decoder_grad.npz")


@functools.lru_cache(maxsize=None)
def load_grad_golden(v):
    """tests/golden/refiner_decoder_grad.npz, variant "full" or "small" -> (G, {parameter name: gradient},
    the style code's gradient, [the condition maps' gradients]), float64."""
    z = np.load(GRAD_GOLDEN)
    sd = {k[len(v) + 9:]: z[k] for k in z.files if k.startswith(f"{v}/grad/sd/")}
    cond = [z[f"{v}/grad/cond/{i}"] for i in range(len([k for k in z.files if k.startswith(f"{v}/grad/cond/")]))]
    return z[f"{v}/G"], sd, z[f"{v}/grad/style"], cond


def scale_err(a, ref):
    """max|a - ref| over the tensor, relative to max|ref|."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64).reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _c(dtype, v):
    return dtype(v)


def sqrt2(dtype):
    return rc.SQRT2 if dtype is F32 else np.float64(2 ** 0.5)


def chunks(H, W):
    """gsr_style_backward_chunks."""
    return -(-(H * (W // 4)) // CHUNK_QUADS)


def depth_plane(H, W):
    """Additions a term of a plane sum passes through, at most: lane 2, wave 6, chunk 3, then the chunks:
    ceil(chunks / 64) strided and 6 more."""
    return 11 + -(-chunks(H, W) // 64) + 6


def depth_strided(n):
    """A wave's sum of n values: 64 strided sums in ascending order and a butterfly."""
    return -(-n // 64) + 6


# ------------------------------------------------------------------ up2T

def _fold(idx, n):
    return np.clip(idx, 0, n - 1)


def tap_t(a, b, c, d, dtype=F32):
    q, t = _c(dtype, 0.25), _c(dtype, 0.75)
    return ((q * a + t * b) + t * c) + q * d


def up2t(g, dtype=F32):
    """[..., 2h, 2w] -> [..., h, w]: columns first, then rows; an index one step outside folds onto the
    border."""
    g = np.asarray(g, dtype)
    H, W = g.shape[-2:]
    h, w = H // 2, W // 2
    c, i = np.arange(w), np.arange(h)
    u = tap_t(g[..., :, _fold(2 * c - 1, W)], g[..., :, 2 * c], g[..., :, 2 * c + 1], g[..., :, _fold(2 * c + 2, W)], dtype)
    r = [_fold(2 * i - 1 + k, H) for k in range(4)]
    out = tap_t(u[..., r[0], :], u[..., r[1], :], u[..., r[2], :], u[..., r[3], :], dtype)
    assert out.dtype == dtype
    return out


def _up2(x, dtype):
    if dtype is F32:
        return rc.up2(x)
    x = np.asarray(x, dtype)
    h, w = x.shape[-2:]
    rn, rf = rc.up_index(2 * h, h)
    cn, cf = rc.up_index(2 * w, w)
    v = 0.75 * x[..., rn, :] + 0.25 * x[..., rf, :]
    return 0.75 * v[..., :, cn] + 0.25 * v[..., :, cf]


def _sum64(terms, axes):
    """The float64 sum of float32 terms and the sum of their magnitudes."""
    t = np.asarray(terms, np.float64)
    return t.sum(axes), np.abs(t).sum(axes)


# ------------------------------------------------------------------ upmod

def upmod_bwd(g_y, x, s, up=True, dtype=F32):
    """-> g_x (stated order), (g_s in float64, sum|term|) [B,C]."""
    g_y, x, s = np.asarray(g_y, dtype), np.asarray(x, dtype), np.asarray(s, dtype)
    B = g_y.shape[0]
    sb = s[:, :, None, None]
    if up:
        assert x.shape[0] == B
        g_x = sb * up2t(g_y, dtype)
        terms = g_y * _up2(x, dtype)
    else:
        terms = g_y * x  # x of batch 1 broadcasts
        if x.shape[0] == B:
            g_x = sb * g_y
        else:  # the broadcast input: frames added in ascending order
            g_x = sb[0] * g_y[0]
            for b in range(1, B):
                g_x = g_x + sb[b] * g_y[b]
            g_x = g_x[None]
    assert g_x.dtype == dtype and terms.dtype == dtype
    return g_x, _sum64(terms, (2, 3))


# ------------------------------------------------------------------ epilogue

def epilogue_bwd(g_y, x, d, bias, noise=None, noise_weight=None, scale=None, shift=None, post=None, dtype=F32):
    """-> dict: g_x, g_scale, g_shift (stated order; None without the SFT maps) and, each as (float64 sum
    of the float32 terms, sum|term|): S_x, S_v, S_p per plane [B,C]; S_n likewise from the exact float64
    products, as the kernel forms them."""
    g_y, x = np.asarray(g_y, dtype), np.asarray(x, dtype)
    B, C = x.shape[:2]
    r2, slope = sqrt2(dtype), _c(dtype, 0.2)
    a = (r2 * np.asarray(d, dtype) if d is not None else np.full((B, C), r2, dtype))[:, :, None, None]
    nz = np.asarray(noise, dtype) if noise is not None else np.zeros((1, 1) + x.shape[2:], dtype)
    nw = _c(dtype, noise_weight) if noise is not None else _c(dtype, 0.0)
    v = ((a * x) + (nw * nz)) + np.asarray(bias, dtype).reshape(1, C, 1, 1)
    pos = v >= 0  # a NaN takes the 0.2 branch
    l = np.where(pos, v, slope * v).astype(dtype)
    g1 = g_y * np.asarray(post, dtype)[:, :, None, None] if post is not None else g_y
    if scale is not None:
        scale, shift = np.asarray(scale, dtype), np.asarray(shift, dtype)
        y1, gl = (l * scale) + shift, g1 * scale
    else:
        y1, gl = l, g1
    g_v = np.where(pos, gl, slope * gl).astype(dtype)
    out = dict(g_x=a * g_v, g_scale=g1 * l if scale is not None else None, g_shift=g1 if scale is not None else None,
               S_x=_sum64(g_v * x, (2, 3)), S_v=_sum64(g_v, (2, 3)),
               S_n=_sum64(np.asarray(g_v, np.float64) * np.asarray(nz, np.float64), (2, 3)),  # exact products
               S_p=_sum64(g_y * y1, (2, 3)), l=l)
    assert out["g_x"].dtype == dtype
    return out


# ------------------------------------------------------------------ torgb

def torgb_bwd(g_out, x, weight, s, y=None, skip=None, dtype=F32):
    """y: the forward's sigmoid output or None; skip: None, "same" or "up".
    -> dict: g_x, g_skip (stated order); m [B,O,C] and n [B,O] as (float64 sum, sum|term|)."""
    g_out, x, weight, s = (np.asarray(t, dtype) for t in (g_out, x, weight, s))
    O, C = weight.shape
    g_acc = g_out
    if y is not None:
        y = np.asarray(y, dtype)
        g_acc = g_out * (y * (_c(dtype, 1.0) - y))
    wm = weight[None, :, :] * s[:, None, :]  # [B,O,C]
    g_x = wm[:, 0, :, None, None] * g_acc[:, 0, None]
    for o in range(1, O):
        g_x = g_x + wm[:, o, :, None, None] * g_acc[:, o, None]
    g_skip = None if skip is None else (up2t(g_acc, dtype) if skip == "up" else g_acc)
    assert g_x.dtype == dtype
    return dict(g_x=g_x, g_skip=g_skip, m=_sum64(g_acc[:, :, None] * x[:, None], (3, 4)), n=_sum64(g_acc, (2, 3)))


# ------------------------------------------------------------------ coeffs

def coeffs_bwd(g_s, g_d, s, d, w2, layers, dtype=F32):
    """layers as style_coeffs takes them; w2 the flat table.  -> (g_s with the demodulated layers' share
    added, g_w2 flat): both in the header's stated order."""
    g_s, g_d, s, d, w2 = (np.asarray(t, dtype) for t in (g_s, g_d, s, d, w2))
    g_s, g_w2 = g_s.copy(), np.zeros_like(w2)
    half, two = _c(dtype, -0.5), _c(dtype, 2.0)
    for s_off, c_in, d_off, c_out, w2_off, _ in layers:
        if d_off < 0:
            continue
        dd, tab = d[:, d_off:d_off + c_out], w2[w2_off:w2_off + c_out * c_in].reshape(c_out, c_in)
        t = (half * ((dd * dd) * dd)) * g_d[:, d_off:d_off + c_out]  # [B,c_out]
        sv = s[:, s_off:s_off + c_in]
        acc = t[:, 0, None] * tab[None, 0]
        for o in range(1, c_out):
            acc = acc + t[:, o, None] * tab[None, o]
        g_s[:, s_off:s_off + c_in] = g_s[:, s_off:s_off + c_in] + (two * sv) * acc
        sq = sv * sv
        gw = t[0, :, None] * sq[0, None, :]
        for b in range(1, s.shape[0]):
            gw = gw + t[b, :, None] * sq[b, None, :]
        g_w2[w2_off:w2_off + c_out * c_in] = gw.reshape(-1)
    assert g_s.dtype == dtype and g_w2.dtype == dtype
    return g_s, g_w2
