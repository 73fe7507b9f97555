"""numpy float32 restatement of the UV Gaussian extraction (include/gsr_extract.h,
guava_renderer_amd/csrc/extract_dev.h), op for op: every intermediate is a float32 array, every
operation is written with the header's parentheses, there is no fused multiply-add.  The GPU test
compares the kernels against it on the bits; test_gaussian_extract_ref.py judges it against torch in
float64.
"""
import numpy as np

F32 = np.float32
LOG2E = F32(1.44269504)
LN2_HI = F32(0.693359375)        # 355/512: n * LN2_HI is exact for |n| <= 2^15
LN2_LO = F32(-2.12194440e-4)
EXP_C = tuple(F32(c) for c in (5.0000001201e-1, 1.6666665459e-1, 4.1665795894e-2, 8.3334519073e-3,
                               1.3981999507e-3, 1.9875691500e-4))
EXP_OVERFLOW = F32(88.72284)     # above: +inf
EXP_UNDERFLOW = F32(-104.0)      # below: +0
ROT_EPS = F32(1e-12)


def _f(a):
    return np.asarray(a, dtype=F32)


def _pow2(k):
    """2^k for integer k in [-126, 127] as float32, from the exponent field."""
    return ((np.asarray(k, np.int32) + 127) << 23).astype(np.uint32).view(F32)


def ex_exp(x):
    x = _f(x)
    with np.errstate(all="ignore"):
        xc = np.fmin(np.fmax(x, EXP_UNDERFLOW), EXP_OVERFLOW)  # (the clamp only keeps the lanes below finite)
        xc = np.where(np.isnan(x), F32(0), xc).astype(F32)
        n = np.floor(xc * LOG2E + F32(0.5))
        r = (xc - n * LN2_HI) - n * LN2_LO
        z = r * r
        p = EXP_C[5]
        for c in (EXP_C[4], EXP_C[3], EXP_C[2], EXP_C[1], EXP_C[0]):
            p = p * r + c
        y = (p * z + r) + F32(1.0)
        k = n.astype(np.int32)
        k1 = k >> 1
        k2 = k - k1
        y = (y * _pow2(k1)) * _pow2(k2)
        y = np.where(x > EXP_OVERFLOW, F32(np.inf), y)
        y = np.where(x < EXP_UNDERFLOW, F32(0), y)
        y = np.where(np.isnan(x), x, y)
    return y.astype(F32)


def ex_sigmoid(x):
    with np.errstate(all="ignore"):
        return (F32(1.0) / (F32(1.0) + ex_exp(-_f(x)))).astype(F32)


ROT_LO, ROT_HI = F32(1e-24), F32(1e30)  # the range of S in which the norm is refined
SPLIT = F32(4097.0)                      # Dekker's splitter for a 24-bit significand


def _two_sum(a, b):
    """s = a + b and its rounding error (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _square(a):
    """p = a*a and its rounding error (Dekker, no fma)."""
    p = a * a
    t = SPLIT * a
    hi = t - (t - a)
    lo = a - hi
    return p, ((hi * hi - p) + (hi + hi) * lo) + lo * lo


def rot_norm(x):
    """x [...,4] -> (n, d).  S = ((x0*x0 + x1*x1) + x2*x2) + x3*x3, n0 = sqrtf(S).  For
    1e-24f <= S <= 1e30f the norm is refined by the rounding errors of S (c) and one Newton step,
    n = n0 + (((S - p) - pe) + c) / (n0 + n0) with (p, pe) the exact square of n0; otherwise n = n0.
    d = fmaxf(n, 1e-12f)."""
    x = _f(x)
    with np.errstate(all="ignore"):
        p0, e0 = _square(x[..., 0])
        p1, e1 = _square(x[..., 1])
        p2, e2 = _square(x[..., 2])
        p3, e3 = _square(x[..., 3])
        s1, f1 = _two_sum(p0, p1)
        s2, f2 = _two_sum(s1, p2)
        S, f3 = _two_sum(s2, p3)
        c = ((e0 + e1) + (e2 + e3)) + ((f1 + f2) + f3)
        n0 = np.sqrt(S)
        p, pe = _square(n0)
        n1 = n0 + (((S - p) - pe) + c) / (n0 + n0)
        n = np.where((S >= ROT_LO) & (S <= ROT_HI), n1, n0)
        d = np.fmax(n, ROT_EPS)  # fmaxf: a NaN n gives 1e-12f
    return n.astype(F32), d.astype(F32)


def rot_forward(x):
    n, d = rot_norm(x)
    with np.errstate(all="ignore"):
        return (_f(x) / d[..., None]).astype(F32)


def rot_backward(x, g):
    x, g = _f(x), _f(g)
    n, d = rot_norm(x)
    with np.errstate(all="ignore"):
        y = x / d[..., None]
        s = ((g[..., 0] * y[..., 0] + g[..., 1] * y[..., 1]) + g[..., 2] * y[..., 2]) + g[..., 3] * y[..., 3]
        full = (g - y * s[..., None]) / d[..., None]
        clamp = g / d[..., None]
    return np.where((n >= ROT_EPS)[..., None], full, clamp).astype(F32)


def sigmoid_backward(x, g):
    y = ex_sigmoid(x)
    with np.errstate(all="ignore"):
        return ((_f(g) * (F32(1.0) - y)) * y).astype(F32)


def exp_backward(x, g):
    with np.errstate(all="ignore"):
        return (_f(g) * ex_exp(x)).astype(F32)


# ---- tile and slot arithmetic ------------------------------------------------------------------------

def tile_bases(keep):
    """keep bool [T] -> int32 [ceil(T/64) + 1]: the exclusive scan of the per-tile counts, total last."""
    keep = np.asarray(keep, bool)
    T = keep.shape[0]
    nt = (T + 63) // 64
    pad = np.zeros(nt * 64, bool)
    pad[:T] = keep
    out = np.zeros(nt + 1, np.int32)
    out[1:] = np.cumsum(pad.reshape(nt, 64).sum(1))
    return out


def slots(keep):
    """keep bool [T] -> int64 [T]: tile_base[tile] + the kept lanes below, -1 for a dropped texel."""
    keep = np.asarray(keep, bool)
    T = keep.shape[0]
    base = tile_bases(keep)
    s = np.full(T, -1, np.int64)
    for tile in range(base.shape[0] - 1):
        k = keep[tile * 64:(tile + 1) * 64]
        below = np.cumsum(k) - k
        s[tile * 64:tile * 64 + k.shape[0]] = np.where(k, base[tile] + below, -1)
    return s


KEYS = ("colors", "opacities", "scales", "rotations", "local_pos")
WIDTH = dict(opacities=1, scales=3, rotations=4, local_pos=3)


def to_rows(maps, raw):
    """The five maps as [B,T,k] arrays: planar [B,k,U,U] (raw) transposed, rows [B,U,U,k] reshaped."""
    out = {}
    for key in KEYS:
        m = _f(maps[key])
        B = m.shape[0]
        out[key] = m.reshape(B, m.shape[1], -1).transpose(0, 2, 1) if raw else m.reshape(B, -1, m.shape[-1])
    return out


def activate(rows, raw, rgb_sigmoid):
    """Per-texel forward on [B,T,k] rows (every texel, masked or not)."""
    col = rows["colors"].copy()
    if rgb_sigmoid:
        col[..., :3] = ex_sigmoid(col[..., :3])
    if not raw:
        return dict(rows, colors=col)
    return dict(colors=col, opacities=ex_sigmoid(rows["opacities"]), scales=ex_exp(rows["scales"]),
                rotations=rot_forward(rows["rotations"]), local_pos=rows["local_pos"].copy())


def extract(maps, mask, raw=True, rgb_sigmoid=True, threshold=None, texel_face=None, texel_bary=None):
    """The forward.  mask [T] (0/1).  threshold None: tables of N = mask.sum() rows.  Else (B = 1) the
    predicate is mask && opacity > threshold on the float32 opacity; tables keep N rows, rows
    [count, N) are zeros.  -> dict of the five tables [B,N,k], 'count', and with texel_face / texel_bary
    'binding_face' int32 [N] and 'face_bary' [N,3]."""
    mask = np.asarray(mask).reshape(-1) != 0
    act = activate(to_rows(maps, raw), raw, rgb_sigmoid)
    N = int(mask.sum())
    keep = mask
    if threshold is not None:
        assert act["opacities"].shape[0] == 1
        with np.errstate(invalid="ignore"):
            keep = mask & (act["opacities"][0, :, 0] > F32(threshold))
    s = slots(keep)
    sel = np.nonzero(keep)[0]
    assert np.array_equal(s[sel], np.arange(sel.size))  # ascending in texel order: the boolean gather's order
    out = {"count": int(sel.size)}
    for key in KEYS:
        a = act[key]
        t = np.zeros((a.shape[0], N, a.shape[2]), F32)
        t[:, :sel.size] = a[:, sel]
        out[key] = t
    if texel_face is not None:
        bf = np.zeros(N, np.int32)
        bf[:sel.size] = np.asarray(texel_face, np.int32).reshape(-1)[sel]
        fb = np.zeros((N, 3), F32)
        fb[:sel.size] = _f(texel_bary).reshape(-1, 3)[sel]
        out["binding_face"], out["face_bary"] = bf, fb
    return out


def extract_backward(maps, mask, grads, raw=True, rgb_sigmoid=True):
    """grads: dict of the five table gradients [B,N,k] -> dict of map gradients in the maps' layout
    (planar [B,k,U,U] when raw, rows [B,U,U,k] otherwise); a texel outside the mask gets +0."""
    mask = np.asarray(mask).reshape(-1) != 0
    rows = to_rows(maps, raw)
    sel = np.nonzero(mask)[0]
    out = {}
    for key in KEYS:
        x = rows[key][:, sel]
        g = _f(grads[key])
        if key == "colors":
            d = g.copy()
            if rgb_sigmoid:
                d[..., :3] = sigmoid_backward(x[..., :3], g[..., :3])
        elif not raw or key == "local_pos":
            d = g.copy()
        elif key == "opacities":
            d = sigmoid_backward(x, g)
        elif key == "scales":
            d = exp_backward(x, g)
        else:
            d = rot_backward(x, g)
        full = np.zeros(rows[key].shape, F32)
        full[:, sel] = d
        m = _f(maps[key])
        out[key] = (np.ascontiguousarray(full.transpose(0, 2, 1)).reshape(m.shape) if raw else full.reshape(m.shape))
    return out
