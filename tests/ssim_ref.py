"""Float64 reference of the fused SSIM (csrc/ssim.hip) with per-pixel error bounds, in plain torch on
the CPU.  The GPU tests (tests/test_gpu_ssim.py) compare every element of every kernel output with
this reference and assert |got - ref| <= tol at each one; tests/test_ssim_ref.py checks the reference
and the bounds themselves.

Reference.  The separable zero-padded 11-tap filter G with the kernel's float32 taps taken to float64;
with m = G*(x1, x2, x1^2, x2^2, x1 x2) = (mu1, mu2, e11, e22, e12) and
  s1 = e11 - mu1^2, s2 = e22 - mu2^2, s12 = e12 - mu1 mu2,
  Cn = 2 mu1 mu2 + C1, D = 2 s12 + C2, A = mu1^2 + mu2^2 + C1, Bd = s1 + s2 + C2
the four outputs of the forward are
  map           = Cn D / (A Bd)
  dm_dmu1       = 2 mu2 D/(A Bd) - 2 mu2 Cn/(A Bd) - 2 mu1 Cn D/(A^2 Bd) + 2 mu1 Cn D/(A Bd^2)
  dm_dsigma1_sq = -Cn D / (A Bd^2)
  dm_dsigma12   = 2 Cn / (A Bd)
(dm_dmu1 is the total derivative with e11 and e12 held fixed) and the backward is
  dL_dimg1 = G*(dL p0) + 2 x1 G*(dL p1) + x2 G*(dL p2),   (p0, p1, p2) the three partial maps.
C1 and C2 are rounded to float32 first: the kernel receives floats.

Bounds, with u = 2^-24 (float32 unit roundoff) and mbar = G*(|x1|, |x2|, x1^2, x2^2, |x1 x2|).  They
are first-order bounds derived from the operation count, not tuned to any implementation:
  forward, each output o:  tol_o = FWD_ACC u sum_i |do/dm_i| mbar_i + FWD_OWN u |o|
      FWD_ACC = 24: a moment is two 11-tap passes = 22 accumulation roundings, plus the rounding of
      the product (x^2, x1 x2) and that of the E - mu^2 subtraction; every partial sum is bounded by
      the sum of absolute values, mbar.  FWD_OWN = 8 covers the closed form's own operations.
      do/dm_i is float64 autograd of the closed form; an input an output does not depend on counts 0.
      The bound is first order, so condition() must stay small: every case asserts it <= COND_MAX.
  backward kernel alone (linear in dL p):  tol = BWD_ACC u (G*|dL p0| + 2|x1| G*|dL p1| + |x2| G*|dL p2|)
      BWD_ACC = 26: the product dL p, 22 accumulation roundings, the product with x and the final sum.
  end-to-end gradient:  the backward bound plus the forward's partial bounds pushed through the same
      absolute-value operator, G*(|dL| tol_dmu1) + 2|x1| G*(|dL| tol_ds1) + |x2| G*(|dL| tol_ds12).
  mean value:  mean(tol_map) + MEAN_ACC u mean|map|, MEAN_ACC = 32 for the reduction.
Where reference and bound are both 0 (all-zero images) the check is equality.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FWD_ACC, FWD_OWN, BWD_ACC, MEAN_ACC = 24, 8, 26, 32
COND_MAX = 0.01
OUTPUTS = ("map", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12")

# the kernel's taps (csrc/ssim.hip kG): float32 values, written as the kernel writes them
TAPS32 = torch.tensor([0.001028380123898387, 0.0075987582094967365, 0.036000773310661316,
                       0.10936068743467331, 0.21300552785396576, 0.26601171493530273,
                       0.21300552785396576, 0.10936068743467331, 0.036000773310661316,
                       0.0075987582094967365, 0.001028380123898387], dtype=torch.float32)
C1 = float(np.float32(0.01 ** 2))
C2 = float(np.float32(0.03 ** 2))


def taps(dtype=torch.float64):
    return TAPS32.to(dtype)


def gfilter(x, g=None, mode="constant"):
    """G*x on the last two dims of [B, CH, H, W]: horizontal pass, then vertical, each a sequential
    sum over the eleven taps in x's dtype (no FMA: every product and every add rounds).  `g` replaces
    the taps, `mode` the zero padding (both only for the negative controls)."""
    g = taps(x.dtype) if g is None else g.to(x.dtype)
    H, W = x.shape[-2:]
    p = F.pad(x, (5, 5, 5, 5), mode=mode)
    h = torch.zeros_like(p[..., :, :W])
    for k in range(11):
        h = h + g[k] * p[..., :, k:k + W]
    v = torch.zeros_like(x)
    for k in range(11):
        v = v + g[k] * h[..., k:k + H, :]
    return v


def moments(x1, x2, filt=gfilter):
    return filt(x1), filt(x2), filt(x1 * x1), filt(x2 * x2), filt(x1 * x2)


def closed_form(mu1, mu2, e11, e22, e12, c1=C1, c2=C2):
    """The four outputs from the five moments, operation for operation as the kernel evaluates them."""
    s1 = e11 - mu1 * mu1
    s2 = e22 - mu2 * mu2
    s12 = e12 - mu1 * mu2
    Cn = 2.0 * (mu1 * mu2) + c1
    D = 2.0 * s12 + c2
    A = (mu1 * mu1 + mu2 * mu2) + c1
    Bd = (s1 + s2) + c2
    m = (Cn * D) / (A * Bd)
    dmu1 = (mu2 * 2.0 * D) / (A * Bd) - (mu2 * 2.0 * Cn) / (A * Bd) - (mu1 * 2.0 * Cn * D) / (A * A * Bd) \
        + (mu1 * 2.0 * Cn * D) / (A * Bd * Bd)
    ds1 = (-Cn * D) / (A * Bd * Bd)
    ds12 = (2.0 * Cn) / (A * Bd)
    return m, dmu1, ds1, ds12


def evaluate(x1, x2, dtype=torch.float64, filt=gfilter, c1=C1, c2=C2):
    """The forward in `dtype` -> dict of the four outputs.  float64: the reference; float32: a plain
    evaluation that must itself stay inside the bounds."""
    x1, x2 = x1.to(dtype), x2.to(dtype)
    return dict(zip(OUTPUTS, closed_form(*moments(x1, x2, filt), c1, c2)))


def forward(x1, x2, c1=C1, c2=C2):
    """Reference outputs, their per-pixel bounds and the first-order condition number.
    -> (ref: dict, tol: dict, cond: tensor), float64, shaped like x1."""
    x1, x2 = x1.double(), x2.double()
    m = [t.detach().requires_grad_(True) for t in moments(x1, x2)]
    mbar = moments(x1.abs(), x2.abs())
    outs = closed_form(*m, c1, c2)
    ref, tol = {}, {}
    for name, o in zip(OUTPUTS, outs):
        grads = torch.autograd.grad(o.sum(), m, retain_graph=True, allow_unused=True)
        amp = sum(g.abs() * mb for g, mb in zip(grads, mbar) if g is not None)
        ref[name] = o.detach()
        tol[name] = FWD_ACC * U * amp + FWD_OWN * U * o.detach().abs()
    mu1, mu2, e11, e22, _ = (t.detach() for t in m)
    s = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + c2
    cond = FWD_ACC * U * (mbar[2] + mbar[3] + mu1 * mu1 + mu2 * mu2) / s
    return ref, tol, cond


def condition_ok(cond):
    return bool((cond <= COND_MAX).all())


def backward(x1, x2, dL, p0, p1, p2, filt=gfilter):
    """Reference of the backward kernel alone and its bound -> (dL_dimg1, tol), float64."""
    x1, x2, dL, p0, p1, p2 = (t.double() for t in (x1, x2, dL, p0, p1, p2))
    ref = filt(dL * p0) + 2.0 * x1 * filt(dL * p1) + x2 * filt(dL * p2)
    tol = BWD_ACC * U * push_abs(x1, x2, (dL * p0).abs(), (dL * p1).abs(), (dL * p2).abs())
    return ref, tol


def push_abs(x1, x2, a0, a1, a2):
    """The backward's absolute-value operator on three non-negative maps."""
    return gfilter(a0) + 2.0 * x1.abs() * gfilter(a1) + x2.abs() * gfilter(a2)


def gradient(x1, x2, dL, c1=C1, c2=C2):
    """End to end: d sum(dL map) / d x1 by float64 autograd through filter and closed form, and the
    bound on forward + backward kernels together -> (grad, tol, fwd_ref, fwd_tol, cond)."""
    x1d, x2d, dLd = x1.double(), x2.double(), dL.double()
    x = x1d.detach().clone().requires_grad_(True)
    m = closed_form(*moments(x, x2d), c1, c2)[0]
    (grad,) = torch.autograd.grad((m * dLd).sum(), x)
    ref, tol, cond = forward(x1d, x2d, c1, c2)
    _, tb = backward(x1d, x2d, dLd, ref["dm_dmu1"], ref["dm_dsigma1_sq"], ref["dm_dsigma12"])
    a = dLd.abs()
    tg = tb + push_abs(x1d, x2d, a * tol["dm_dmu1"], a * tol["dm_dsigma1_sq"], a * tol["dm_dsigma12"])
    return grad, tg, ref, tol, cond


def mean_tol(ref_map, tol_map):
    return tol_map.mean().item() + MEAN_ACC * U * ref_map.abs().mean().item()


def ratio(got, ref, tol):
    """max over ALL elements of |got - ref| / tol; an element with tol == 0 counts 0 if it is equal
    and inf if not.  <= 1 means inside the bound everywhere.  A non-finite `got` gives inf."""
    got, ref, tol = got.detach().double().cpu(), ref.double(), tol.double()
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return r.max().item()


def assert_within(got, ref, tol, what=""):
    """|got - ref| <= tol at every element (equality where tol is 0) -> the max error/bound ratio."""
    r = ratio(got, ref, tol)
    if not r <= 1.0:
        err = (got.detach().double().cpu() - ref).abs()
        i = int(torch.argmax(torch.where(tol > 0, err / tol.clamp_min(1e-300), err * 1e300)))
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
        raise AssertionError(f"{what}: error/bound {r:.3g} at {idx}: got {got.detach().double().cpu()[idx].item():.9g}, "
                             f"ref {ref[idx].item():.9g}, tol {tol[idx].item():.3g}")
    return r


# ---- input regimes (float32 [B, CH, H, W] pairs); the GPU tests import these same builders ----------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, g):
    return torch.rand(shape, generator=g, dtype=torch.float32)


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float32)


def _smooth(shape, g):
    B, CH, H, W = shape
    y = torch.arange(H, dtype=torch.float32)[:, None]
    x = torch.arange(W, dtype=torch.float32)[None, :]
    ph = _rand((B, CH, 1, 1), g) * 6.28
    return 0.5 + 0.4 * torch.sin(0.11 * x + 0.07 * y + ph) * torch.cos(0.05 * y - 0.03 * x)


def _disc(shape):
    _, _, H, W = shape
    y = torch.arange(H, dtype=torch.float32)[:, None]
    x = torch.arange(W, dtype=torch.float32)[None, :]
    r = 0.35 * max(min(H, W), 1)
    return (((y - 0.45 * H) ** 2 + (x - 0.55 * W) ** 2) <= r * r).float().expand(shape)


def _masked(shape, g, bg):
    """A render that is `bg` outside a disc, against its target: same background, the foreground off
    by 2e-2 noise, and the target's disc one pixel wider in x (a silhouette error)."""
    m1 = _disc(shape)
    m2 = torch.maximum(m1, torch.roll(m1, 1, dims=-1)) if shape[-1] > 1 else m1
    fg = _smooth(shape, g)
    a = m1 * (fg + 2e-2 * _randn(shape, g)).clamp(0, 1) + (1 - m1) * bg
    b = m2 * fg + (1 - m2) * bg
    return a, b


def _independent(shape, g):
    return _rand(shape, g), _rand(shape, g)


def _identical(shape, g):
    a = _rand(shape, g)
    return a, a.clone()


def _noise(s):
    def build(shape, g):
        b = _rand(shape, g)
        return b + s * _randn(shape, g), b
    return build


def _constants(shape, g):
    return torch.full(shape, 0.3), torch.full(shape, 0.7)


def _same_constant(shape, g):
    return torch.full(shape, 0.6), torch.full(shape, 0.6)


def _zeros(shape, g):
    return torch.zeros(shape), torch.zeros(shape)


def _sinusoid(shape, g):
    b = _smooth(shape, g)
    return b + 1e-3 * _randn(shape, g), b


def _wide_independent(shape, g):
    return _rand(shape, g) * 5 - 2, _rand(shape, g) * 5 - 2


def _wide_near(shape, g):
    b = _rand(shape, g) * 5 - 2
    return b + 1e-2 * _randn(shape, g), b


REGIMES = {
    "independent": _independent,
    "identical": _identical,
    "noise1e-2": _noise(1e-2),
    "noise1e-3": _noise(1e-3),
    "constants": _constants,
    "sinusoid": _sinusoid,
    "masked_bg0": lambda shape, g: _masked(shape, g, 0.0),
    "masked_bg1": lambda shape, g: _masked(shape, g, 1.0),
    "wide_independent": _wide_independent,
    "wide_near": _wide_near,
    "same_constant": _same_constant,
    "zeros": _zeros,
}
REGIME_SHAPE = (2, 3, 45, 77)


def make(regime, shape=REGIME_SHAPE, seed=0):
    """The float32 CPU image pair (img1, img2) of a regime; the same bits for the same arguments."""
    a, b = REGIMES[regime](tuple(shape), _gen(1000 + seed))
    return a.contiguous(), b.contiguous()


def signed(shape, seed, scale=1.0):
    """A float32 signed random map (upstream gradients, synthetic partials)."""
    return (scale * _randn(tuple(shape), _gen(7000 + seed))).contiguous()
