"""CPU checks of tests/ssim_ref.py, the float64 reference and per-pixel bounds that the GPU tests of
the fused SSIM compare against: the reference is the conv2d SSIM; a plain float32 evaluation of the
same formula stays inside every bound in every input regime; and the checker rejects each of a set
of subtly wrong float64 "kernels" (negative controls)."""
import pytest
import torch
import torch.nn.functional as F

import ssim_ref as R


def _conv_ssim(img1, img2):
    """The formula of tests/test_gpu_ssim.py::_torch_ssim_map, float64 on the CPU."""
    ch = img1.shape[1]
    g = R.taps(torch.float64)
    w = (g[:, None] @ g[None, :]).expand(ch, 1, 11, 11).contiguous()
    mu1 = F.conv2d(img1, w, padding=5, groups=ch)
    mu2 = F.conv2d(img2, w, padding=5, groups=ch)
    s1 = F.conv2d(img1 * img1, w, padding=5, groups=ch) - mu1 ** 2
    s2 = F.conv2d(img2 * img2, w, padding=5, groups=ch) - mu2 ** 2
    s12 = F.conv2d(img1 * img2, w, padding=5, groups=ch) - mu1 * mu2
    return ((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 ** 2 + mu2 ** 2 + R.C1) * (s1 + s2 + R.C2))


@pytest.mark.parametrize("shape", [(2, 3, 45, 77), (1, 2, 1, 1), (1, 1, 4, 7), (1, 1, 10, 11), (2, 1, 33, 31)])
def test_reference_is_conv2d_ssim(shape):
    a, b = (t.double() for t in R.make("independent", shape, seed=3))
    ref = R.evaluate(a, b)
    assert (ref["map"] - _conv_ssim(a, b)).abs().max().item() <= 1e-12
    # the three partials are the derivatives of the map with respect to mu1, E[x1^2], E[x1 x2]
    m = [t.detach().requires_grad_(True) for t in R.moments(a, b)]
    f = R.closed_form(*m)[0]
    g_mu1, g_e11, g_e12 = torch.autograd.grad(f.sum(), (m[0], m[2], m[4]))
    for name, want in (("dm_dmu1", g_mu1), ("dm_dsigma1_sq", g_e11), ("dm_dsigma12", g_e12)):
        assert (ref[name] - want).abs().max().item() <= 1e-9 * max(1.0, want.abs().max().item()), name
    # and the backward formula is autograd of sum(dL map) through filter and closed form
    dL = R.signed(shape, 1).double()
    grad = R.gradient(a, b, dL)[0]
    got, _ = R.backward(a, b, dL, ref["dm_dmu1"], ref["dm_dsigma1_sq"], ref["dm_dsigma12"])
    assert (got - grad).abs().max().item() <= 1e-9 * max(1.0, grad.abs().max().item())


def test_constants_are_float32():
    assert R.C1 == torch.tensor(0.01 ** 2, dtype=torch.float32).item()
    assert R.C2 == torch.tensor(0.03 ** 2, dtype=torch.float32).item()
    assert R.taps().dtype == torch.float64 and torch.equal(R.taps().float(), R.TAPS32)
    assert torch.equal(R.TAPS32, R.TAPS32.flip(0))


@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_float32_evaluation_is_inside_the_forward_bounds(regime):
    a, b = R.make(regime)
    assert a.shape == R.REGIME_SHAPE and a.dtype == torch.float32
    ref, tol, cond = R.forward(a, b)
    assert R.condition_ok(cond), cond.max().item()
    got = R.evaluate(a, b, torch.float32)
    worst = 0.0
    for name in R.OUTPUTS:
        worst = max(worst, R.assert_within(got[name], ref[name], tol[name], f"{regime} {name}"))
    mean_err = abs(got["map"].mean().item() - ref["map"].mean().item())
    assert mean_err <= R.mean_tol(ref["map"], tol["map"])
    print(f"  {regime}: float32 max error/bound {worst:.3g}, condition {cond.max().item():.3g}")
    assert worst <= 1.0


def test_zero_images_have_zero_bound_where_the_reference_is_zero():
    a, b = R.make("zeros")
    ref, tol, _ = R.forward(a, b)
    assert torch.equal(ref["dm_dmu1"], torch.zeros_like(ref["dm_dmu1"])) and tol["dm_dmu1"].max().item() == 0.0
    assert (ref["map"] - 1.0).abs().max().item() <= 1e-15
    # equality is what the checker asks there
    assert R.ratio(torch.zeros(a.shape), ref["dm_dmu1"], tol["dm_dmu1"]) == 0.0
    assert R.ratio(torch.full(a.shape, 1e-30), ref["dm_dmu1"], tol["dm_dmu1"]) == float("inf")
    assert R.ratio(torch.full(a.shape, float("nan")), ref["map"], tol["map"]) == float("inf")


@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_float32_backward_is_inside_the_linear_bound(scale):
    a, b = R.make("independent")
    dL = R.signed(a.shape, 2)
    p = [R.signed(a.shape, 3 + k, scale) for k in range(3)]
    ref, tol = R.backward(a, b, dL, *p)
    got = R.gfilter(dL * p[0]) + 2.0 * a * R.gfilter(dL * p[1]) + b * R.gfilter(dL * p[2])
    assert got.dtype == torch.float32
    r = R.assert_within(got, ref, tol, f"backward scale {scale}")
    print(f"  backward, partials at scale {scale:g}: float32 max error/bound {r:.3g}")


@pytest.mark.parametrize("regime", ["independent", "noise1e-3", "masked_bg1", "wide_near"])
def test_float32_gradient_is_inside_the_end_to_end_bound(regime):
    a, b = R.make(regime)
    dL = R.signed(a.shape, 9)
    grad, tol, _, _, cond = R.gradient(a, b, dL)
    assert R.condition_ok(cond)
    f = R.evaluate(a, b, torch.float32)
    got = R.gfilter(dL * f["dm_dmu1"]) + 2.0 * a * R.gfilter(dL * f["dm_dsigma1_sq"]) + b * R.gfilter(dL * f["dm_dsigma12"])
    r = R.assert_within(got, grad, tol, f"gradient {regime}")
    print(f"  gradient {regime}: float32 max error/bound {r:.3g}")


# ---- negative controls: float64 evaluations that are each wrong in one small way ----------------------
def _drop_ends(x):
    g = R.taps()
    g[0] = g[10] = 0.0
    return R.gfilter(x, g)


def _centre_scaled(x):
    g = R.taps()
    g[5] = g[5] * (1.0 + 2.0 ** -17)
    return R.gfilter(x, g)


def _replicate(x):
    return R.gfilter(x, mode="replicate")


@pytest.mark.parametrize("name,filt", [("taps 0 and 10 dropped", _drop_ends),
                                       ("centre tap * (1 + 2^-17)", _centre_scaled),
                                       ("replicate padding", _replicate)])
def test_checker_rejects_a_wrong_filter(name, filt):
    a, b = R.make("independent")
    ref, tol, _ = R.forward(a, b)
    wrong = R.evaluate(a, b, torch.float64, filt)
    r = R.ratio(wrong["map"], ref["map"], tol["map"])
    print(f"  {name}: map at {r:.3g} of the bound")
    assert r > 1.0
    with pytest.raises(AssertionError):
        R.assert_within(wrong["map"], ref["map"], tol["map"], name)
    # all four outputs see it
    for o in R.OUTPUTS:
        assert R.ratio(wrong[o], ref[o], tol[o]) > 1.0, o


def test_checker_rejects_a_copied_seam_column():
    a, b = R.make("independent")
    ref, tol, _ = R.forward(a, b)
    for o in R.OUTPUTS:
        wrong = ref[o].clone()
        wrong[..., 32] = wrong[..., 31]
        r = R.ratio(wrong, ref[o], tol[o])
        print(f"  column 32 <- 31, {o}: {r:.3g} of the bound")
        assert r > 1.0, o
        with pytest.raises(AssertionError):
            R.assert_within(wrong, ref[o], tol[o], o)


@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_checker_rejects_dL_of_the_next_channel(scale):
    a, b = R.make("independent")
    dL = R.signed(a.shape, 2)
    p = [R.signed(a.shape, 3 + k, scale) for k in range(3)]
    ref, tol = R.backward(a, b, dL, *p)
    wrong, _ = R.backward(a, b, torch.roll(dL, -1, dims=1), *p)
    r = R.ratio(wrong, ref, tol)
    print(f"  dL of channel c+1, partials at scale {scale:g}: {r:.3g} of the bound")
    assert r > 1.0
    # the same with a dL that only differs between planes by a small factor: still far outside
    planes = 1.0 + 1e-3 * torch.arange(a.shape[0] * a.shape[1], dtype=torch.float32).reshape(a.shape[0], a.shape[1], 1, 1)
    dL2 = dL[:1, :1] * planes
    ref2, tol2 = R.backward(a, b, dL2, *p)
    wrong2, _ = R.backward(a, b, torch.roll(dL2, -1, dims=1), *p)
    assert R.ratio(wrong2, ref2, tol2) > 1.0


def test_builders_are_reproducible_and_sized():
    for regime in R.REGIMES:
        a, b = R.make(regime, (1, 2, 5, 9), seed=4)
        a2, b2 = R.make(regime, (1, 2, 5, 9), seed=4)
        assert torch.equal(a, a2) and torch.equal(b, b2) and a.shape == (1, 2, 5, 9)
        assert a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype == torch.float32
    a, _ = R.make("wide_independent")
    assert a.min().item() < -1.5 and a.max().item() > 2.5
    a, b = R.make("masked_bg1")
    assert (a == 1.0).float().mean().item() > 0.3 and not torch.equal(a, b)
