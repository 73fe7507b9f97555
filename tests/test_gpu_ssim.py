"""GPU parity of the fused SSIM (csrc/ssim.hip) against the plain-torch conv2d SSIM -- the comparison
the reference's own test makes (submodules/fused-ssim/tests/test.py:22-57, 106-140: torch.isclose
on the mean value and on img1.grad).  SSIM of random images is near 0, so the float32 mean cancels
heavily; the bound is therefore stated against a float64 evaluation of the same formula: the
kernel must be within torch.isclose's tolerance (rtol 1e-5, atol 1e-8) of it, or at least as close
as torch's own float32 conv2d path (x2).  Gradients likewise, elementwise, with a floor of 1e-9.

Those two tests only see independent random images and dL = 1/N.  The tests after them hold every
element of every output to the derived per-pixel bounds of tests/ssim_ref.py, in the regimes
training visits (near-identical, flat, masked, unclamped), at shapes around the 32-pixel tile and
the 11-tap window, with arbitrary upstream gradients, and pin the kernel's stated invariants
bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _window(ch):
    g = torch.tensor([np.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = g / g.sum()
    w2 = (g[:, None] @ g[None, :]).float()
    return w2.expand(ch, 1, 11, 11).contiguous().to(DEV)


def _torch_ssim_map(img1, img2):
    ch = img1.shape[1]
    w = _window(ch).to(img1.dtype)
    mu1 = F.conv2d(img1, w, padding=5, groups=ch)
    mu2 = F.conv2d(img2, w, padding=5, groups=ch)
    s1 = F.conv2d(img1 * img1, w, padding=5, groups=ch) - mu1 ** 2
    s2 = F.conv2d(img2 * img2, w, padding=5, groups=ch) - mu2 ** 2
    s12 = F.conv2d(img1 * img2, w, padding=5, groups=ch) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))


@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 5, 77, 45), (6, 3, 512, 512)])
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_fused_ssim_matches_conv2d(shape, padding):
    from fused_ssim import fused_ssim
    torch.manual_seed(0)
    a = torch.rand(shape, device=DEV)
    b = torch.rand(shape, device=DEV)
    def run_ref(dtype):
        x = a.clone().to(dtype).requires_grad_(True)
        m = _torch_ssim_map(x, b.to(dtype))
        if padding == "valid":
            m = m[:, :, 5:-5, 5:-5]
        v = m.mean()
        v.backward()
        return v.detach(), x.grad
    ref32, g32 = run_ref(torch.float32)
    ref64, g64 = run_ref(torch.float64)
    x_gpu = a.clone().requires_grad_(True)
    got = fused_ssim(x_gpu, b, padding=padding)
    got.backward()
    err = abs(got.item() - ref64.item())
    tol = max(1e-8 + 1e-5 * abs(ref64.item()), 2 * abs(ref32.item() - ref64.item()))
    assert err <= tol, (got.item(), ref32.item(), ref64.item())
    gerr = (x_gpu.grad.double() - g64).abs()
    gtol = torch.maximum(1e-9 + 1e-5 * g64.abs(), 2 * (g32.double() - g64).abs())
    assert (gerr <= gtol).float().mean().item() > 0.999, (gerr.max().item(), gtol.max().item())
    assert gerr.max().item() < 1e-3 * g64.abs().max().item()


def test_fused_ssim_maps_and_partials():
    """Per-pixel map vs torch, and the three partials vs autograd of the closed form."""
    from guava_renderer_amd.fused_ssim import fusedssim
    torch.manual_seed(1)
    a = torch.rand((2, 3, 50, 70), device=DEV)
    b = torch.rand((2, 3, 50, 70), device=DEV)
    m, dmu, ds1, ds12 = fusedssim(0.01 ** 2, 0.03 ** 2, a, b, True)
    ref = _torch_ssim_map(a, b)
    assert (m - ref).abs().max().item() < 2e-5
    m2, e1, e2, e3 = fusedssim(0.01 ** 2, 0.03 ** 2, a, b, False)
    assert torch.equal(m, m2) and e1.numel() == 0
    # partials: d map / d(mu1, E[x1^2], E[x1 x2]) by autograd of the closed form (the reference's
    # dm_dmu1 is the total derivative with E[x1^2], E[x1 x2] fixed; ssim.cu:267-276)
    w = _window(3)
    mu1 = F.conv2d(a, w, padding=5, groups=3).requires_grad_(True)
    mu2 = F.conv2d(b, w, padding=5, groups=3)
    e11 = F.conv2d(a * a, w, padding=5, groups=3).requires_grad_(True)
    e12 = F.conv2d(a * b, w, padding=5, groups=3).requires_grad_(True)
    s1, s12 = e11 - mu1 ** 2, e12 - mu1 * mu2
    s2 = F.conv2d(b * b, w, padding=5, groups=3) - mu2 ** 2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    f = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
    g_mu1, g_s1, g_s12 = torch.autograd.grad(f.sum(), (mu1, e11, e12))
    for got, want in ((dmu, g_mu1), (ds1, g_s1), (ds12, g_s12)):
        err = (got - want).abs().max().item()
        assert err < 1e-3 * want.abs().max().item() + 1e-4, err


# ---- per-pixel bound tests (tests/ssim_ref.py: float64 reference, derived bounds, input regimes) ------
# Every comparison below is |got - ref| <= tol at EVERY element (equality where the bound is 0), or
# bit-for-bit equality.  Each test prints its max error/bound ratio (DESIGN.md 5.4 records them).
import ctypes  # noqa: E402
import functools  # noqa: E402

import ssim_ref as R  # noqa: E402


@functools.lru_cache(maxsize=None)
def _regime(regime):
    a, b = R.make(regime)
    ref, tol, cond = R.forward(a, b)
    assert R.condition_ok(cond), (regime, cond.max().item())
    return a, b, ref, tol


def _fwd_ratio(outs, ref, tol, what):
    return max(R.assert_within(o, ref[n], tol[n], f"{what} {n}") for n, o in zip(R.OUTPUTS, outs))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_forward_and_partials_within_bounds(regime):
    from guava_renderer_amd.fused_ssim import fusedssim
    a, b, ref, tol = _regime(regime)
    ad, bd = a.to(DEV), b.to(DEV)
    outs = fusedssim(R.C1, R.C2, ad, bd, True)
    r = _fwd_ratio(outs, ref, tol, regime)
    print(f"  forward {regime}: max error/bound {r:.3g}")
    m2, e1, e2, e3 = fusedssim(R.C1, R.C2, ad, bd, False)
    assert torch.equal(m2, outs[0])
    assert e1.numel() == 0 and e2.numel() == 0 and e3.numel() == 0


_EDGE_HW = [(1, 1), (1, 40), (40, 1), (4, 7), (5, 5), (10, 11), (11, 10), (16, 16), (31, 33), (32, 32), (33, 31),
            (42, 43), (64, 65), (65, 64)]
_EDGE_CASES = [(B, CH, H, W) for (H, W) in _EDGE_HW for B in (1, 3) for CH in (1, 5)] + [(1, 32, 33, 31)]


def _edge_case(B, CH, H, W, regime, padding):
    """One shape, regime and padding: the four forward outputs, the gradient of a random signed
    upstream dL through FusedSSIMMap, and fused_ssim(...) with its backward (dL = 1/N)
    -> max error/bound ratio."""
    from guava_renderer_amd.fused_ssim import FusedSSIMMap, fused_ssim, fusedssim
    shape = (B, CH, H, W)
    a, b = R.make(regime, shape, seed=H * 100 + W)
    crop = (slice(None), slice(None), slice(5, H - 5), slice(5, W - 5)) if padding == "valid" else (Ellipsis,)
    what = f"{shape} {regime} {padding}"
    # (a) arbitrary dL through the autograd Function
    dL = torch.zeros(shape)
    dL[crop] = R.signed(shape, 11)[crop]
    grad, gtol, ref, tol, cond = R.gradient(a, b, dL)
    assert R.condition_ok(cond), what
    x = a.to(DEV).requires_grad_(True)
    m = FusedSSIMMap.apply(R.C1, R.C2, x, b.to(DEV), padding, True)
    assert m.shape == ref["map"][crop].shape
    r = R.assert_within(m, ref["map"][crop], tol["map"][crop], what + " map")
    if padding == "same":
        r = max(r, _fwd_ratio(fusedssim(R.C1, R.C2, x.detach(), b.to(DEV), True), ref, tol, what))
    (m * dL[crop].to(DEV)).sum().backward()
    r = max(r, R.assert_within(x.grad, grad, gtol, what + " gradient"))
    # (b) the mean and its gradient
    n = ref["map"][crop].numel()
    dL1 = torch.zeros(shape)
    dL1[crop] = (torch.ones((), dtype=torch.float32) / n).item()
    grad1, gtol1 = R.gradient(a, b, dL1)[:2]
    x = a.to(DEV).requires_grad_(True)
    v = fused_ssim(x, b.to(DEV), padding=padding)
    v.backward()
    verr = abs(v.item() - ref["map"][crop].mean().item())
    vtol = R.mean_tol(ref["map"][crop], tol["map"][crop])
    assert verr <= vtol, (what, verr, vtol)
    return max(r, verr / vtol, R.assert_within(x.grad, grad1, gtol1, what + " gradient of the mean"))


@pytest.mark.parametrize("B,CH,H,W", _EDGE_CASES)
def test_shape_edges_forward_and_gradient(B, CH, H, W):
    worst = 0.0
    for regime in ("noise1e-2", "masked_bg1"):
        for padding in ("same", "valid") if min(H, W) >= 11 else ("same",):
            worst = max(worst, _edge_case(B, CH, H, W, regime, padding))
    print(f"  {(B, CH, H, W)}: max error/bound {worst:.3g}")


@pytest.mark.parametrize("shape", [(2, 3, 45, 77), (1, 2, 33, 65)])
@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_backward_kernel_alone(shape, scale):
    """k_ssim_bwd on a random signed dL and random signed partial maps that no forward produced."""
    from guava_renderer_amd.fused_ssim import fusedssim_backward
    a, b = R.make("independent", shape, seed=5)
    dL = R.signed(shape, 20)
    p = [R.signed(shape, 21 + k, scale) for k in range(3)]
    ref, tol = R.backward(a, b, dL, *p)
    got = fusedssim_backward(R.C1, R.C2, a.to(DEV), b.to(DEV), dL.to(DEV), *(t.to(DEV) for t in p))
    r = R.assert_within(got, ref, tol, f"backward {shape} scale {scale:g}")
    print(f"  backward alone {shape}, partials at scale {scale:g}: max error/bound {r:.3g}")


@pytest.mark.parametrize("shape", [(2, 3, 45, 77), (1, 2, 33, 65)])
def test_backward_planes_are_independent(shape):
    """A dL that differs per channel and per batch: each plane of the batched result is, bit for bit,
    the single-plane call on that plane's inputs (a wrong plane offset cannot pass)."""
    from guava_renderer_amd.fused_ssim import fusedssim_backward
    B, CH, H, W = shape
    a, b = (t.to(DEV) for t in R.make("independent", shape, seed=6))
    planes = torch.arange(1, B * CH + 1, dtype=torch.float32).reshape(B, CH, 1, 1)
    dL = (R.signed(shape, 30) * planes).to(DEV)
    p = [R.signed(shape, 31 + k, 10.0 ** k).to(DEV) for k in range(3)]
    got = fusedssim_backward(R.C1, R.C2, a, b, dL, *p)
    for bi in range(B):
        for c in range(CH):
            s = (slice(bi, bi + 1), slice(c, c + 1))
            one = fusedssim_backward(R.C1, R.C2, a[s], b[s], dL[s], *(t[s] for t in p))
            assert torch.equal(one, got[s]), (bi, c)


@pytest.mark.parametrize("py,px", [(0, 0), (31, 31), (32, 32), (31, 32), (69, 69)])
def test_impulse_response(py, px):
    """dL = 1 at one pixel of channel 0: the gradient is exactly 0 outside that pixel's 11 x 11
    footprint (and on the whole other channel), and within bound inside it."""
    from guava_renderer_amd.fused_ssim import FusedSSIMMap
    shape = (1, 2, 70, 70)
    a, b = R.make("noise1e-2", shape, seed=7)
    dL = torch.zeros(shape)
    dL[0, 0, py, px] = 1.0
    grad, gtol, _, _, cond = R.gradient(a, b, dL)
    assert R.condition_ok(cond)
    x = a.to(DEV).requires_grad_(True)
    m = FusedSSIMMap.apply(R.C1, R.C2, x, b.to(DEV), "same", True)
    (m * dL.to(DEV)).sum().backward()
    g = x.grad.cpu()
    inside = torch.zeros(shape, dtype=torch.bool)
    inside[0, 0, max(py - 5, 0):py + 6, max(px - 5, 0):px + 6] = True
    assert bool((g[~inside] == 0).all()), "gradient outside the footprint"
    assert bool((grad[~inside] == 0).all()) and bool((gtol[~inside] == 0).all())
    assert grad[inside].abs().min().item() > 0  # (the footprint is not vacuous)
    r = R.assert_within(g, grad, gtol, f"impulse at {(py, px)}")
    print(f"  impulse at {(py, px)}: max error/bound {r:.3g}")


@pytest.mark.parametrize("oy,ox", [(0, 0), (1, 3), (27, 30), (32, 32), (40, 51)])
def test_zero_embedding_is_bit_identical(oy, ox):
    """An image pair placed on an all-zero canvas: zero padding equals canvas zeros and the tap order
    does not depend on the position, so inside the window all four outputs and (with dL zero outside
    it) dL_dimg1 are the bits of the pair alone, wherever the tile seams fall."""
    from guava_renderer_amd.fused_ssim import fusedssim, fusedssim_backward
    h, w, Hc, Wc = 37, 29, 96, 80
    small = (2, 3, h, w)
    a, b = (t.to(DEV) for t in R.make("noise1e-2", small, seed=8))
    dL = R.signed(small, 40).to(DEV)
    outs = fusedssim(R.C1, R.C2, a, b, True)
    g = fusedssim_backward(R.C1, R.C2, a, b, dL, *outs[1:])
    win = (slice(None), slice(None), slice(oy, oy + h), slice(ox, ox + w))
    A, Bc, DL = (torch.zeros((2, 3, Hc, Wc), device=DEV) for _ in range(3))
    A[win], Bc[win], DL[win] = a, b, dL
    big = fusedssim(R.C1, R.C2, A, Bc, True)
    for n, o, O in zip(R.OUTPUTS, outs, big):
        assert torch.equal(O[win], o), n
    G = fusedssim_backward(R.C1, R.C2, A, Bc, DL, *big[1:])
    assert torch.equal(G[win], g)


def test_outputs_written_everywhere_and_nowhere_else():
    """C ABI on outputs that are the middle of NaN-filled buffers with one plane of guard either side:
    every output element is written (finite), no guard element is, and a second run gives the same bits."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    B, CH, H, W = 1, 2, 33, 47
    n, guard = B * CH * H * W, H * W
    a, b = (t.to(DEV) for t in R.make("noise1e-2", (B, CH, H, W), seed=9))
    dL = R.signed((B, CH, H, W), 50).to(DEV)

    def run():
        bufs = [torch.full((n + 2 * guard,), float("nan"), device=DEV) for _ in range(5)]
        mid = [t[guard:guard + n] for t in bufs]
        _lib.check(L.gsr_fused_ssim(B, CH, H, W, R.C1, R.C2, a.data_ptr(), b.data_ptr(), *(t.data_ptr() for t in mid[:4]),
                                    _stream()), "gsr_fused_ssim")
        _lib.check(L.gsr_fused_ssim_backward(B, CH, H, W, R.C1, R.C2, a.data_ptr(), b.data_ptr(), dL.data_ptr(),
                                             *(t.data_ptr() for t in mid[1:4]), mid[4].data_ptr(), _stream()),
                   "gsr_fused_ssim_backward")
        torch.cuda.synchronize()
        return bufs

    first, second = run(), run()
    for k, (t, t2) in enumerate(zip(first, second)):
        assert bool(torch.isfinite(t[guard:guard + n]).all()), f"output {k}: an element was not written"
        assert bool(torch.isnan(t[:guard]).all()) and bool(torch.isnan(t[guard + n:]).all()), f"output {k}: guard"
        assert torch.equal(t[guard:guard + n], t2[guard:guard + n]), f"output {k}: run-to-run"
    ref, tol, _ = R.forward(a.cpu(), b.cpu())
    _fwd_ratio([t[guard:guard + n].reshape(B, CH, H, W) for t in first[:4]], ref, tol, "C ABI")


def _value_and_grad(x, b, padding="same"):
    from guava_renderer_amd.fused_ssim import fused_ssim
    x.retain_grad()
    v = fused_ssim(x, b, padding=padding)
    v.backward()
    return v.detach(), x.grad


def test_wrapper_layouts_streams_and_valid():
    from guava_renderer_amd.fused_ssim import FusedSSIMMap, fused_ssim, fusedssim
    shape = (2, 3, 37, 45)
    a, b = (t.to(DEV) for t in R.make("noise1e-2", shape, seed=10))
    outs0 = fusedssim(R.C1, R.C2, a, b, True)
    v0, g0 = _value_and_grad(a.clone().requires_grad_(True), b)
    # channels-last and a sliced view of a larger tensor: the same bits as the contiguous copy
    big = torch.rand((2, 3, 37 + 5, 45 + 5), device=DEV)
    big[:, :, 3:-2, 1:-4] = a
    for name, x in (("channels_last", a.contiguous(memory_format=torch.channels_last).requires_grad_(True)),
                    ("view", big.requires_grad_(True)[:, :, 3:-2, 1:-4])):
        assert not x.is_contiguous() and torch.equal(x, a), name
        for o, o0 in zip(fusedssim(R.C1, R.C2, x, b, True), outs0):
            assert o.is_contiguous() and torch.equal(o, o0), name
        v, g = _value_and_grad(x, b)
        assert torch.equal(v, v0) and torch.equal(g, g0), name
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[:, :, 3:-2, 1:-4] = False
    assert bool((big.grad[outside] == 0).all()) and torch.equal(big.grad[:, :, 3:-2, 1:-4], g0)
    # both images given non-contiguous
    for o, o0 in zip(fusedssim(R.C1, R.C2, a.contiguous(memory_format=torch.channels_last),
                               b.contiguous(memory_format=torch.channels_last), True), outs0):
        assert torch.equal(o, o0)
    # an expanded batch
    xe = a[:1].expand(2, -1, -1, -1)
    ae = xe.contiguous()
    assert not xe.is_contiguous()
    for o, o0 in zip(fusedssim(R.C1, R.C2, xe, b, True), fusedssim(R.C1, R.C2, ae, b, True)):
        assert torch.equal(o, o0)
    ve0, ge0 = _value_and_grad(ae.clone().requires_grad_(True), b)
    ve, ge = _value_and_grad(a[:1].clone().requires_grad_(True).expand(2, -1, -1, -1), b)
    assert torch.equal(ve, ve0) and torch.equal(ge, ge0)
    # img2.requires_grad: no gradient for img2, as in the reference
    x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    fused_ssim(x, y).backward()
    assert y.grad is None and torch.equal(x.grad, g0)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xs = a.clone().requires_grad_(True)
        vs = fused_ssim(xs, b)
        vs.backward()
        outs_s = fusedssim(R.C1, R.C2, a, b, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(vs.detach(), v0) and torch.equal(xs.grad, g0)
    for o, o0 in zip(outs_s, outs0):
        assert torch.equal(o, o0)
    # "valid" at the crop terms' 16 x 16 is "same" with dL zeroed outside the crop
    a16, b16 = (t.to(DEV) for t in R.make("noise1e-2", (2, 3, 16, 16), seed=11))
    x = a16.clone().requires_grad_(True)
    vv = fused_ssim(x, b16, padding="valid")
    vv.backward()
    x2 = a16.clone().requires_grad_(True)
    m = FusedSSIMMap.apply(R.C1, R.C2, x2, b16, "same", True)
    dL = torch.zeros_like(a16)
    dL[:, :, 5:-5, 5:-5] = torch.ones((), device=DEV) / (2 * 3 * 6 * 6)
    (m * dL).sum().backward()
    assert torch.equal(vv.detach(), m.detach()[:, :, 5:-5, 5:-5].mean())
    assert torch.equal(x.grad, x2.grad)


def test_host_side_argument_checks():
    """Calls that gsr_fused_ssim* must turn away (or finish) on the host, before any launch."""
    from guava_renderer_amd import _lib
    from guava_renderer_amd.fused_ssim import FusedSSIMMap, fusedssim, fusedssim_backward
    L = _lib.load()
    ARG = -1  # -GSR_ERR_ARG (include/gsr.h)
    for shape in ((0, 3, 8, 8), (2, 0, 8, 8), (2, 3, 0, 8)):
        e = torch.empty(shape, device=DEV)
        outs = fusedssim(R.C1, R.C2, e, e, True)
        assert all(o.shape == shape for o in outs)
        assert fusedssim_backward(R.C1, R.C2, e, e, e, *outs[1:]).shape == shape
        B, CH, H, W = shape
        assert L.gsr_fused_ssim(B, CH, H, W, R.C1, R.C2, None, None, None, None, None, None, _stream()) == 0
        assert L.gsr_fused_ssim_backward(B, CH, H, W, R.C1, R.C2, None, None, None, None, None, None, None,
                                         _stream()) == 0
    a = torch.rand((1, 1, 8, 8), device=DEV)
    out = [torch.full_like(a, float("nan")) for _ in range(4)]
    for given in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        ptrs = [out[1 + k].data_ptr() if given[k] else None for k in range(3)]
        assert L.gsr_fused_ssim(1, 1, 8, 8, R.C1, R.C2, a.data_ptr(), a.data_ptr(), out[0].data_ptr(), *ptrs,
                                _stream()) == ARG, given
        assert b"all three" in L.gsr_last_error()
    # B above the grid's z limit
    n = 65536
    many = torch.zeros((n, 1, 1, 1), device=DEV)
    outs = [torch.full_like(many, float("nan")) for _ in range(5)]
    assert L.gsr_fused_ssim(n, 1, 1, 1, R.C1, R.C2, many.data_ptr(), many.data_ptr(),
                            *(t.data_ptr() for t in outs[:4]), _stream()) == ARG
    assert L.gsr_fused_ssim_backward(n, 1, 1, 1, R.C1, R.C2, many.data_ptr(), many.data_ptr(), many.data_ptr(),
                                     *(t.data_ptr() for t in outs[1:4]), outs[4].data_ptr(), _stream()) == ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in out + outs), "a rejected call wrote an output"
    # backward of an inference forward: the partial maps do not exist
    x = a.clone().requires_grad_(True)
    m = FusedSSIMMap.apply(R.C1, R.C2, x, a, "same", False)
    with pytest.raises(RuntimeError, match="gsr_fused_ssim_backward"):
        m.sum().backward()
