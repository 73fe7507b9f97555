"""GPU tests of the refiner decoder's glue (include/gsr_refiner.h, csrc/refiner.hip,
guava_renderer_amd/refiner.py).

upmod, epilogue and torgb are compared on the bits against tests/refiner_cases.py, the numpy restatement
of their stated float32 arithmetic; coeffs, whose sums have the kernel's own order, against float64
within the header's bounds.  The whole decoder runs on the weights and inputs of
tests/golden/refiner_decoder.npz against the reference project's own float64 outputs: 1e-5 of scale
before the sigmoid, 1e-5 absolute after it (the project's bar against a float64 restatement, DESIGN.md
1 row f3); StyleUNetRunner against tests/refiner_ref.py's StyleUNet in float64 at the same bar.
"""
import functools

import numpy as np
import pytest
import torch

import helpers
import refiner_cases as rc
import refiner_ref
from refiner_cases import BAR, CFG, load_variant, scale_err, sigmoid64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits_equal(got, want):
    got = got.cpu().numpy()
    want = np.ascontiguousarray(want, np.float32)
    return got.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _rng(*key):
    return np.random.default_rng(list(key))


def _normal(rng, shape, scale=1.0):
    return (rng.normal(size=shape) * scale).astype(np.float32)


# ------------------------------------------------------------------ upmod

@pytest.mark.parametrize("B,C,h,w,up,xb", [
    (2, 3, 4, 4, True, 2),    # 8x8: every lane's four pixels touch a clamped edge
    (2, 3, 4, 12, True, 2),   # 8x24: H != W
    (2, 3, 2, 2, True, 2),    # 4x4: one lane per row
    (3, 3, 4, 4, False, 1),   # the plain scale, x of batch 1 broadcast
    (2, 5, 20, 36, True, 2),  # more than one workgroup
])
def test_upmod(B, C, h, w, up, xb):
    from guava_renderer_amd import refiner
    rng = _rng(1, B, C, h, w)
    x, s = _normal(rng, (xb, C, h, w)), _normal(rng, (B, C))
    y = refiner.style_upmod(_d(x), _d(s), up=up)
    assert _bits_equal(y, rc.upmod(x, s, up))


def test_upmod_strided_coefficients():
    """s as a column range of a wider table, as the decoder passes it."""
    from guava_renderer_amd import refiner
    rng = _rng(2)
    x, table = _normal(rng, (2, 3, 4, 4)), _normal(rng, (2, 11))
    y = refiner.style_upmod(_d(x), _d(table)[:, 5:8], up=True)
    assert _bits_equal(y, rc.upmod(x, table[:, 5:8], True))


def test_upmod_rejects_width_6():
    from guava_renderer_amd import refiner
    x, s = torch.zeros((2, 3, 3, 3), device=DEV), torch.ones((2, 3), device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        refiner.style_upmod(x, s, up=True)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        refiner.style_upmod(torch.zeros((2, 3, 4, 6), device=DEV), s, up=False)


# ------------------------------------------------------------------ epilogue

@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("sft", [False, True])
@pytest.mark.parametrize("noise_batch", [0, 1, 3])
def test_epilogue(noise_batch, sft, post):
    from guava_renderer_amd import refiner
    B, C, H, W = 3, 5, 4, 4  # a plane of 16 elements: several planes per wave
    rng = _rng(3, noise_batch, sft, post)
    x, d, bias = _normal(rng, (B, C, H, W), 2.0), np.abs(_normal(rng, (B, C))) + np.float32(0.1), _normal(rng, (C,))
    noise = _normal(rng, (noise_batch, 1, H, W)) if noise_batch else None
    nw = np.float32(0.7)
    scale, shift = (_normal(rng, (B, C, H, W)), _normal(rng, (B, C, H, W))) if sft else (None, None)
    ps = _normal(rng, (B, C)) if post else None
    assert (x < 0).any() and (x > 0).any()
    want = rc.epilogue(x, d, bias, noise, nw, scale, shift, ps)
    opt = lambda a: None if a is None else _d(a)  # noqa: E731
    y = refiner.style_epilogue(_d(x), _d(d), _d(bias).reshape(1, C, 1, 1), opt(noise), _d(np.array([nw])), opt(scale),
                               opt(shift), opt(ps))
    assert _bits_equal(y, want)
    assert (want < 0).any() and (want > 0).any()


def test_epilogue_in_place_and_larger():
    from guava_renderer_amd import refiner
    B, C, H, W = 2, 3, 24, 40  # more than one workgroup
    rng = _rng(4)
    x, d, bias = _normal(rng, (B, C, H, W)), np.abs(_normal(rng, (B, C))) + np.float32(0.1), _normal(rng, (C,))
    noise, scale, shift = _normal(rng, (B, 1, H, W)), _normal(rng, (B, C, H, W)), _normal(rng, (B, C, H, W))
    want = rc.epilogue(x, d, bias, noise, np.float32(-0.3), scale, shift, None)
    xg = _d(x)
    y = refiner.style_epilogue(xg, _d(d), _d(bias), _d(noise), _d(np.array([-0.3], np.float32)), _d(scale), _d(shift),
                               out=xg)
    assert y.data_ptr() == xg.data_ptr()
    assert _bits_equal(xg, want)
    # without a demodulation factor
    y = refiner.style_epilogue(_d(x), None, _d(bias))
    assert _bits_equal(y, rc.epilogue(x, None, bias))


# ------------------------------------------------------------------ torgb

@pytest.mark.parametrize("C,O,skip,sigmoid", [
    (1, 1, None, False), (7, 3, "same", False), (256, 4, "up", True), (7, 4, "up", False), (256, 3, None, True),
    (1, 3, "same", True), (7, 1, "up", True),
])
def test_torgb(C, O, skip, sigmoid):
    from guava_renderer_amd import refiner
    B, H, W = 2, 8, 8
    rng = _rng(5, C, O, sigmoid)
    x, w, s, bias = _normal(rng, (B, C, H, W)), _normal(rng, (O, C), 0.5), _normal(rng, (B, C)), _normal(rng, (O,))
    sk = None if skip is None else _normal(rng, (B, O, H, W) if skip == "same" else (B, O, H // 2, W // 2))
    want = rc.torgb(x, w, s, bias, sk, skip_up=skip == "up", sigmoid=sigmoid)
    y = refiner.style_torgb(_d(x), _d(w), _d(s), _d(bias).reshape(1, O, 1, 1), None if sk is None else _d(sk),
                            skip_up=skip == "up", sigmoid=sigmoid)
    assert _bits_equal(y, want)


def test_torgb_limits():
    from guava_renderer_amd import refiner
    z = lambda *shape: torch.zeros(shape, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError):
        refiner.style_torgb(z(1, 2, 4, 4), z(5, 2), z(1, 2), z(5))      # out_dim 5
    with pytest.raises(RuntimeError):
        refiner.style_torgb(z(1, 513, 4, 4), z(3, 513), z(1, 513), z(3))  # C 513


# ------------------------------------------------------------------ coeffs

def test_coeffs():
    from guava_renderer_amd import refiner
    B, S, eps = 3, 64, 1e-8
    rng = _rng(6)
    # (c_in, c_out or 0 for a ToRGB-like layer without demodulation)
    shapes = [(1, 5), (7, 0), (130, 3), (3, 2)]
    latent = _normal(rng, (B, S))
    sum_in = sum(c for c, _ in shapes)
    mw, mb = _normal(rng, (sum_in, S), 0.2), _normal(rng, (sum_in,)) + np.float32(1.0)
    mw[-3:], mb[-3:] = 0.0, 0.0  # the last layer: s = 0 exactly
    layers, w2, s_off, d_off = [], [], 0, 0
    for c_in, c_out in shapes:
        layers.append((s_off, c_in, d_off if c_out else -1, c_out or 3, sum(t.size for t in w2), eps))
        if c_out:
            w2.append(np.abs(_normal(rng, (c_out, c_in))) + np.float32(0.01))
            d_off += c_out
        s_off += c_in
    s, d = refiner.style_coeffs(_d(latent), _d(mw), _d(mb), _d(np.concatenate([t.reshape(-1) for t in w2])), layers, d_off)
    s, d = s.cpu().numpy(), d.cpu().numpy()
    assert s.shape == (B, sum_in) and d.shape == (B, d_off)
    s64, mag = rc.coeffs64(latent, mw, mb)
    excess = np.abs(s - s64) - (S + 2) * U * mag
    print(f"  s: max error / bound {float((np.abs(s - s64) / np.maximum((S + 2) * U * mag, 1e-300)).max()):.3g}")
    assert (excess <= 0).all()
    tables = iter(w2)
    for (so, c_in, do, c_out, _, _), (_, has_d) in zip(layers, shapes):
        if not has_d:
            continue
        want = rc.demod64(s[:, so:so + c_in], next(tables), eps)
        rel = np.abs(d[:, do:do + c_out] - want) / want
        print(f"  d (c_in {c_in}): max relative error {float(rel.max()) / U:.3g} * 2^-24, bound {c_in + 4}")
        assert (rel <= (c_in + 4) * U).all()
    assert np.array_equal(s[:, -3:], np.zeros((B, 3), np.float32))
    assert np.array_equal(d[:, -2:], np.full((B, 2), np.float32(1.0) / np.sqrt(np.float32(eps)), np.float32))


# ------------------------------------------------------------------ the whole decoder

@functools.lru_cache(maxsize=None)
def _golden(v):
    return load_variant(v)


@pytest.mark.parametrize("v", ["full", "small"])
def test_decoder_against_reference_float64(v):
    from guava_renderer_amd.refiner import StyleDecoder
    sd, style, cond, noise, out = _golden(v)
    dec = StyleDecoder.from_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, CFG["out_size"], v == "small",
                                       device=DEV)
    ref32 = refiner_ref.load_reference_state(refiner_ref.StyleDecoderRef(small=v == "small", **CFG), sd).to(DEV).eval()
    with torch.no_grad():
        args = (_d(style), [_d(c) for c in cond], [_d(n) for n in noise])
        y = dec.forward(*args).cpu().numpy()
        ys = dec.forward(*args, sigmoid=True).cpu().numpy()
        r = ref32(*args).cpu().numpy()
    err, err_s, err_r = scale_err(y, out), float(np.abs(ys - sigmoid64(out)).max()), scale_err(r, out)
    print(f"  {v}: StyleDecoder {err:.3g} of scale ({err_s:.3g} absolute after the sigmoid); the torch restatement "
          f"in float32 on the GPU {err_r:.3g}; ratio {err / max(err_r, 1e-30):.2f} (NOISE_FACTOR {helpers.NOISE_FACTOR})")
    assert y.shape == out.shape and y.dtype == np.float32
    assert err <= BAR
    assert err_s <= BAR


def test_decoder_draws_noise_and_checks_inputs():
    from guava_renderer_amd.refiner import StyleDecoder
    sd, style, cond, noise, _ = _golden("small")
    dec = StyleDecoder.from_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, CFG["out_size"], True, device=DEV)
    args = (_d(style), [_d(c) for c in cond])
    with torch.no_grad():
        g = torch.Generator(device=DEV)
        a = dec.forward(*args, generator=g.manual_seed(7))
        b = dec.forward(*args, generator=g.manual_seed(7))
        c = dec.forward(*args, generator=g.manual_seed(8))
        assert torch.equal(a, b) and not torch.equal(a, c)
        with pytest.raises(RuntimeError, match="one per style conv"):
            dec.forward(*args, noise=[_d(n) for n in noise[:-1]])
        with pytest.raises(RuntimeError, match="GPU only"):
            dec.forward(torch.from_numpy(style), args[1])
    with pytest.raises(NotImplementedError):
        dec.forward(_d(style).requires_grad_(True), args[1])


# ------------------------------------------------------------------ StyleUNetRunner

@pytest.mark.parametrize("small", [True, False])
def test_runner(small):
    from guava_renderer_amd.refiner import StyleUNetRunner
    torch.manual_seed(21)
    net = refiner_ref.StyleUNetRef(in_size=16, out_size=16, in_dim=32, out_dim=3, num_style_feat=64, num_mlp=2,
                                   activation=True, channel_scale=32, small=small).eval()
    refiner_ref.randomize_noise_params(net, 9)
    g = torch.Generator().manual_seed(22)
    x = torch.rand((2, 32, 16, 16), generator=g)
    noise = [torch.randn((2, 1, n, n), generator=g) for n in net.stylegan_decoder.noise_sizes()]
    with torch.no_grad():
        import copy
        want = copy.deepcopy(net).double()(x.double(), [n.double() for n in noise]).numpy()
    net = net.to(DEV)
    run = StyleUNetRunner(net)
    xg, ng = x.to(DEV), [n.to(DEV) for n in noise]
    with torch.no_grad():
        y = run.forward(xg, noise=ng)
        feat = torch.nn.functional.leaky_relu_(net.conv_body_first(xg), negative_slope=0.2)
        z = run.rest(feat, noise=ng)
    assert torch.equal(y, z)
    err = float(np.abs(y.cpu().numpy() - want).max())
    print(f"  small={small}: StyleUNetRunner vs the float64 StyleUNet: {err:.3g} absolute (after the sigmoid)")
    assert tuple(y.shape) == (2, 3, 16, 16) and err <= BAR
    # a parameter requires grad and grad is enabled: no backward yet
    assert next(net.parameters()).requires_grad
    with pytest.raises(NotImplementedError):
        run.forward(xg, noise=ng)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU only"):
            run.forward(x, noise=ng)
        with pytest.raises(RuntimeError, match="GPU only"):
            run.rest(feat.cpu(), noise=ng)
