"""The refiner decoder's two references, judged on the CPU against the reference project's own float64
outputs (tests/golden/refiner_decoder.npz, built by tests/golden/make_refiner_golden.py):
  * tests/refiner_ref.py, the torch restatement (grouped-conv formulation), in float64: 1e-12;
  * tests/refiner_cases.py, the numpy restatement of the four HIP kernels' stated float32 arithmetic,
    chained with a float64 conv as guava_renderer_amd/refiner.py chains the kernels with F.conv2d: the
    GPU test's bar, 1e-5 of scale before the sigmoid and 1e-5 absolute after it.
"""
import os

import numpy as np
import pytest
import torch

import refiner_cases as rc
import refiner_ref
from refiner_cases import BAR, CFG, GOLDEN, load_variant, scale_err, sigmoid64


def test_golden_is_small_and_nontrivial():
    assert os.path.getsize(GOLDEN) < 400 * 1024
    for v in ("full", "small"):
        sd, style, cond, noise, out = load_variant(v)
        assert out.dtype == np.float64 and out.shape == (2, 3, 16, 16)
        assert len(noise) == (5 if v == "full" else 3) and len(cond) == 4
        assert all(np.abs(sd[k]).min() > 0 for k in sd if k.endswith("style_conv1.weight") or k.endswith(".bias"))


@pytest.mark.parametrize("v", ["full", "small"])
def test_torch_restatement_float64(v):
    sd, style, cond, noise, out = load_variant(v)
    dec = refiner_ref.load_reference_state(refiner_ref.StyleDecoderRef(small=v == "small", **CFG), sd).double().eval()
    t = lambda a: torch.from_numpy(a).double()  # noqa: E731
    with torch.no_grad():
        y = dec(t(style), [t(c) for c in cond], [t(n) for n in noise]).numpy()
    err = scale_err(y, out)
    print(f"  {v}: torch restatement (float64) vs the reference: {err:.3g} of scale")
    assert err <= 1e-12


@pytest.mark.parametrize("v", ["full", "small"])
def test_kernel_arithmetic_chain(v):
    sd, style, cond, noise, out = load_variant(v)
    y = rc.decoder(sd, v == "small", style, cond, noise)
    assert y.dtype == np.float32
    err = scale_err(y, out)
    ys = rc.decoder(sd, v == "small", style, cond, noise, sigmoid=True)
    err_s = float(np.abs(ys.astype(np.float64) - sigmoid64(out)).max())
    print(f"  {v}: kernels' float32 arithmetic + float64 conv vs the reference: {err:.3g} of scale, "
          f"{err_s:.3g} absolute after the sigmoid")
    assert err <= BAR and err_s <= BAR


def test_up2_is_torch_bilinear():
    """The stated taps are F.interpolate(x2, bilinear, align_corners=False), H != W included."""
    rng = np.random.default_rng(0)
    x = rng.normal(size=(2, 3, 4, 12)).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(x).double(), scale_factor=2, mode="bilinear",
                                           align_corners=False).numpy()
    got = rc.up2(x)
    assert got.shape == (2, 3, 8, 24)
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(x).max()
    assert np.array_equal(rc.up2(np.full((1, 1, 2, 2), 3.0, np.float32)), np.full((1, 1, 4, 4), 3.0, np.float32))


def test_modulated_conv_as_plain_conv():
    """conv(x, W*s*d) == d * conv(s*x, W), the identity the HIP path rests on, in float64."""
    g = torch.Generator().manual_seed(3)
    m = refiner_ref.ModulatedConv2d(5, 7, 3, 16, True, True).double()
    x, style = torch.randn((2, 5, 4, 6), generator=g).double(), torch.randn((2, 16), generator=g).double()
    with torch.no_grad():
        want = m(x, style).numpy()
        s = m.modulation(style).numpy()
        w = m.weight[0].numpy()
    d = rc.demod64(s, (w ** 2).sum((-1, -2)), m.eps)
    xs = torch.from_numpy(s)[:, :, None, None] * refiner_ref.up2(x)
    got = torch.nn.functional.conv2d(xs, torch.from_numpy(w), padding=1).numpy() * d[:, :, None, None]
    assert scale_err(got, want) <= 1e-13
