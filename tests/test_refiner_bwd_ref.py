"""The references of the refiner decoder's backward, judged on the CPU:
  * tests/refiner_bwd_cases.py, the numpy restatement of the four HIP backward passes, run in float64
    against float64 torch autograd of tests/refiner_ref.py's modules, op by op (the ops of both decoder
    variants: with and without the SFT maps, with the second conv's modulation folded in as `post`, the
    ToRGB with a x2 skip, the demodulated conv as upmod + plain conv + output scale): 1e-12 of scale, the
    bar tests/test_refiner_ref.py sets for the forward;
  * up2T against up2: the adjoint identity, and against autograd of F.interpolate;
  * tests/golden/refiner_decoder_grad.npz, the reference project's own float64 gradients, against
    refiner_ref's float64 autograd: 1e-12 of scale.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import refiner_bwd_cases as rb
import refiner_cases as rc
import refiner_ref
from refiner_bwd_cases import GRAD_GOLDEN, load_grad_golden, scale_err
from refiner_cases import CFG, load_variant

F64 = np.float64


def _t(a, grad=True):
    return torch.from_numpy(np.asarray(a, F64)).requires_grad_(grad)


def _rng(*key):
    return np.random.default_rng(list(key))


# ------------------------------------------------------------------ up2T

@pytest.mark.parametrize("h,w", [(1, 2), (2, 2), (4, 12), (5, 6), (3, 2)])
def test_up2t_is_the_adjoint_of_up2(h, w):
    rng = _rng(1, h, w)
    x, g = rng.normal(size=(2, 3, h, w)), rng.normal(size=(2, 3, 2 * h, 2 * w))
    lhs, rhs = float((rb._up2(x, F64) * g).sum()), float((x * rb.up2t(g, F64)).sum())
    assert abs(lhs - rhs) <= 1e-13 * np.abs(rb._up2(x, F64) * g).sum()
    xt = _t(x)
    (refiner_ref.up2(xt) * torch.from_numpy(g)).sum().backward()
    assert scale_err(rb.up2t(g, F64), xt.grad.numpy()) <= 1e-13
    # float32, as the kernels run it: each side rounds a sample within 4 * 2^-24
    x32, g32 = x.astype(np.float32), g.astype(np.float32)
    a = (rc.up2(x32).astype(F64) * g32).sum()
    b = (x32.astype(F64) * rb.up2t(g32)).sum()
    assert abs(a - b) <= 16 * rb.U * np.abs(rc.up2(x32).astype(F64) * g32).sum()
    # a constant g: every input pixel collects exactly 4 g, the folded border included
    assert np.array_equal(rb.up2t(np.full((1, 1, 2 * h, 2 * w), -3.5, np.float32)), np.full((1, 1, h, w), -14.0, np.float32))


# ------------------------------------------------------------------ op by op, float64

@pytest.mark.parametrize("up,xb", [(True, 2), (False, 2), (False, 1)])
def test_upmod_backward(up, xb):
    rng = _rng(2, up, xb)
    B, C, h, w = 2, 3, 4, 6
    x, s = rng.normal(size=(xb, C, h, w)), rng.normal(size=(B, C))
    G = rng.normal(size=(B, C, 2 * h, 2 * w) if up else (B, C, h, w))
    xt, st = _t(x), _t(s)
    y = st[:, :, None, None] * (refiner_ref.up2(xt) if up else xt)
    (y * torch.from_numpy(G)).sum().backward()
    g_x, (g_s, _) = rb.upmod_bwd(G, x, s, up, dtype=F64)
    assert scale_err(g_x, xt.grad.numpy()) <= 1e-12 and scale_err(g_s, st.grad.numpy()) <= 1e-12


# (SFT maps, post, noise batch): the full decoder's first conv of a level, its second conv / conv1
# (batch-1 noise), and the small decoder's style conv
@pytest.mark.parametrize("sft,post,nb", [(True, True, 2), (False, False, 1), (True, False, 2), (False, False, 0)])
def test_epilogue_backward(sft, post, nb):
    rng = _rng(3, sft, post, nb)
    B, C, H, W = 2, 3, 4, 8
    x, d, bias = rng.normal(size=(B, C, H, W)) * 2, np.abs(rng.normal(size=(B, C))) + 0.1, rng.normal(size=(C,))
    noise, nw = (rng.normal(size=(nb, 1, H, W)), 0.7) if nb else (None, None)
    scale, shift = (rng.normal(size=(B, C, H, W)), rng.normal(size=(B, C, H, W))) if sft else (None, None)
    ps = rng.normal(size=(B, C)) if post else None
    G = rng.normal(size=(B, C, H, W))
    t = {k: _t(v) for k, v in dict(x=x, d=d, bias=bias, nw=nw, scale=scale, shift=shift, ps=ps).items() if v is not None}
    v = 2 ** 0.5 * t["d"][:, :, None, None] * t["x"] + t["bias"].view(1, C, 1, 1)
    if nb:
        v = v + t["nw"] * torch.from_numpy(noise)
    y = F.leaky_relu(v, 0.2)
    assert bool((v < 0).any()) and bool((v > 0).any())
    if sft:
        y = y * t["scale"] + t["shift"]
    if post:
        y = y * t["ps"][:, :, None, None]
    (y * torch.from_numpy(G)).sum().backward()
    r = rb.epilogue_bwd(G, x, d, bias, noise, nw, scale, shift, ps, dtype=F64)
    assert scale_err(r["g_x"], t["x"].grad.numpy()) <= 1e-12
    assert scale_err(2 ** 0.5 * r["S_x"][0], t["d"].grad.numpy()) <= 1e-12
    assert scale_err(r["S_v"][0].sum(0), t["bias"].grad.numpy()) <= 1e-12
    if nb:
        assert scale_err(r["S_n"][0].sum(), t["nw"].grad.numpy()) <= 1e-12
    if sft:
        assert scale_err(r["g_scale"], t["scale"].grad.numpy()) <= 1e-12
        assert scale_err(r["g_shift"], t["shift"].grad.numpy()) <= 1e-12
    if post:
        assert scale_err(r["S_p"][0], t["ps"].grad.numpy()) <= 1e-12


@pytest.mark.parametrize("skip,sigmoid", [(None, False), ("up", False), ("up", True), ("same", True)])
def test_torgb_backward(skip, sigmoid):
    """refiner_ref.ToRGB (the grouped-conv formulation) under float64 autograd."""
    rng = _rng(4, skip is None, sigmoid)
    B, C, O, H, W, S = 2, 5, 3, 4, 8, 6
    m = refiner_ref.ToRGB(C, O, S, upsample=skip == "up").double()
    with torch.no_grad():
        m.bias.copy_(torch.from_numpy(rng.normal(size=(1, O, 1, 1))))
    x, style = _t(rng.normal(size=(B, C, H, W))), _t(rng.normal(size=(B, S)))
    sk = None if skip is None else _t(rng.normal(size=(B, O, H // 2, W // 2) if skip == "up" else (B, O, H, W)))
    G = rng.normal(size=(B, O, H, W))
    y = m(x, style, sk)
    y = torch.sigmoid(y) if sigmoid else y
    (y * torch.from_numpy(G)).sum().backward()
    with torch.no_grad():
        s = m.modulated_conv.modulation(style).numpy()
    w = m.modulated_conv.weight.detach().numpy().reshape(O, C)
    r = rb.torgb_bwd(G, x.detach().numpy(), w, s, y.detach().numpy() if sigmoid else None, skip, dtype=F64)
    mm, n = r["m"][0], r["n"][0]
    assert scale_err(r["g_x"], x.grad.numpy()) <= 1e-12
    assert scale_err(np.einsum("boc,bc->oc", mm, s), m.modulated_conv.weight.grad.numpy()) <= 1e-12
    assert scale_err(n.sum(0), m.bias.grad.numpy()) <= 1e-12
    g_s = np.einsum("boc,oc->bc", mm, w)
    assert scale_err(g_s.T @ style.detach().numpy(), m.modulated_conv.modulation.weight.grad.numpy()) <= 1e-12
    assert scale_err(g_s.sum(0), m.modulated_conv.modulation.bias.grad.numpy()) <= 1e-12
    assert scale_err(g_s @ m.modulated_conv.modulation.weight.detach().numpy(), style.grad.numpy()) <= 1e-12
    if skip is not None:
        assert scale_err(r["g_skip"], sk.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("up", [True, False])
def test_demodulated_conv_backward(up):
    """refiner_ref.ModulatedConv2d (per-sample weights, grouped conv) under float64 autograd against the
    chain the HIP path runs: upmod -> plain conv -> output scale d, with coeffs' backward behind it."""
    rng = _rng(5, up)
    B, ci, co, S, h, w = 2, 5, 7, 6, 4, 6
    m = refiner_ref.ModulatedConv2d(ci, co, 3, S, True, up).double()
    x, style = _t(rng.normal(size=(B, ci, h, w))), _t(rng.normal(size=(B, S)))
    y = m(x, style)
    G = rng.normal(size=tuple(y.shape))
    (y * torch.from_numpy(G)).sum().backward()
    W = m.weight.detach().numpy()[0]
    mw, xs, st = m.modulation.weight.detach().numpy(), x.detach().numpy(), style.detach().numpy()
    s = st @ mw.T + m.modulation.bias.detach().numpy()
    w2 = (W ** 2).sum((-1, -2))
    d = 1.0 / np.sqrt((s * s) @ w2.T + m.eps)
    xm = s[:, :, None, None] * (rb._up2(xs, F64) if up else xs)
    xm_t, W_t = _t(xm), _t(W)
    conv = F.conv2d(xm_t, W_t, padding=1)
    # the output scale: g_d = sum g_y * conv, g_conv = d * g_y
    g_d = (G * conv.detach().numpy()).sum((2, 3))
    conv.backward(torch.from_numpy(d[:, :, None, None] * G))
    g_x, (g_s, _) = rb.upmod_bwd(xm_t.grad.numpy(), xs, s, up, dtype=F64)
    layers = [(0, ci, 0, co, 0, m.eps)]
    g_s, g_w2 = rb.coeffs_bwd(g_s, g_d, s, d, w2.reshape(-1), layers, dtype=F64)
    g_W = W_t.grad.numpy() + 2.0 * W * g_w2.reshape(co, ci)[:, :, None, None]
    assert scale_err(g_x, x.grad.numpy()) <= 1e-12
    assert scale_err(g_W, m.weight.grad.numpy()) <= 1e-12
    assert scale_err(g_s.T @ st, m.modulation.weight.grad.numpy()) <= 1e-12
    assert scale_err(g_s.sum(0), m.modulation.bias.grad.numpy()) <= 1e-12
    assert scale_err(g_s @ mw, style.grad.numpy()) <= 1e-12


def test_coeffs_backward_leaves_plain_layers_alone():
    rng = _rng(6)
    B = 2
    layers = [(0, 3, -1, 2, 0, 1e-8), (3, 4, 0, 2, 0, 1e-8)]
    g_s, s = rng.normal(size=(B, 7)).astype(np.float32), rng.normal(size=(B, 7)).astype(np.float32)
    g_d, d = rng.normal(size=(B, 2)).astype(np.float32), np.abs(rng.normal(size=(B, 2))).astype(np.float32)
    w2 = np.abs(rng.normal(size=(8,))).astype(np.float32)
    out, g_w2 = rb.coeffs_bwd(g_s, g_d, s, d, w2, layers)
    assert out.dtype == np.float32 and g_w2.dtype == np.float32
    assert np.array_equal(out[:, :3], g_s[:, :3]) and not np.array_equal(out[:, 3:], g_s[:, 3:])


# ------------------------------------------------------------------ the golden

def test_grad_golden_is_small_and_complete():
    assert os.path.getsize(GRAD_GOLDEN) < 400 * 1024
    for v in ("full", "small"):
        sd, _, cond, _, out = load_variant(v)
        G, g_sd, g_style, g_cond = load_grad_golden(v)
        assert G.shape == out.shape and G.dtype == F64
        assert set(g_sd) == set(sd) and len(g_cond) == len(cond) == 4
        assert all(g_sd[k].dtype == F64 and g_sd[k].shape == sd[k].shape and np.abs(g_sd[k]).max() > 0 for k in sd)
        assert g_style.shape == (2, CFG["num_style_feat"]) and all(g.shape == c.shape for g, c in zip(g_cond, cond))


@pytest.mark.parametrize("v", ["full", "small"])
def test_torch_restatement_gradients_float64(v):
    sd, style, cond, noise, _ = load_variant(v)
    G, g_sd, g_style, g_cond = load_grad_golden(v)
    dec = refiner_ref.load_reference_state(refiner_ref.StyleDecoderRef(small=v == "small", **CFG), sd).double().eval()
    st, cs = _t(style), [_t(c) for c in cond]
    y = dec(st, cs, [torch.from_numpy(n).double() for n in noise])
    (y * torch.from_numpy(G)).sum().backward()
    worst = max([scale_err(p.grad.numpy(), g_sd[k]) for k, p in dec.named_parameters()]
                + [scale_err(st.grad.numpy(), g_style)] + [scale_err(c.grad.numpy(), g) for c, g in zip(cs, g_cond)])
    print(f"  {v}: torch restatement's float64 gradients vs the reference's: worst tensor {worst:.3g} of scale")
    assert worst <= 1e-12
