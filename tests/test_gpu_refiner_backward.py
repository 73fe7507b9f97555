"""GPU tests of the refiner decoder's backward (include/gsr_refiner.h second half, csrc/refiner_bwd.hip,
guava_renderer_amd/refiner.py: style_*_backward, style_*_grad, StyleDecoder / StyleUNetRunner grad=True).

Per kernel: every elementwise or stated-order output on the bits against tests/refiner_bwd_cases.py;
every sum over the pixels of a plane against the float64 sum of the same float32 terms within the
header's bound (D + k) * 2^-24 * sum|term|, D the depth of the kernel's fixed summation tree (the
measured fraction of the bound is printed).  The whole decoder and the runner: forward bit-equal to the
no-grad call, gradients against the reference project's float64 gradients
(tests/golden/refiner_decoder_grad.npz) and the float64 StyleUNetRef, at refiner_cases.BAR of each
tensor's largest |gradient|; where tests/refiner_ref.py's float32 torch chain on the same GPU is itself
over the bar for a tensor, that tensor's bar is twice the chain's error.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

import refiner_bwd_cases as rb
import refiner_cases as rc
import refiner_ref
from refiner_bwd_cases import U, depth_plane, depth_strided, load_grad_golden, scale_err
from refiner_cases import BAR, CFG, load_variant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _opt(a):
    return None if a is None else _d(a)


def _bits_equal(got, want):
    got = got.cpu().numpy()
    want = np.ascontiguousarray(want, np.float32)
    return got.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _normal(rng, shape, scale=1.0):
    return (rng.normal(size=shape) * scale).astype(np.float32)


def _within(name, got, ref, bound):
    """|got - ref| <= bound elementwise (bound: the header's, from the written expression); prints the
    largest fraction of the bound that was used."""
    got, ref, bound = np.asarray(got.cpu().numpy(), np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print(f"  {name}: {frac:.3g} of the bound")
    assert (err <= bound).all(), (name, frac)
    return frac


@contextlib.contextmanager
def _deterministic_convs():
    """torch's own conv backward is not ours: keep its algorithm choice deterministic where two runs are
    compared on the bits."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = old


# ------------------------------------------------------------------ epilogue

@pytest.mark.parametrize("has_d", [True, False])
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("sft", [False, True])
@pytest.mark.parametrize("noise_batch", [0, 1, "B"])
@pytest.mark.parametrize("shape", [(3, 5, 4, 4), (2, 3, 40, 56)])  # 4 quads a plane; 560 quads: three chunks
def test_epilogue_backward(shape, noise_batch, sft, post, has_d):
    from guava_renderer_amd import refiner
    B, C, H, W = shape
    nb = B if noise_batch == "B" else noise_batch
    rng = _rng(1, B, H, nb, sft, post, has_d)
    x, g_y, bias = _normal(rng, shape, 2.0), _normal(rng, shape), _normal(rng, (C,))
    d = np.abs(_normal(rng, (B, C))) + np.float32(0.1) if has_d else None
    noise, nw = (_normal(rng, (nb, 1, H, W)), np.float32(0.7)) if nb else (None, None)
    scale, shift = (_normal(rng, shape), _normal(rng, shape)) if sft else (None, None)
    ps = _normal(rng, (B, C)) if post else None
    want = rb.epilogue_bwd(g_y, x, d, bias, noise, nw, scale, shift, ps)
    assert (want["l"] < 0).any() and (want["l"] > 0).any()  # both LeakyReLU branches
    g = refiner.style_epilogue_backward(_d(g_y), _d(x), _opt(d), _d(bias).reshape(1, C, 1, 1), _opt(noise),
                                        _d(np.array([nw])) if nb else None, _opt(scale), _opt(shift), _opt(ps))
    assert _bits_equal(g["x"], want["g_x"])
    if sft:
        assert _bits_equal(g["scale"], want["g_scale"]) and _bits_equal(g["shift"], want["g_shift"])
    else:
        assert g["scale"] is None and g["shift"] is None
    D = depth_plane(H, W)
    assert rb.chunks(H, W) == (1 if H == 4 else 3)
    if has_d:
        r2 = float(rc.SQRT2)
        _within("g_d", g["d"], r2 * want["S_x"][0], (D + 2) * U * r2 * want["S_x"][1])
    else:
        assert g["d"] is None
    if post:
        _within("g_post", g["post"], want["S_p"][0], (D + 1) * U * want["S_p"][1])
    _within("g_bias", g["bias"], want["S_v"][0].sum(0), (D + B) * U * want["S_v"][1].sum(0))
    if nb:
        ref = want["S_n"][0].sum().reshape(1)  # formed and added in float64 by the kernel, rounded once
        _within("g_noise_weight", g["noise_weight"], ref,
                U * np.abs(ref) + (D + depth_strided(B * C) + 1) * 2.0 ** -53 * want["S_n"][1].sum().reshape(1))
    else:
        assert g["noise_weight"] is None


# ------------------------------------------------------------------ upmod

@pytest.mark.parametrize("B,C,h,w,up,xb", [
    (2, 3, 2, 2, True, 2),     # 4x4: one lane-quad per row, every tap folded
    (2, 3, 4, 4, True, 2),     # 8x8
    (2, 3, 4, 12, True, 2),    # 8x24: H != W
    (2, 5, 20, 36, True, 2),   # 40x72: 720 quads a plane, three chunks
    (3, 3, 4, 4, False, 1),    # the constant input: x of batch 1, its gradient summed over the frames
    (3, 3, 4, 8, False, 3),    # the plain scale
])
def test_upmod_backward(B, C, h, w, up, xb):
    from guava_renderer_amd import refiner
    rng = _rng(2, B, C, h, w, up, xb)
    H, W = (2 * h, 2 * w) if up else (h, w)
    x, table, g_y = _normal(rng, (xb, C, h, w)), _normal(rng, (B, C + 8)), _normal(rng, (B, C, H, W))
    s = table[:, 5:5 + C]  # a column range of a wider table, as the decoder passes it
    want_x, (want_s, mag) = rb.upmod_bwd(g_y, x, s, up)
    g_x, g_s = refiner.style_upmod_backward(_d(g_y), _d(x), _d(table)[:, 5:5 + C], up=up)
    assert _bits_equal(g_x, want_x)
    _within("g_s", g_s, want_s, (depth_plane(H, W) + 1) * U * mag)


# ------------------------------------------------------------------ torgb

@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("skip", [None, "same", "up"])
@pytest.mark.parametrize("H,W", [(4, 4), (8, 24), (40, 56)])
@pytest.mark.parametrize("C", [1, 7, 40])
@pytest.mark.parametrize("O", [1, 3, 4])
def test_torgb_backward(O, C, H, W, skip, sigmoid):
    from guava_renderer_amd import refiner
    B = 2
    rng = _rng(3, O, C, H, W, skip is None, skip == "up", sigmoid)
    x, w, table, bias = _normal(rng, (B, C, H, W)), _normal(rng, (O, C), 0.5), _normal(rng, (B, C + 3)), _normal(rng, (O,))
    s = table[:, 2:2 + C]
    sk = None if skip is None else _normal(rng, (B, O, H // 2, W // 2) if skip == "up" else (B, O, H, W))
    g_out = _normal(rng, (B, O, H, W))
    y = rc.torgb(x, w, s, bias, sk, skip_up=skip == "up", sigmoid=True) if sigmoid else None
    want = rb.torgb_bwd(g_out, x, w, s, y, skip)
    g_x, g_w, g_s, g_b, g_skip = refiner.style_torgb_backward(_d(g_out), _d(x), _d(w), _d(table)[:, 2:2 + C], y=_opt(y),
                                                              skip=skip)
    assert _bits_equal(g_x, want["g_x"])
    if skip is None:
        assert g_skip is None
    else:
        assert _bits_equal(g_skip, want["g_skip"])
    D = depth_plane(H, W)
    (m, m_mag), (n, n_mag) = want["m"], want["n"]
    s64, w64 = s.astype(np.float64), w.astype(np.float64)
    _within("g_bias", g_b, n.sum(0), (D + B) * U * n_mag.sum(0))
    _within("g_weight", g_w, np.einsum("boc,bc->oc", m, s64), (D + B + 1) * U * np.einsum("boc,bc->oc", m_mag, np.abs(s64)))
    _within("g_s", g_s, np.einsum("boc,oc->bc", m, w64), (D + O + 1) * U * np.einsum("boc,oc->bc", m_mag, np.abs(w64)))


# ------------------------------------------------------------------ coeffs

def _coeff_table(rng, B, S, eps=1e-8):
    # (c_in, c_out or 0 for a plain ToRGB-like layer): 70 > one wave's lanes, 20 > one workgroup's waves
    shapes = [(1, 3), (7, 0), (70, 20), (7, 3), (70, 0)]
    layers, w2, s_off, d_off = [], [], 0, 0
    for c_in, c_out in shapes:
        layers.append((s_off, c_in, d_off if c_out else -1, c_out or 3, sum(t.size for t in w2), eps))
        if c_out:
            w2.append(np.abs(_normal(rng, (c_out, c_in))) + np.float32(0.01))
            d_off += c_out
        s_off += c_in
    return layers, np.concatenate([t.reshape(-1) for t in w2]), s_off, d_off


@pytest.mark.parametrize("S", [5, 130])
def test_coeffs_backward(S):
    from guava_renderer_amd import refiner
    B = 3
    rng = _rng(4, S)
    layers, w2, sum_in, sum_out = _coeff_table(rng, B, S)
    latent, mw, mb = _normal(rng, (B, S)), _normal(rng, (sum_in, S), 0.3), _normal(rng, (sum_in,)) + np.float32(1.0)
    G_s, G_d = _normal(rng, (B, sum_in)), _normal(rng, (B, sum_out))
    # the kernel alone, on the s and d the forward kernel stored: stated order, so on the bits
    with torch.no_grad():
        s, d = refiner.style_coeffs(_d(latent), _d(mw), _d(mb), _d(w2), layers, sum_out)
    want_s, want_w2 = rb.coeffs_bwd(G_s, G_d, s.cpu().numpy(), d.cpu().numpy(), w2, layers)
    g_in = _d(G_s)
    g_s, g_w2 = refiner.style_coeffs_backward(g_in, _d(G_d), s, d, _d(w2), layers)
    assert _bits_equal(g_s, want_s) and _bits_equal(g_w2, want_w2)
    assert _bits_equal(g_in, G_s)  # the caller's g_s is not modified
    plain = np.concatenate([np.arange(so, so + ci) for so, ci, do, _, _, _ in layers if do < 0])
    assert np.array_equal(g_s.cpu().numpy()[:, plain], G_s[:, plain])  # a plain layer's g_s passes through
    # under autograd, with the three dense products: against float64 autograd of the same formulas
    t = [_d(a).requires_grad_(True) for a in (latent, mw, mb, w2)]
    s, d = refiner.style_coeffs_grad(*t, layers, sum_out)
    ((s * _d(G_s)).sum() + (d * _d(G_d)).sum()).backward()
    t64 = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (latent, mw, mb, w2)]
    s64 = t64[0] @ t64[1].T + t64[2]
    loss = (s64 * torch.from_numpy(G_s.astype(np.float64))).sum()
    for so, ci, do, co, wo, eps in layers:
        if do >= 0:
            d64 = torch.rsqrt((s64[:, so:so + ci] ** 2) @ t64[3][wo:wo + co * ci].reshape(co, ci).T + float(np.float32(eps)))
            loss = loss + (d64 * torch.from_numpy(G_d[:, do:do + co].astype(np.float64))).sum()
    loss.backward()
    for name, a, b in zip(("latent", "mod_weight", "mod_bias", "w2"), t, t64):
        err = scale_err(a.grad.cpu().numpy(), b.grad.numpy())
        print(f"  style_coeffs_grad {name}: {err:.3g} of scale")
        assert err <= BAR


# ------------------------------------------------------------------ argument errors

def test_backward_rejects_bad_arguments():
    """Width 6, a misaligned pointer and mismatched shapes: RuntimeError (GSR_ERR_ARG, nothing launched)."""
    from guava_renderer_amd import refiner
    z = lambda *shape: torch.zeros(shape, device=DEV)  # noqa: E731

    def off4(*shape):  # contiguous, 4 bytes off a 16-byte boundary
        n = int(np.prod(shape))
        return torch.zeros(n + 1, device=DEV)[1:].view(shape)

    with pytest.raises(RuntimeError, match="multiple of 4"):
        refiner.style_epilogue_backward(z(2, 3, 4, 6), z(2, 3, 4, 6), z(2, 3), z(3))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        refiner.style_upmod_backward(z(2, 3, 6, 6), z(2, 3, 3, 3), z(2, 3), up=True)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        refiner.style_torgb_backward(z(2, 3, 4, 6), z(2, 5, 4, 6), z(3, 5), z(2, 5))
    with pytest.raises(RuntimeError, match="misaligned"):
        refiner.style_epilogue_backward(off4(2, 3, 4, 4), z(2, 3, 4, 4), z(2, 3), z(3))
    with pytest.raises(RuntimeError, match="misaligned"):
        refiner.style_upmod_backward(off4(2, 3, 8, 8), z(2, 3, 4, 4), z(2, 3), up=True)
    with pytest.raises(RuntimeError, match="misaligned"):
        refiner.style_torgb_backward(z(2, 3, 4, 4), off4(2, 5, 4, 4), z(3, 5), z(2, 5))
    with pytest.raises(RuntimeError):
        refiner.style_epilogue_backward(z(2, 3, 4, 8), z(2, 3, 4, 4), z(2, 3), z(3))      # g_y is not x's shape
    with pytest.raises(RuntimeError):
        refiner.style_upmod_backward(z(2, 3, 8, 8), z(2, 3, 4, 8), z(2, 3), up=True)       # x is not half of g_y
    with pytest.raises(RuntimeError):
        refiner.style_upmod_backward(z(2, 3, 8, 8), z(1, 3, 4, 4), z(2, 3), up=True)       # a broadcast x with up
    with pytest.raises(RuntimeError):
        refiner.style_torgb_backward(z(2, 3, 4, 4), z(2, 5, 4, 4), z(4, 5), z(2, 5))       # g_out has 3 planes, weight 4
    with pytest.raises(RuntimeError):
        refiner.style_coeffs_backward(z(2, 7), z(2, 3), z(2, 7), z(2, 3), z(10), [(0, 7, 0, 3, 0, 1e-8)])  # w2 too short
    with pytest.raises(RuntimeError, match="GPU only"):
        refiner.style_upmod_backward(torch.zeros(2, 3, 8, 8), z(2, 3, 4, 4), z(2, 3))


# ------------------------------------------------------------------ the whole decoder

def _tensor_bars(rows):
    """rows: (name, ours, torch chain, float64).  Prints both errors per tensor; -> the tensors over their bar."""
    bad = []
    for name, ours, chain, ref in rows:
        e_o, e_t = scale_err(ours, ref), scale_err(chain, ref)
        bar = BAR if e_t <= BAR else 2.0 * e_t
        print(f"  {name:58s} ours {e_o:.3g}  torch chain {e_t:.3g}  bar {bar:.3g}")
        if not e_o <= bar:
            bad.append((name, e_o, bar))
    return bad


@pytest.mark.parametrize("v", ["full", "small"])
def test_decoder_gradients_against_reference_float64(v):
    from guava_renderer_amd.refiner import StyleDecoder
    sd, style, cond, noise, _ = load_variant(v)
    G, g_sd, g_style, g_cond = load_grad_golden(v)
    dec = StyleDecoder.from_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, CFG["out_size"], v == "small",
                                       device=DEV)
    names = sorted(g_sd)
    params = [dec._get(k).requires_grad_(True) for k in names]
    st, cs, ns = _d(style).requires_grad_(True), [_d(c).requires_grad_(True) for c in cond], [_d(n) for n in noise]
    Gd = _d(G.astype(np.float32))
    leaves = params + [st] + cs
    with torch.no_grad():
        plain = dec.forward(st, cs, ns)
        assert torch.equal(dec.forward(st, cs, ns, grad=True), plain)  # grad disabled: just the forward

    def run():
        y = dec.forward(st, cs, ns, grad=True)
        assert torch.equal(y.detach(), plain)  # bit-equal to the no-grad forward
        return torch.autograd.grad((y * Gd).sum(), leaves)

    with _deterministic_convs():
        first = run()
        second = run()
    for name, a, b in zip(names + ["style"] + [f"cond/{i}" for i in range(len(cs))], first, second):
        assert torch.equal(a, b), f"{name}: a second backward gives other bits"
    ref32 = refiner_ref.load_reference_state(refiner_ref.StyleDecoderRef(small=v == "small", **CFG), sd).to(DEV).eval()
    rp = dict(ref32.named_parameters())
    st2, cs2 = _d(style).requires_grad_(True), [_d(c).requires_grad_(True) for c in cond]
    chain = torch.autograd.grad((ref32(st2, cs2, ns) * Gd).sum(), [rp[k] for k in names] + [st2] + cs2)
    rows = [(k, a, b, g_sd[k]) for k, a, b in zip(names, first, chain)]
    rows.append(("style", first[len(names)], chain[len(names)], g_style))
    rows += [(f"cond/{i}", first[len(names) + 1 + i], chain[len(names) + 1 + i], g) for i, g in enumerate(g_cond)]
    bad = _tensor_bars([(n, a.cpu().numpy(), b.cpu().numpy(), r) for n, a, b, r in rows])
    assert not bad, bad
    with pytest.raises(NotImplementedError):  # the default call stays forward only
        dec.forward(st, cs, ns)


# ------------------------------------------------------------------ StyleUNetRunner

@pytest.mark.parametrize("small", [True, False])
def test_runner_gradients(small):
    from guava_renderer_amd.refiner import StyleUNetRunner
    torch.manual_seed(23)
    net = refiner_ref.StyleUNetRef(in_size=16, out_size=16, in_dim=32, out_dim=3, num_style_feat=64, num_mlp=2,
                                   activation=True, channel_scale=32, small=small).eval()
    refiner_ref.randomize_noise_params(net, 10)
    g = torch.Generator().manual_seed(24)
    x = torch.rand((2, 32, 16, 16), generator=g)
    noise = [torch.randn((2, 1, n, n), generator=g) for n in net.stylegan_decoder.noise_sizes()]
    G = torch.randn((2, 3, 16, 16), generator=g)
    picked = ["stylegan_decoder.style_convs.0.modulated_conv.weight", "condition_scale.0.0.weight"]
    with torch.no_grad():
        feat = torch.nn.functional.leaky_relu(net.conv_body_first(x), 0.2)
    net64 = copy.deepcopy(net).double()
    f64 = feat.double().requires_grad_(True)
    p64 = dict(net64.named_parameters())
    want = torch.autograd.grad((net64.rest(f64, [n.double() for n in noise]) * G.double()).sum(),
                               [f64] + [p64[k] for k in picked])
    net = net.to(DEV)
    run = StyleUNetRunner(net)
    p32 = dict(net.named_parameters())
    fg, ng, Gg = feat.to(DEV).requires_grad_(True), [n.to(DEV) for n in noise], G.to(DEV)
    leaves = [fg] + [p32[k] for k in picked]
    with torch.no_grad():
        plain = run.rest(fg, noise=ng)
        assert torch.equal(run.forward(x.to(DEV), noise=ng, grad=True), run.forward(x.to(DEV), noise=ng))
    y = run.rest(fg, noise=ng, grad=True)
    assert torch.equal(y.detach(), plain)
    ours = torch.autograd.grad((y * Gg).sum(), leaves)
    chain = torch.autograd.grad((net.rest(fg, ng) * Gg).sum(), leaves)
    bad = _tensor_bars([(n, a.cpu().numpy(), b.cpu().numpy(), r.numpy())
                        for n, a, b, r in zip(["feat"] + picked, ours, chain, want)])
    assert not bad, bad
    # every parameter of the module is reached
    y = run.forward(x.to(DEV).requires_grad_(True), noise=ng, grad=True)
    grads = torch.autograd.grad(y.sum(), list(net.parameters()), allow_unused=True)
    missing = [k for (k, _), gr in zip(net.named_parameters(), grads) if gr is None]
    assert not missing, missing
