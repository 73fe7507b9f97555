"""The StyleUNet refiner's decoder on gfx950 (csrc/refiner.hip through include/gsr_refiner.h): the
StyleGAN2 decoder of the reference (models/modules/net_module/styleunet/styleunet.py:211-407) with its
modulated convs written as plain convs -- scale the input by s[b,c_in], convolve with the shared weight,
scale the output by d[b,c_out] -- so that F.conv2d runs an ordinary batched conv and everything around
it is one HIP pass in front (upsample + input modulation) and one behind (demodulation, noise, bias,
LeakyReLU, SFT), plus one launch for every layer's s and d and one fused ToRGB per level.

  StyleDecoder.from_module(dec) / .from_state_dict(sd, out_size, small)
      .forward(style_code [B,S], conditions, noise=None, generator=None, sigmoid=False, grad=False)
                                                                                   -> [B,out_dim,H,W]
  StyleUNetRunner(styleunet)
      .forward(x32, ...)    the whole refiner on the 32-channel render
      .rest(feat16, ...)    from RefineHead.out / render_refined's `refined` (conv_body_first + LeakyReLU)

Float32, on the caller's current stream.  Semantics: include/gsr_refiner.h.  GPU only:
CPU tensors raise RuntimeError; there is no CPU fallback.

The default calls are forward only: with grad enabled and an input or parameter that requires it they
raise NotImplementedError.  Training is opt-in: grad=True runs the same forward kernels (bit-equal
values, the epilogue out of place) under torch.autograd, with the backward of the four kernels in HIP
(csrc/refiner_bwd.hip: style_upmod_grad, style_epilogue_grad, style_torgb_grad, style_coeffs_grad) and
the convolutions, the style MLP, normal_convs and the UNet half under ordinary autograd.  Noise tensors
get no gradient; there is no double backward.
"""
import ctypes
import math

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _gpu(t, what, dims=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"the refiner decoder runs on the GPU only ({what} is not a GPU tensor)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32, got {t.dtype}")
    if dims is not None and t.dim() != dims:
        raise RuntimeError(f"{what} must have {dims} dimensions, got {tuple(t.shape)}")
    return t


def _rows(t, what, B, C):
    """A [B,C] coefficient table, possibly a column range of a wider one -> (tensor, row stride)."""
    _gpu(t, what, 2)
    if tuple(t.shape) != (B, C) or t.stride(1) != 1:
        raise RuntimeError(f"{what} must be ({B}, {C}) with unit column stride, got {tuple(t.shape)}")
    return t, (t.stride(0) if B > 1 else max(t.stride(0), C))  # (a single row's stride is arbitrary in torch)


# ------------------------------------------------------------------ the four kernels

def style_coeffs(latent, mod_weight, mod_bias, w2, layers, sum_out):
    """gsr_style_coeffs.  layers: (s_off, c_in, d_off or -1, c_out, w2_off, eps) per modulated conv.
    -> (s [B, sum_in], d [B, sum_out] or None)."""
    latent = _gpu(latent, "latent", 2).contiguous()
    mod_weight, mod_bias = _gpu(mod_weight, "mod_weight", 2).contiguous(), _gpu(mod_bias, "mod_bias", 1).contiguous()
    B, S = latent.shape
    sum_in = int(mod_weight.shape[0])
    if mod_weight.shape[1] != S or mod_bias.shape[0] != sum_in:
        raise RuntimeError(f"mod_weight must be (sum_in, {S}) and mod_bias (sum_in,), got {tuple(mod_weight.shape)} "
                           f"and {tuple(mod_bias.shape)}")
    if w2 is not None:
        w2 = _gpu(w2, "w2", 1).contiguous()
    table = (_lib.StyleLayer * len(layers))(*[_lib.StyleLayer(int(a), int(b), int(c), int(d), int(e), float(f))
                                              for a, b, c, d, e, f in layers])
    dev = latent.device
    s = torch.empty((B, sum_in), dtype=torch.float32, device=dev)
    d = torch.empty((B, sum_out), dtype=torch.float32, device=dev) if sum_out else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsr_style_coeffs(B, S, len(layers), table, sum_in, int(sum_out),
                                                0 if w2 is None else w2.numel(), _p(latent), _p(mod_weight),
                                                _p(mod_bias), _p(w2), _p(s), _p(d), _stream(dev)), "gsr_style_coeffs")
    return s, d


def style_upmod(x, s, up=True):
    """gsr_style_upmod: s[b,c] * up2(x[b,c]) (up) or s[b,c] * x[b,c].  x [1 or B,C,h,w]; s [B,C]."""
    x = _gpu(x, "x", 4).contiguous()
    xb, C, h, w = x.shape
    B = int(s.shape[0]) if torch.is_tensor(s) and s.dim() == 2 else -1
    s, ss = _rows(s, "s", B, C)
    if xb not in (1, B):
        raise RuntimeError(f"x must have batch 1 or {B}, got {xb}")
    H, W = (2 * h, 2 * w) if up else (h, w)
    y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().gsr_style_upmod(B, C, H, W, 1 if up else 0, xb, _p(x), _p(s), ss, _p(y), _stream(x.device)),
                   "gsr_style_upmod")
    return y


def style_epilogue(x, d, bias, noise=None, noise_weight=None, scale=None, shift=None, post=None, out=None):
    """gsr_style_epilogue on x [B,C,H,W]: lrelu(sqrt(2)*d*x + nw*noise + bias), then *scale + shift, then
    *post.  d, post [B,C] or None; bias C values; noise [1 or B,1,H,W] or None, noise_weight one device
    float; out: None (a new tensor) or x itself (in place)."""
    x = _gpu(x, "x", 4)
    if not x.is_contiguous():
        raise RuntimeError("x must be contiguous")
    B, C, H, W = x.shape
    d, ds = _rows(d, "d", B, C) if d is not None else (None, 0)
    post, ps = _rows(post, "post", B, C) if post is not None else (None, 0)
    bias = _gpu(bias, "bias").reshape(-1).contiguous()
    if bias.numel() != C:
        raise RuntimeError(f"bias must hold {C} values, got {tuple(bias.shape)}")
    nb = 0
    if noise is not None:
        noise = _gpu(noise, "noise", 4).contiguous()
        nb = int(noise.shape[0])
        if tuple(noise.shape[1:]) != (1, H, W) or nb not in (1, B):
            raise RuntimeError(f"noise must be (1 or {B}, 1, {H}, {W}), got {tuple(noise.shape)}")
        noise_weight = _gpu(noise_weight, "noise_weight").reshape(-1)
    if (scale is None) != (shift is None):
        raise RuntimeError("scale and shift come together")
    if scale is not None:
        scale, shift = _gpu(scale, "scale", 4).contiguous(), _gpu(shift, "shift", 4).contiguous()
        if tuple(scale.shape) != tuple(x.shape) or tuple(shift.shape) != tuple(x.shape):
            raise RuntimeError(f"scale and shift must be {tuple(x.shape)}, got {tuple(scale.shape)} and "
                               f"{tuple(shift.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif out.data_ptr() != x.data_ptr() or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
        raise RuntimeError("out must be None or x itself")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().gsr_style_epilogue(B, C, H, W, _p(x), _p(d), ds, _p(noise), nb, _p(noise_weight) if nb else None,
                                                  _p(bias), _p(scale), _p(shift), _p(post), ps, _p(out),
                                                  _stream(x.device)), "gsr_style_epilogue")
    return out


def style_torgb(x, weight, s, bias, skip=None, skip_up=False, sigmoid=False):
    """gsr_style_torgb: out[b,o] = sum_c (weight[o,c]*s[b,c]) * x[b,c] + bias[o] (+ skip or up2(skip))
    (sigmoid).  x [B,C,H,W]; weight [O,C]; s [B,C]; bias O values; skip [B,O,H,W] or [B,O,H/2,W/2]."""
    x = _gpu(x, "x", 4).contiguous()
    B, C, H, W = x.shape
    weight = _gpu(weight, "weight", 2).contiguous()
    O = int(weight.shape[0])
    if weight.shape[1] != C:
        raise RuntimeError(f"weight must be (out_dim, {C}), got {tuple(weight.shape)}")
    s, ss = _rows(s, "s", B, C)
    bias = _gpu(bias, "bias").reshape(-1).contiguous()
    if bias.numel() != O:
        raise RuntimeError(f"bias must hold {O} values, got {tuple(bias.shape)}")
    if skip is not None:
        skip = _gpu(skip, "skip", 4).contiguous()
        want = (B, O, H // 2, W // 2) if skip_up else (B, O, H, W)
        if tuple(skip.shape) != want or (skip_up and (H % 2 or W % 2)):
            raise RuntimeError(f"skip must be {want}, got {tuple(skip.shape)}")
    out = torch.empty((B, O, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().gsr_style_torgb(B, C, O, H, W, _p(x), _p(weight), _p(s), ss, _p(bias), _p(skip),
                                               1 if skip_up else 0, 1 if sigmoid else 0, _p(out), _stream(x.device)),
                   "gsr_style_torgb")
    return out


# ------------------------------------------------------------------ their backward (csrc/refiner_bwd.hip)

def _chunks(H, W):
    n = int(_lib.load().gsr_style_backward_chunks(int(H), int(W)))
    return max(n, 1)  # (a refused shape: the entry itself reports it, with nothing launched)


def _layer_table(layers):
    return (_lib.StyleLayer * len(layers))(*[_lib.StyleLayer(int(a), int(b), int(c), int(d), int(e), float(f))
                                             for a, b, c, d, e, f in layers])


def _f32(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def style_upmod_backward(g_y, x, s, up=True):
    """gsr_style_upmod_backward -> (g_x shaped as x, g_s [B,C])."""
    g_y, x = _gpu(g_y, "g_y", 4), _gpu(x, "x", 4).contiguous()
    if not g_y.is_contiguous():
        raise RuntimeError("g_y must be contiguous")
    B, C, H, W = g_y.shape
    s, ss = _rows(s, "s", B, C)
    xb = int(x.shape[0])
    want = (xb, C, H // 2, W // 2) if up else (xb, C, H, W)
    if xb not in (1, B) or tuple(x.shape) != want or (up and (H % 2 or W % 2)):
        raise RuntimeError(f"x must be (1 or {B}, {C}, {want[2]}, {want[3]}), got {tuple(x.shape)}")
    dev = g_y.device
    g_x, g_s = torch.empty_like(x), _f32((B, C), dev)
    ws = _f32((B * C * _chunks(H, W),), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsr_style_upmod_backward(B, C, H, W, 1 if up else 0, xb, _p(g_y), _p(x), _p(s), ss, _p(g_x),
                                                        _p(g_s), _p(ws), _stream(dev)), "gsr_style_upmod_backward")
    return g_x, g_s


def style_epilogue_backward(g_y, x, d, bias, noise=None, noise_weight=None, scale=None, shift=None, post=None):
    """gsr_style_epilogue_backward on the forward's operands (x: what the forward read)
    -> dict(x, d, bias [C], noise_weight [1], scale, shift, post), None where the operand is absent."""
    g_y, x = _gpu(g_y, "g_y", 4), _gpu(x, "x", 4)
    if not x.is_contiguous() or not g_y.is_contiguous():
        raise RuntimeError("x and g_y must be contiguous")
    if tuple(g_y.shape) != tuple(x.shape):
        raise RuntimeError(f"g_y must be {tuple(x.shape)}, got {tuple(g_y.shape)}")
    B, C, H, W = x.shape
    d, ds = _rows(d, "d", B, C) if d is not None else (None, 0)
    post, ps = _rows(post, "post", B, C) if post is not None else (None, 0)
    bias = _gpu(bias, "bias").reshape(-1).contiguous()
    if bias.numel() != C:
        raise RuntimeError(f"bias must hold {C} values, got {tuple(bias.shape)}")
    nb = 0
    if noise is not None:
        noise = _gpu(noise, "noise", 4).contiguous()
        nb = int(noise.shape[0])
        if tuple(noise.shape[1:]) != (1, H, W) or nb not in (1, B):
            raise RuntimeError(f"noise must be (1 or {B}, 1, {H}, {W}), got {tuple(noise.shape)}")
        noise_weight = _gpu(noise_weight, "noise_weight").reshape(-1)
    if (scale is None) != (shift is None):
        raise RuntimeError("scale and shift come together")
    if scale is not None:
        scale, shift = _gpu(scale, "scale", 4).contiguous(), _gpu(shift, "shift", 4).contiguous()
        if tuple(scale.shape) != tuple(x.shape) or tuple(shift.shape) != tuple(x.shape):
            raise RuntimeError(f"scale and shift must be {tuple(x.shape)}, got {tuple(scale.shape)} and "
                               f"{tuple(shift.shape)}")
    dev = x.device
    g = dict(x=torch.empty_like(x), bias=_f32((C,), dev),
             d=_f32((B, C), dev) if d is not None else None, post=_f32((B, C), dev) if post is not None else None,
             noise_weight=_f32((1,), dev) if nb else None,
             scale=torch.empty_like(x) if scale is not None else None,
             shift=torch.empty_like(x) if scale is not None else None)
    ws = _f32((6 * B * C * (_chunks(H, W) + 1),), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsr_style_epilogue_backward(
            B, C, H, W, _p(g_y), _p(x), _p(d), ds, _p(noise), nb, _p(noise_weight) if nb else None, _p(bias), _p(scale),
            _p(shift), _p(post), ps, _p(g["x"]), _p(g["scale"]), _p(g["shift"]), _p(g["d"]), _p(g["post"]), _p(g["bias"]),
            _p(g["noise_weight"]), _p(ws), _stream(dev)), "gsr_style_epilogue_backward")
    return g


def style_torgb_backward(g_out, x, weight, s, y=None, skip=None):
    """gsr_style_torgb_backward.  y: the forward's output where it applied the sigmoid, else None; skip:
    None, "same" or "up" (how the forward took its skip) -> (g_x, g_weight [O,C], g_s [B,C], g_bias [O],
    g_skip or None)."""
    g_out, x = _gpu(g_out, "g_out", 4), _gpu(x, "x", 4).contiguous()
    if not g_out.is_contiguous():
        raise RuntimeError("g_out must be contiguous")
    B, C, H, W = x.shape
    weight = _gpu(weight, "weight", 2).contiguous()
    O = int(weight.shape[0])
    if weight.shape[1] != C or tuple(g_out.shape) != (B, O, H, W):
        raise RuntimeError(f"weight must be (out_dim, {C}) and g_out ({B}, out_dim, {H}, {W}), got {tuple(weight.shape)} "
                           f"and {tuple(g_out.shape)}")
    s, ss = _rows(s, "s", B, C)
    if y is not None:
        y = _gpu(y, "y", 4).contiguous()
        if tuple(y.shape) != tuple(g_out.shape):
            raise RuntimeError(f"y must be {tuple(g_out.shape)}, got {tuple(y.shape)}")
    if skip not in (None, "same", "up") or (skip == "up" and (H % 2 or W % 2)):
        raise RuntimeError(f"skip must be None, 'same' or 'up' (even sizes), got {skip!r}")
    dev = x.device
    g_x, g_w, g_s, g_b = torch.empty_like(x), _f32((O, C), dev), _f32((B, C), dev), _f32((O,), dev)
    g_skip = None if skip is None else _f32((B, O, H // 2, W // 2) if skip == "up" else (B, O, H, W), dev)
    ws = _f32((B * _chunks(H, W) * (O * C + O),), dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsr_style_torgb_backward(B, C, O, H, W, _p(g_out), _p(y), _p(x), _p(weight), _p(s), ss,
                                                        1 if skip == "up" else 0, _p(g_x), _p(g_skip), _p(g_w), _p(g_s),
                                                        _p(g_b), _p(ws), _stream(dev)), "gsr_style_torgb_backward")
    return g_x, g_w, g_s, g_b, g_skip


def style_coeffs_backward(g_s, g_d, s, d, w2, layers):
    """gsr_style_coeffs_backward: the demodulation's share.  g_s [B,sum_in] (what reached s directly; not
    modified), g_d [B,sum_out] -> (g_s with the demodulated layers' share added, g_w2 shaped as w2)."""
    g_s, s = _gpu(g_s, "g_s", 2), _gpu(s, "s", 2).contiguous()
    B, sum_in = s.shape
    if tuple(g_s.shape) != (B, sum_in):
        raise RuntimeError(f"g_s must be {(B, sum_in)}, got {tuple(g_s.shape)}")
    g_s = g_s.clone(memory_format=torch.contiguous_format)
    if d is None:
        return g_s, None
    d, g_d, w2 = _gpu(d, "d", 2).contiguous(), _gpu(g_d, "g_d", 2).contiguous(), _gpu(w2, "w2", 1).contiguous()
    if tuple(g_d.shape) != tuple(d.shape) or d.shape[0] != B:
        raise RuntimeError(f"d and g_d must be ({B}, sum_out), got {tuple(d.shape)} and {tuple(g_d.shape)}")
    covered = sum(int(c_in) * int(c_out) for _, c_in, d_off, c_out, _, _ in layers if d_off >= 0)
    g_w2 = torch.empty_like(w2) if covered == w2.numel() else torch.zeros_like(w2)
    with torch.cuda.device(s.device):
        _lib.check(_lib.load().gsr_style_coeffs_backward(B, len(layers), _layer_table(layers), sum_in, int(d.shape[1]),
                                                         w2.numel(), _p(s), _p(d), _p(w2), _p(g_d), _p(g_s), _p(g_w2),
                                                         _stream(s.device)), "gsr_style_coeffs_backward")
    return g_s, g_w2


def _like(g, t):
    """A gradient in the shape of the operand it belongs to (None stays None)."""
    return None if g is None or t is None else g.reshape(t.shape)


class _Upmod(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s, up):
        ctx.save_for_backward(x, s)
        ctx.up = up
        return style_upmod(x, s, up=up)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y):
        x, s = ctx.saved_tensors
        g_x, g_s = style_upmod_backward(g_y.contiguous(), x, s, up=ctx.up)
        return _like(g_x, x), g_s, None


class _Epilogue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, d, bias, noise, noise_weight, scale, shift, post):
        ctx.save_for_backward(x, d, bias, noise, noise_weight, scale, shift, post)
        return style_epilogue(x, d, bias, noise, noise_weight, scale, shift, post)  # out of place: x is kept

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y):
        x, d, bias, noise, nw, scale, shift, post = ctx.saved_tensors
        g = style_epilogue_backward(g_y.contiguous(), x, d, bias, noise, nw, scale, shift, post)
        return (g["x"], g["d"], _like(g["bias"], bias), None, _like(g["noise_weight"], nw), _like(g["scale"], scale),
                _like(g["shift"], shift), g["post"])


class _ToRGB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, s, bias, skip, skip_up, sigmoid):
        out = style_torgb(x, weight, s, bias, skip, skip_up=skip_up, sigmoid=sigmoid)
        ctx.save_for_backward(x, weight, s, bias, out if sigmoid else None)
        ctx.skip = None if skip is None else ("up" if skip_up else "same")
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        x, weight, s, bias, y = ctx.saved_tensors
        g_x, g_w, g_s, g_b, g_skip = style_torgb_backward(g_out.contiguous(), x, weight, s, y=y, skip=ctx.skip)
        return _like(g_x, x), _like(g_w, weight), g_s, _like(g_b, bias), g_skip, None, None


class _Coeffs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latent, mod_weight, mod_bias, w2, layers, sum_out):
        s, d = style_coeffs(latent, mod_weight, mod_bias, w2, layers, sum_out)
        if d is None:  # no demodulated layer: an empty table stands in, without a gradient
            d = latent.new_empty((latent.shape[0], 0))
            ctx.mark_non_differentiable(d)
        ctx.save_for_backward(latent, mod_weight, w2, s, d)
        ctx.layers = layers
        return s, d

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, g_d):
        latent, mod_weight, w2, s, d = ctx.saved_tensors
        g_s, g_w2 = style_coeffs_backward(g_s, g_d, s, d if d.shape[1] else None, w2, ctx.layers)
        # the three dense products are rocBLAS GEMMs on the stacked tables: plumbing, and already one
        # launch each for every layer at once
        return torch.mm(g_s, mod_weight), torch.mm(g_s.t(), latent), g_s.sum(0), g_w2, None, None


def style_upmod_grad(x, s, up=True):
    """style_upmod under torch.autograd: gradients for x and s."""
    return _Upmod.apply(_gpu(x, "x", 4), s, bool(up))


def style_epilogue_grad(x, d, bias, noise=None, noise_weight=None, scale=None, shift=None, post=None):
    """style_epilogue (out of place) under torch.autograd: gradients for x, d, bias, noise_weight, scale,
    shift and post; none for the noise."""
    return _Epilogue.apply(x, d, bias, noise, noise_weight if noise is not None else None, scale, shift, post)


def style_torgb_grad(x, weight, s, bias, skip=None, skip_up=False, sigmoid=False):
    """style_torgb under torch.autograd: gradients for x, weight, s, bias and skip."""
    return _ToRGB.apply(x, weight, s, bias, skip, bool(skip_up), bool(sigmoid))


def style_coeffs_grad(latent, mod_weight, mod_bias, w2, layers, sum_out):
    """style_coeffs under torch.autograd: gradients for latent, mod_weight, mod_bias and w2."""
    if w2 is None:
        w2 = latent.new_zeros((0,))
    s, d = _Coeffs.apply(latent, mod_weight, mod_bias, w2, tuple(tuple(l) for l in layers), int(sum_out))
    return s, (d if sum_out else None)


# ------------------------------------------------------------------ the decoder

def _no_backward(tensors, what):
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what} is forward only: call it under torch.no_grad() "
                                  "(an input or a parameter requires grad, and there is no backward yet)")


def _module_get(root):
    def get(name):
        obj = root
        for part in name.split("."):
            obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
        return obj
    return get


class StyleDecoder:
    """StyleGAN2GeneratorCSFT / StyleGAN2GeneratorCSFT_small.  Holds references to the parameters it was
    built from (no copies of the conv weights); the stacked modulation weights and the sum-of-squares
    tables of the no-grad path are copies: call invalidate() after a weight update.  forward(grad=True)
    builds those tables from the live parameters on every call and is differentiable."""

    def __init__(self, get, small, levels, mlp_index, eps=1e-8):
        self._get, self.small, self.levels, self._mlp_index = get, bool(small), int(levels), tuple(mlp_index)
        self.eps = float(eps)
        self.invalidate()

    @classmethod
    def from_module(cls, dec):
        """dec: a decoder with the reference's attribute names -- style_mlp, constant_input, style_conv1,
        to_rgb1, style_convs, to_rgbs, and normal_convs (the `small` variant) or two style convs per level."""
        for name in ("style_mlp", "constant_input", "style_conv1", "to_rgb1", "style_convs", "to_rgbs"):
            if not hasattr(dec, name):
                raise RuntimeError(f"not a StyleGAN2 decoder: it has no {name}")
        small = hasattr(dec, "normal_convs")
        levels = len(dec.to_rgbs)
        if len(dec.style_convs) != (levels if small else 2 * levels) or (small and len(dec.normal_convs) != levels):
            raise RuntimeError("the decoder's style_convs / normal_convs / to_rgbs do not pair up")
        mlp = [i for i, m in enumerate(dec.style_mlp) if hasattr(m, "weight")]
        eps = float(getattr(dec.style_conv1.modulated_conv, "eps", 1e-8))
        return cls(_module_get(dec), small, levels, mlp, eps)

    @classmethod
    def from_state_dict(cls, sd, out_size, small, eps=1e-8, device="cuda"):
        """sd: the decoder's state_dict (the reference's names)."""
        levels = int(math.log2(out_size)) - 2
        if levels < 0 or 2 ** (levels + 2) != out_size:
            raise RuntimeError(f"out_size must be a power of two >= 4, got {out_size}")
        sd = {k: v.to(device=device, dtype=torch.float32) for k, v in sd.items() if not k.startswith("noises.")}
        mlp = sorted(int(k.split(".")[1]) for k in sd if k.startswith("style_mlp.") and k.endswith(".weight"))
        return cls(lambda name: sd[name], small, levels, mlp, eps)

    # -- parameters

    def _mod(self, prefix):
        g = self._get
        return dict(mod_w=g(prefix + ".modulated_conv.modulation.weight"), mod_b=g(prefix + ".modulated_conv.modulation.bias"),
                    weight=g(prefix + ".modulated_conv.weight"), bias=g(prefix + ".bias"))

    def _style(self, prefix):
        return dict(self._mod(prefix), nw=self._get(prefix + ".weight"))

    def invalidate(self):
        """Rebuild everything derived from the parameters."""
        g = self._get
        self.mlp = [(g(f"style_mlp.{i}.weight"), g(f"style_mlp.{i}.bias")) for i in self._mlp_index]
        self.const = g("constant_input.weight")
        self.conv1, self.rgb1 = self._style("style_conv1"), self._mod("to_rgb1")
        self.level = []
        for i in range(self.levels):
            if self.small:
                lv = dict(a=self._style(f"style_convs.{i}"), b=None,
                          normal=(g(f"normal_convs.{i}.0.weight"), g(f"normal_convs.{i}.0.bias")))
            else:
                lv = dict(a=self._style(f"style_convs.{2 * i}"), b=self._style(f"style_convs.{2 * i + 1}"), normal=None)
            lv["rgb"] = self._mod(f"to_rgbs.{i}")
            self.level.append(lv)
        mods = [self.conv1, self.rgb1]
        for lv in self.level:
            mods += [lv["a"]] + ([lv["b"]] if lv["b"] is not None else []) + [lv["rgb"]]
        for t in self.parameters():
            _gpu(t, "a decoder parameter")
        s_off = d_off = w2_off = 0
        table, w2 = [], []
        with torch.no_grad():
            for m in mods:
                w = m["weight"]  # [1, c_out, c_in, k, k]
                c_out, c_in = int(w.shape[1]), int(w.shape[2])
                m["s"] = (s_off, s_off + c_in)
                if "nw" in m:  # a StyleConv: demodulated
                    m["d"] = (d_off, d_off + c_out)
                    m["conv_w"] = w[0]
                    w2.append(w[0].pow(2).sum((-1, -2)).reshape(-1))
                    table.append((s_off, c_in, d_off, c_out, w2_off, self.eps))
                    d_off += c_out
                    w2_off += c_out * c_in
                else:  # a ToRGB
                    if w.shape[-1] != 1 or c_out > 4 or c_in > 512:
                        raise RuntimeError(f"a ToRGB must be 1x1 with out_dim <= 4 and C <= 512, got {tuple(w.shape)}")
                    m["rgb_w"] = w.reshape(c_out, c_in)
                    table.append((s_off, c_in, -1, c_out, 0, self.eps))
                s_off += c_in
            self.mod_weight = torch.cat([m["mod_w"] for m in mods]).contiguous()
            self.mod_bias = torch.cat([m["mod_b"] for m in mods]).contiguous()
            self.w2 = torch.cat(w2).contiguous()
        self.table, self.sum_out, self._mods = table, d_off, mods
        self.num_noise = 1 + self.levels * (1 if self.small else 2)
        self.out_dim = int(self.rgb1["weight"].shape[1])
        self.num_style_feat = int(self.mod_weight.shape[1])

    def parameters(self):
        out = [t for pair in self.mlp for t in pair] + [self.const]
        mods = [self.conv1, self.rgb1]
        for lv in self.level:
            mods += [lv["a"], lv["rgb"]] + ([lv["b"]] if lv["b"] is not None else [])
            out += list(lv["normal"] or ())
        for m in mods:
            out += [m[k] for k in ("mod_w", "mod_b", "weight", "bias", "nw") if k in m]
        return out

    # -- the call

    def _noise(self, noise, generator, B, dev):
        """The per-style-conv noise tensors: the caller's list, or fresh normals [B,1,h,w] drawn as
        StyleConv.forward draws them."""
        sizes = [4] + [2 ** (3 + i) for i in range(self.levels) for _ in range(1 if self.small else 2)]
        if noise is None:
            return [torch.randn((B, 1, n, n), dtype=torch.float32, device=dev, generator=generator) for n in sizes]
        if len(noise) != self.num_noise:
            raise RuntimeError(f"noise must list {self.num_noise} tensors (one per style conv), got {len(noise)}")
        return list(noise)

    def _style_conv(self, x, m, s, d, noise, up, scale=None, shift=None, post=None, modulated=False):
        if not modulated:
            x = style_upmod(x, s[:, m["s"][0]:m["s"][1]], up=up)
        y = F.conv2d(x, m["conv_w"], padding=m["conv_w"].shape[-1] // 2)
        return style_epilogue(y, d[:, m["d"][0]:m["d"][1]], m["bias"], noise, m["nw"], scale, shift, post, out=y)

    def forward(self, style_code, conditions, noise=None, generator=None, sigmoid=False, grad=False):
        """style_code [B,S]; conditions: the SFT maps, scale and shift alternating, as StyleUNet.forward
        builds them; noise: None (fresh normals per style conv, from `generator`) or one tensor
        [1 or B,1,h,w] per style conv; sigmoid: StyleUNet's final activation, fused into the last ToRGB;
        grad: differentiable (the same values; with grad disabled it is the plain forward)."""
        _gpu(style_code, "style_code", 2)
        conditions = [_gpu(c, "a condition map", 4) for c in conditions]
        if noise is not None:
            noise = [_gpu(n, "a noise tensor", 4) for n in noise]
        if grad and torch.is_grad_enabled():
            return self._forward_grad(style_code, conditions, noise, generator, sigmoid)
        _no_backward([style_code] + conditions + list(noise or ()) + self.parameters(), "StyleDecoder.forward")
        B, dev = int(style_code.shape[0]), style_code.device
        noise = self._noise(noise, generator, B, dev)
        lat = style_code * torch.rsqrt(torch.mean(style_code ** 2, dim=1, keepdim=True) + 1e-8)
        for w, b in self.mlp:
            lat = F.leaky_relu_(F.linear(lat, w, b), 0.2)
        s, d = style_coeffs(lat, self.mod_weight, self.mod_bias, self.w2, self.table, self.sum_out)
        rows = lambda m: s[:, m["s"][0]:m["s"][1]]  # noqa: E731
        out = self._style_conv(self.const, self.conv1, s, d, noise[0], up=False)
        last = self.levels == 0
        skip = style_torgb(out, self.rgb1["rgb_w"], rows(self.rgb1), self.rgb1["bias"], sigmoid=sigmoid and last)
        n = 1
        for k, lv in enumerate(self.level):
            # the reference's index arithmetic: `i < len(conditions)` with i = 1 + k (small) or 1 + 2k
            i = 1 + k if self.small else 1 + 2 * k
            c0 = (i - 1) * 2 if self.small else i - 1
            scale, shift = (conditions[c0], conditions[c0 + 1]) if i < len(conditions) else (None, None)
            post = rows(lv["b"]) if lv["b"] is not None else None
            out = self._style_conv(out, lv["a"], s, d, noise[n], up=True, scale=scale, shift=shift, post=post)
            n += 1
            if self.small:
                out = F.leaky_relu_(F.conv2d(out, lv["normal"][0], lv["normal"][1], padding=lv["normal"][0].shape[-1] // 2),
                                    0.2)
            else:
                out = self._style_conv(out, lv["b"], s, d, noise[n], up=False, modulated=True)
                n += 1
            last = k == self.levels - 1
            skip = style_torgb(out, lv["rgb"]["rgb_w"], rows(lv["rgb"]), lv["rgb"]["bias"], skip=skip, skip_up=True,
                               sigmoid=sigmoid and last)
        return skip

    def _forward_grad(self, style_code, conditions, noise, generator, sigmoid):
        """forward() under autograd: the same kernels on the same values, the tables built from the live
        parameters with differentiable torch ops, the epilogue out of place (its backward reads the conv
        output), the convs, the MLP and normal_convs under torch's own autograd."""
        B, dev = int(style_code.shape[0]), style_code.device
        noise = [n.detach() for n in self._noise(noise, generator, B, dev)]
        mods = self._mods
        demod = [m for m in mods if "nw" in m]
        mod_weight = torch.cat([m["mod_w"] for m in mods]).contiguous()
        mod_bias = torch.cat([m["mod_b"] for m in mods]).contiguous()
        w2 = torch.cat([m["weight"][0].pow(2).sum((-1, -2)).reshape(-1) for m in demod]).contiguous()
        lat = style_code * torch.rsqrt(torch.mean(style_code ** 2, dim=1, keepdim=True) + 1e-8)
        for w, b in self.mlp:
            lat = F.leaky_relu_(F.linear(lat, w, b), 0.2)
        s, d = style_coeffs_grad(lat, mod_weight, mod_bias, w2, self.table, self.sum_out)
        # one split (one cat in the backward) instead of a slice per layer
        s_of = {id(m): t for m, t in zip(mods, s.split([m["s"][1] - m["s"][0] for m in mods], dim=1))}
        d_of = {id(m): t for m, t in zip(demod, d.split([m["d"][1] - m["d"][0] for m in demod], dim=1))}

        def style_conv(x, m, n, up, scale=None, shift=None, post=None, modulated=False):
            if not modulated:
                x = style_upmod_grad(x, s_of[id(m)], up=up)
            w = m["weight"][0]
            y = F.conv2d(x, w, padding=w.shape[-1] // 2)
            return style_epilogue_grad(y, d_of[id(m)], m["bias"], n, m["nw"], scale, shift, post)

        def to_rgb(x, m, skip, last):
            w = m["weight"]
            return style_torgb_grad(x, w.reshape(w.shape[1], w.shape[2]), s_of[id(m)], m["bias"], skip=skip,
                                    skip_up=skip is not None, sigmoid=sigmoid and last)

        out = style_conv(self.const, self.conv1, noise[0], up=False)
        skip = to_rgb(out, self.rgb1, None, self.levels == 0)
        n = 1
        for k, lv in enumerate(self.level):
            i = 1 + k if self.small else 1 + 2 * k  # the reference's index arithmetic, as in forward()
            c0 = (i - 1) * 2 if self.small else i - 1
            scale, shift = (conditions[c0], conditions[c0 + 1]) if i < len(conditions) else (None, None)
            post = s_of[id(lv["b"])] if lv["b"] is not None else None
            out = style_conv(out, lv["a"], noise[n], up=True, scale=scale, shift=shift, post=post)
            n += 1
            if self.small:
                w, b = lv["normal"]
                out = F.leaky_relu_(F.conv2d(out, w, b, padding=w.shape[-1] // 2), 0.2)
            else:
                out = style_conv(out, lv["b"], noise[n], up=False, modulated=True)
                n += 1
            skip = to_rgb(out, lv["rgb"], skip, k == self.levels - 1)
        return skip

    __call__ = forward


class StyleUNetRunner:
    """The reference's StyleUNet with its decoder on the HIP path.  The UNet half (conv_body_first,
    the ResBlocks, final_conv, final_linear, the SFT condition convs) runs through the module's own
    torch layers, without the condition maps' clones; the decoder through StyleDecoder."""

    def __init__(self, styleunet):
        self.net = styleunet
        self.decoder = StyleDecoder.from_module(styleunet.stylegan_decoder)

    def invalidate(self):
        self.decoder.invalidate()

    def _check(self, x, what, noise, extra_style, grad=False):
        _gpu(x, what, 4)
        if grad:
            return
        params = [p for p in self.net.parameters()] if hasattr(self.net, "parameters") else self.decoder.parameters()
        _no_backward([x, extra_style] + list(noise or ()) + params, "StyleUNetRunner")

    def forward(self, x, noise=None, generator=None, extra_style=None, grad=False):
        """x: the 32-channel render [B,in_dim,h,w] -> the refined image [B,out_dim,out_size,out_size].
        grad: differentiable with respect to x and every parameter of the module (the UNet half through
        torch's autograd, the decoder through StyleDecoder.forward(grad=True)); the same values."""
        net = self.net
        self._check(x, "x", noise, extra_style, grad)
        if x.shape[-1] < net.out_size:
            x = F.interpolate(x, size=(net.out_size, net.out_size), mode="bilinear", align_corners=False)
        if net.in_size <= net.out_size:
            feat = F.leaky_relu_(net.conv_body_first(x), negative_slope=0.2)
        else:
            feat = net.conv_body_first[1](F.leaky_relu_(net.conv_body_first[0](x), negative_slope=0.2))
        return self.rest(feat, noise=noise, generator=generator, extra_style=extra_style, grad=grad)

    def rest(self, feat, noise=None, generator=None, extra_style=None, grad=False):
        """feat: conv_body_first + LeakyReLU of the render (RefineHead.out, render_refined's `refined`)."""
        net = self.net
        self._check(feat, "feat", noise, extra_style, grad)
        skips = []
        for down in net.conv_body_down:
            feat = down(feat)
            skips.insert(0, feat)
        feat = F.leaky_relu_(net.final_conv(feat), negative_slope=0.2)
        style = net.final_linear(feat.reshape(feat.size(0), -1))
        if getattr(net, "extra_style_dim", -1) > 0 and extra_style is not None:
            style = net.style_fuse(torch.cat([style, extra_style], dim=1))
        conditions = []
        for i, up in enumerate(net.conv_body_up):
            feat = up(feat + skips[i])
            conditions += [net.condition_scale[i](feat), net.condition_shift[i](feat)]
        return self.decoder.forward(style, conditions, noise=noise, generator=generator, sigmoid=bool(net.activation),
                                    grad=grad)

    __call__ = forward
