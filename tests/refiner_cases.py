"""A numpy restatement of the refiner decoder kernels' stated arithmetic (include/gsr_refiner.h,
guava_renderer_amd/csrc/refiner_dev.h): float32 throughout, every operation rounded as written, so the
GPU's upmod, epilogue and torgb must agree bit for bit; coeffs is stated up to the order of its sums and
is restated in float64 with its bounds.  decoder() chains them with a float64 conv into the whole
decoder, as guava_renderer_amd/refiner.py chains the kernels with F.conv2d.
"""
import os

import numpy as np

from gaussian_extract_ref import ex_sigmoid

F32 = np.float32
SQRT2 = F32(2 ** 0.5)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refiner_decoder.npz")
CFG = dict(out_size=16, out_dim=3, num_style_feat=64, num_mlp=2, channel_scale=32)  # make_refiner_golden.py's
BAR = 1e-5  # against float64: of scale before the sigmoid, absolute after it


def load_variant(v):
    """The golden's variant "full" or "small" -> (state dict of numpy arrays, style, conditions, noise,
    the reference's float64 output)."""
    z = np.load(GOLDEN)
    sd = {k[len(v) + 4:]: z[k] for k in z.files if k.startswith(f"{v}/sd/")}
    lst = lambda name: [z[f"{v}/{name}/{i}"] for i in range(len([k for k in z.files if k.startswith(f"{v}/{name}/")]))]  # noqa: E731
    return sd, z[f"{v}/style"], lst("cond"), lst("noise"), z[f"{v}/out"]


def scale_err(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def tap(near, far):
    """0.75f*near + 0.25f*far, both products rounded."""
    return F32(0.75) * near + F32(0.25) * far


def up_index(n_out, n_in):
    """Nearer and farther (clamped) input index of every output index of one axis."""
    j = np.arange(n_out)
    near = j >> 1
    far = np.clip(np.where(j & 1, near + 1, near - 1), 0, n_in - 1)
    return near, far


def up2(x):
    """[..., h, w] -> [..., 2h, 2w]: rows first, then columns."""
    x = np.asarray(x, F32)
    h, w = x.shape[-2:]
    rn, rf = up_index(2 * h, h)
    cn, cf = up_index(2 * w, w)
    v = tap(x[..., rn, :], x[..., rf, :])
    return tap(v[..., :, cn], v[..., :, cf])


def upmod(x, s, up=True):
    """s[b,c] * up2(x[b,c]) or s[b,c] * x[b,c]; x of batch 1 broadcasts."""
    x, s = np.asarray(x, F32), np.asarray(s, F32)
    v = up2(x) if up else x
    return (s[:, :, None, None] * v).astype(F32)


def epilogue(x, d, bias, noise=None, noise_weight=None, scale=None, shift=None, post=None):
    x = np.asarray(x, F32)
    B, C = x.shape[:2]
    a = SQRT2 * np.asarray(d, F32) if d is not None else np.full((B, C), SQRT2, F32)
    n = F32(noise_weight) * np.asarray(noise, F32) if noise is not None else F32(0.0)
    v = ((a[:, :, None, None] * x) + n) + np.asarray(bias, F32).reshape(1, C, 1, 1)
    y = np.where(v >= 0, v, F32(0.2) * v).astype(F32)
    if scale is not None:
        y = (y * np.asarray(scale, F32)) + np.asarray(shift, F32)
    if post is not None:
        y = y * np.asarray(post, F32)[:, :, None, None]
    return y.astype(F32)


def torgb(x, weight, s, bias, skip=None, skip_up=False, sigmoid=False):
    x, weight, s = np.asarray(x, F32), np.asarray(weight, F32), np.asarray(s, F32)
    B, C, H, W = x.shape
    O = weight.shape[0]
    wm = weight[None, :, :] * s[:, None, :]  # [B,O,C]
    acc = wm[:, :, 0, None, None] * x[:, None, 0]
    for c in range(1, C):
        acc = acc + wm[:, :, c, None, None] * x[:, None, c]
    acc = acc + np.asarray(bias, F32).reshape(1, O, 1, 1)
    if skip is not None:
        acc = acc + (up2(skip) if skip_up else np.asarray(skip, F32))
    assert acc.dtype == F32
    return ex_sigmoid(acc).astype(F32) if sigmoid else acc


def coeffs64(latent, mod_weight, mod_bias):
    """s in float64 and the magnitude sum|w*l| + |b| its float32 bound scales with."""
    l, w, b = (np.asarray(a, np.float64) for a in (latent, mod_weight, mod_bias))
    return l @ w.T + b, np.abs(l) @ np.abs(w).T + np.abs(b)


def demod64(s, w2, eps):
    """d in float64 from given s [B,c_in] and w2 [c_out,c_in]."""
    s, w2 = np.asarray(s, np.float64), np.asarray(w2, np.float64)
    return 1.0 / np.sqrt((s * s) @ w2.T + np.float64(F32(eps)))


def coeffs32(latent, mod_weight, mod_bias):
    """A float32 s in numpy's own summation order (the chained decoder's; within the same bound)."""
    return (np.asarray(latent, F32) @ np.asarray(mod_weight, F32).T + np.asarray(mod_bias, F32)).astype(F32)


def demod32(s, w2, eps):
    s, w2 = np.asarray(s, F32), np.asarray(w2, F32)
    acc = ((s * s)[:, None, :] * w2[None]).sum(-1, dtype=F32)
    return (F32(1.0) / np.sqrt(acc + F32(eps))).astype(F32)


def conv64(x, w, bias=None):
    """A float64 conv (stride 1, same padding) of float32 operands, rounded to float32 once."""
    import torch
    import torch.nn.functional as F
    y = F.conv2d(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64)),
                 None if bias is None else torch.from_numpy(np.asarray(bias, np.float64)), padding=w.shape[-1] // 2)
    return y.numpy().astype(F32)


def decoder(sd, small, style, conditions, noise, sigmoid=False, eps=1e-8):
    """The whole decoder from a state dict of numpy arrays (the reference's names): the style MLP in
    float64 rounded to float32, then the four kernels' arithmetic around float64 convs."""
    levels = len([k for k in sd if k.startswith("to_rgbs.") and k.endswith(".bias") and k.count(".") == 2])
    lat = np.asarray(style, np.float64)
    lat = lat / np.sqrt(np.mean(lat ** 2, axis=1, keepdims=True) + 1e-8)
    for i in sorted(int(k.split(".")[1]) for k in sd if k.startswith("style_mlp.") and k.endswith(".weight")):
        lat = lat @ sd[f"style_mlp.{i}.weight"].astype(np.float64).T + sd[f"style_mlp.{i}.bias"]
        lat = np.where(lat >= 0, lat, 0.2 * lat)
    lat = lat.astype(F32)

    def s_of(p):
        return coeffs32(lat, sd[p + ".modulated_conv.modulation.weight"], sd[p + ".modulated_conv.modulation.bias"])

    def style_conv(x, p, n, up, scale=None, shift=None, post=None, modulated=False):
        w = sd[p + ".modulated_conv.weight"][0]
        s = s_of(p)
        d = demod32(s, (w.astype(F32) ** 2).sum((-1, -2), dtype=F32), eps)
        if not modulated:
            x = upmod(x, s, up)
        return epilogue(conv64(x, w), d, sd[p + ".bias"], n, sd[p + ".weight"][0], scale, shift, post)

    def to_rgb(x, p, skip, last):
        w = sd[p + ".modulated_conv.weight"][0, :, :, 0, 0]
        return torgb(x, w, s_of(p), sd[p + ".bias"], skip, skip_up=skip is not None, sigmoid=sigmoid and last)

    out = style_conv(sd["constant_input.weight"], "style_conv1", noise[0], False)
    skip = to_rgb(out, "to_rgb1", None, levels == 0)
    n = 1
    for k in range(levels):
        i = 1 + k if small else 1 + 2 * k
        scale, shift = (conditions[2 * k], conditions[2 * k + 1]) if i < len(conditions) else (None, None)
        if small:
            out = style_conv(out, f"style_convs.{k}", noise[n], True, scale, shift)
            n += 1
            y = conv64(out, sd[f"normal_convs.{k}.0.weight"], sd[f"normal_convs.{k}.0.bias"])
            out = np.where(y >= 0, y, F32(0.2) * y).astype(F32)
        else:
            out = style_conv(out, f"style_convs.{2 * k}", noise[n], True, scale, shift, post=s_of(f"style_convs.{2 * k + 1}"))
            out = style_conv(out, f"style_convs.{2 * k + 1}", noise[n + 1], False, modulated=True)
            n += 2
        skip = to_rgb(out, f"to_rgbs.{k}", skip, k == levels - 1)
    return skip
