"""A torch restatement of the reference's StyleUNet refiner (models/modules/net_module/styleunet/
styleunet.py), written for the tests: the grouped-conv formulation of the modulated conv, any dtype,
explicit noise tensors only (the reference's stored noise buffers have the wrong sizes for its `small`
decoder and are not mirrored).  Parameter names are the reference's, so a state_dict carries over
(its `noises.*` buffers aside: load_reference_state drops them).

tests/test_refiner_ref.py pins the two decoders in float64 against the reference's own float64 outputs
(tests/golden/refiner_decoder.npz); the GPU tests and tools/bench_refiner.py use them as the float64
reference and as the torch chain to time against.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

BASE_CHANNELS = {4: 256, 8: 256, 16: 256, 32: 256, 64: 128, 128: 64, 256: 32, 512: 16, 1024: 8}


def channels(channel_scale):
    return {k: int(v / channel_scale) for k, v in BASE_CHANNELS.items()}


def up2(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


class NormStyleCode(nn.Module):
    def forward(self, x):
        return x * torch.rsqrt(torch.mean(x ** 2, dim=1, keepdim=True) + 1e-8)


class ConstantInput(nn.Module):
    def __init__(self, c, size):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(1, c, size, size))


class ModulatedConv2d(nn.Module):
    """weight [1,c_out,c_in,k,k] * style [b,1,c_in,1,1], demodulated over (c_in,k,k), as a grouped conv."""

    def __init__(self, c_in, c_out, k, num_style_feat, demodulate, upsample, eps=1e-8):
        super().__init__()
        self.c_in, self.c_out, self.k, self.demodulate, self.upsample, self.eps = c_in, c_out, k, demodulate, upsample, eps
        self.modulation = nn.Linear(num_style_feat, c_in)
        self.weight = nn.Parameter(torch.randn(1, c_out, c_in, k, k) / math.sqrt(c_in * k * k))

    def forward(self, x, style):
        b = x.shape[0]
        w = self.weight * self.modulation(style).view(b, 1, self.c_in, 1, 1)
        if self.demodulate:
            w = w * torch.rsqrt(w.pow(2).sum([2, 3, 4]) + self.eps).view(b, self.c_out, 1, 1, 1)
        if self.upsample:
            x = up2(x)
        h, wd = x.shape[2:]
        y = F.conv2d(x.reshape(1, b * self.c_in, h, wd), w.view(b * self.c_out, self.c_in, self.k, self.k),
                     padding=self.k // 2, groups=b)
        return y.view(b, self.c_out, h, wd)


class StyleConv(nn.Module):
    def __init__(self, c_in, c_out, num_style_feat, upsample):
        super().__init__()
        self.modulated_conv = ModulatedConv2d(c_in, c_out, 3, num_style_feat, True, upsample)
        self.weight = nn.Parameter(torch.zeros(1))
        self.bias = nn.Parameter(torch.zeros(1, c_out, 1, 1))

    def forward(self, x, style, noise):
        y = self.modulated_conv(x, style) * 2 ** 0.5
        return F.leaky_relu(y + self.weight * noise + self.bias, 0.2)


class ToRGB(nn.Module):
    def __init__(self, c_in, out_dim, num_style_feat, upsample):
        super().__init__()
        self.upsample = upsample
        self.modulated_conv = ModulatedConv2d(c_in, out_dim, 1, num_style_feat, False, False)
        self.bias = nn.Parameter(torch.zeros(1, out_dim, 1, 1))

    def forward(self, x, style, skip=None):
        y = self.modulated_conv(x, style) + self.bias
        if skip is not None:
            y = y + (up2(skip) if self.upsample else skip)
        return y


class StyleDecoderRef(nn.Module):
    """Both decoder variants: small=True has one style conv and one plain conv + LeakyReLU per level
    (normal_convs), small=False two style convs."""

    def __init__(self, out_size, out_dim=3, num_style_feat=512, num_mlp=8, channel_scale=1, small=False):
        super().__init__()
        ch = channels(channel_scale)
        self.small, self.log_size = small, int(math.log2(out_size))
        mlp = [NormStyleCode()]
        for _ in range(num_mlp):
            mlp += [nn.Linear(num_style_feat, num_style_feat), nn.LeakyReLU(0.2)]
        self.style_mlp = nn.Sequential(*mlp)
        self.constant_input = ConstantInput(ch[4], 4)
        self.style_conv1 = StyleConv(ch[4], ch[4], num_style_feat, False)
        self.to_rgb1 = ToRGB(ch[4], out_dim, num_style_feat, False)
        self.style_convs, self.to_rgbs = nn.ModuleList(), nn.ModuleList()
        if small:
            self.normal_convs = nn.ModuleList()
        c_in = ch[4]
        for i in range(3, self.log_size + 1):
            c_out = ch[2 ** i]
            self.style_convs.append(StyleConv(c_in, c_out, num_style_feat, True))
            if small:
                self.normal_convs.append(nn.Sequential(nn.Conv2d(c_out, c_out, 3, padding=1), nn.LeakyReLU(0.2)))
            else:
                self.style_convs.append(StyleConv(c_out, c_out, num_style_feat, False))
            self.to_rgbs.append(ToRGB(c_out, out_dim, num_style_feat, True))
            c_in = c_out

    def noise_sizes(self):
        return [4] + [2 ** i for i in range(3, self.log_size + 1) for _ in range(1 if self.small else 2)]

    def forward(self, styles, conditions, noise):
        """noise: one tensor [1 or B,1,h,w] per style conv (noise_sizes())."""
        lat = self.style_mlp(styles)
        out = self.constant_input.weight.repeat(lat.shape[0], 1, 1, 1)
        out = self.style_conv1(out, lat, noise[0])
        skip = self.to_rgb1(out, lat)
        n = 1
        for k, to_rgb in enumerate(self.to_rgbs):
            if self.small:
                i, c0 = 1 + k, 2 * k
            else:
                i, c0 = 1 + 2 * k, 2 * k
            out = (self.style_convs[k] if self.small else self.style_convs[2 * k])(out, lat, noise[n])
            n += 1
            if i < len(conditions):
                out = out * conditions[c0] + conditions[c0 + 1]
            if self.small:
                out = self.normal_convs[k](out)
            else:
                out = self.style_convs[2 * k + 1](out, lat, noise[n])
                n += 1
            skip = to_rgb(out, lat, skip)
        return skip


class ResBlock(nn.Module):
    def __init__(self, c_in, c_out, mode):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, c_in, 3, 1, 1)
        self.conv2 = nn.Conv2d(c_in, c_out, 3, 1, 1)
        self.skip = nn.Conv2d(c_in, c_out, 1, bias=False)
        self.scale_factor = 0.5 if mode == "down" else 2

    def _resize(self, x):
        return F.interpolate(x, scale_factor=self.scale_factor, mode="bilinear", align_corners=False)

    def forward(self, x):
        y = self._resize(F.leaky_relu(self.conv1(x), 0.2))
        return F.leaky_relu(self.conv2(y), 0.2) + self.skip(self._resize(x))


class StyleUNetRef(nn.Module):
    def __init__(self, in_size, out_size, in_dim, out_dim, num_style_feat=512, num_mlp=8, activation=True,
                 channel_scale=1, small=False):
        super().__init__()
        ch = channels(channel_scale)
        assert in_size <= out_size, "the in_size > out_size entry block is not restated"
        self.activation, self.in_size, self.out_size = activation, in_size, out_size
        self.log_size = int(math.log2(out_size))
        self.conv_body_first = nn.Conv2d(in_dim, ch[out_size], 1)
        self.conv_body_down, self.conv_body_up = nn.ModuleList(), nn.ModuleList()
        c = ch[out_size]
        for i in range(self.log_size, 2, -1):
            self.conv_body_down.append(ResBlock(c, ch[2 ** (i - 1)], "down"))
            c = ch[2 ** (i - 1)]
        self.final_conv = nn.Conv2d(c, ch[4], 3, 1, 1)
        c = ch[4]
        for i in range(3, self.log_size + 1):
            self.conv_body_up.append(ResBlock(c, ch[2 ** i], "up"))
            c = ch[2 ** i]
        self.final_linear = nn.Linear(ch[4] * 16, num_style_feat)
        self.stylegan_decoder = StyleDecoderRef(out_size, out_dim, num_style_feat, num_mlp, channel_scale, small)
        self.condition_scale, self.condition_shift = nn.ModuleList(), nn.ModuleList()
        for i in range(3, self.log_size + 1):
            for lst in (self.condition_scale, self.condition_shift):
                lst.append(nn.Sequential(nn.Conv2d(ch[2 ** i], ch[2 ** i], 3, 1, 1), nn.LeakyReLU(0.2),
                                         nn.Conv2d(ch[2 ** i], ch[2 ** i], 3, 1, 1)))

    def first(self, x):
        """conv_body_first + LeakyReLU: what the fused refiner head produces."""
        if x.shape[-1] < self.out_size:
            x = F.interpolate(x, size=(self.out_size, self.out_size), mode="bilinear", align_corners=False)
        return F.leaky_relu(self.conv_body_first(x), 0.2)

    def forward(self, x, noise):
        return self.rest(self.first(x), noise)

    def rest(self, feat, noise):
        """Everything after conv_body_first + LeakyReLU.  The condition maps are cloned as the reference
        clones them (styleunet.py:196, :198): no change in value, but part of the chain that is timed."""
        skips = []
        for down in self.conv_body_down:
            feat = down(feat)
            skips.insert(0, feat)
        feat = F.leaky_relu(self.final_conv(feat), 0.2)
        style = self.final_linear(feat.reshape(feat.size(0), -1))
        conditions = []
        for i, up in enumerate(self.conv_body_up):
            feat = up(feat + skips[i])
            conditions += [self.condition_scale[i](feat).clone(), self.condition_shift[i](feat).clone()]
        image = self.stylegan_decoder(style, conditions, noise)
        return torch.sigmoid(image) if self.activation else image


def load_reference_state(module, sd):
    """Load a reference state_dict (tensors or numpy arrays), its noise buffers dropped."""
    sd = {k: torch.as_tensor(v) for k, v in sd.items() if ".noises." not in k and not k.startswith("noises.")}
    module.load_state_dict(sd, strict=True)
    return module


def randomize_noise_params(module, seed):
    """The reference initialises every StyleConv's noise weight and every bias to 0, which hides errors
    in those terms: give them values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (StyleConv, ToRGB)):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
            if isinstance(m, StyleConv):
                m.weight.copy_(torch.randn(1, generator=g) * 0.5 + 0.7)
    return module
