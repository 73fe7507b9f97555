"""Builds tests/golden/refiner_decoder.npz: float64 outputs of the REFERENCE's own StyleGAN2 decoders
(models/modules/net_module/styleunet/styleunet.py, imported by file path) on small seeded inputs.

Run ONLY where the reference checkout exists (the committed npz is all the tests read):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_refiner_golden.py [path/to/styleunet.py]

Both variants (StyleGAN2GeneratorCSFT as `full`, StyleGAN2GeneratorCSFT_small as `small`) at out_size 16,
channel_scale 32 (8 channels at every level), num_style_feat 64, num_mlp 2, out_dim 3, B = 2.  The noise
weights and all the StyleConv / ToRGB biases, which the reference initialises to 0, get seeded non-zero
values.  The reference is called with randomize_noise=False after its `noises` buffers have been
replaced by this script's explicit tensors: for the small variant the stored buffers have the wrong
sizes (resolutions 4, 8, 8 for layers that run at 4, 8, 16), so as constructed it cannot run that way.
The first noise tensor has batch 1, the others batch B.

Per variant v the file holds  v/sd/<name> (float32 parameters), v/style [B,64], v/cond/<i>, v/noise/<i>
(float32 inputs) and v/out [B,3,16,16] (float64: the module and the inputs cast to double).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/models/modules/net_module/styleunet/styleunet.py"
OUT = os.path.join(HERE, "refiner_decoder.npz")
CFG = dict(out_size=16, out_dim=3, num_style_feat=64, num_mlp=2, channel_scale=32)
B = 2


def _ref_module(path):
    spec = importlib.util.spec_from_file_location("ref_styleunet", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ref = _ref_module(sys.argv[1] if len(sys.argv) > 1 else REF)
    out = {}
    for v, cls in (("full", ref.StyleGAN2GeneratorCSFT), ("small", ref.StyleGAN2GeneratorCSFT_small)):
        torch.manual_seed(11 if v == "full" else 12)
        dec = cls(**CFG).eval()
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for name, p in dec.named_parameters():
                style_conv = name.startswith(("style_conv1.", "style_convs."))
                if name.endswith(".bias") and p.dim() == 4:       # StyleConv / ToRGB bias
                    p.copy_(torch.randn(p.shape, generator=g) * 0.3)
                elif style_conv and name.count(".") == (1 if name.startswith("style_conv1.") else 2) and \
                        name.endswith(".weight"):                 # StyleConv's noise weight
                    assert p.shape == (1,), (name, p.shape)
                    p.copy_(torch.randn(1, generator=g) * 0.5 + 0.7)
                elif name.startswith("style_mlp.") and name.endswith(".bias"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        sizes = [4] + [2 ** i for i in (3, 4) for _ in range(1 if v == "small" else 2)]
        assert len(sizes) == dec.num_layers
        noise = [torch.randn((1 if i == 0 else B, 1, n, n), generator=g) for i, n in enumerate(sizes)]
        style = torch.randn((B, CFG["num_style_feat"]), generator=g)
        cond = [torch.randn((B, 8, n, n), generator=g) * s + m for n in (8, 16) for s, m in ((0.5, 1.0), (0.5, 0.0))]
        for k, p in dec.state_dict().items():
            if not k.startswith("noises."):
                out[f"{v}/sd/{k}"] = p.detach().numpy().astype(np.float32)
        dec = dec.double()
        dec.noises = torch.nn.Module()
        for i, n in enumerate(noise):
            dec.noises.register_buffer(f"noise{i}", n.double())
        with torch.no_grad():
            y = dec(style.double(), [c.double() for c in cond], randomize_noise=False)
        out[f"{v}/style"] = style.numpy()
        for i, c in enumerate(cond):
            out[f"{v}/cond/{i}"] = c.numpy()
        for i, n in enumerate(noise):
            out[f"{v}/noise/{i}"] = n.numpy()
        out[f"{v}/out"] = y.numpy()
        assert y.dtype == torch.float64 and tuple(y.shape) == (B, 3, 16, 16)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
