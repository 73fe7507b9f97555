"""Builds tests/golden/refiner_decoder_grad.npz: float64 gradients of the REFERENCE's own StyleGAN2
decoders (models/modules/net_module/styleunet/styleunet.py, imported by file path) on the parameters and
inputs already in tests/golden/refiner_decoder.npz.

Run ONLY where the reference checkout exists (the committed npz is all the tests read):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_refiner_grad_golden.py [path/to/styleunet.py]

Per variant v ("full", "small") the loss is sum(out * G) for a seeded cotangent G [B,3,16,16] (standard
normal, float64), the module and the inputs cast to double, the noise injected as make_refiner_golden.py
injects it.  The file holds  v/G,  v/grad/sd/<name> for every parameter,  v/grad/style  and
v/grad/cond/<i> for the four condition maps, all float64.  The gradients are random to the last bit and do
not compress, and the file has to stay under 400 KB like refiner_decoder.npz; so each gradient is rounded
to 41 significant bits (the low 12 mantissa bits zero: 2.3e-13 relative per element, well inside the 1e-12
of scale the tests ask of a float64 restatement), which is what lets the compressor fit them.  G is exact.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_refiner_golden import CFG, REF, _ref_module  # noqa: E402

SRC = os.path.join(HERE, "refiner_decoder.npz")
OUT = os.path.join(HERE, "refiner_decoder_grad.npz")


def _round41(a):
    """float64 rounded to nearest with the low 12 mantissa bits zero."""
    bits = np.ascontiguousarray(a, np.float64).view(np.uint64)
    return ((bits + np.uint64(1 << 11)) & ~np.uint64((1 << 12) - 1)).view(np.float64).reshape(np.shape(a))


def main():
    ref = _ref_module(sys.argv[1] if len(sys.argv) > 1 else REF)
    z = np.load(SRC)
    out = {}
    for v, cls in (("full", ref.StyleGAN2GeneratorCSFT), ("small", ref.StyleGAN2GeneratorCSFT_small)):
        dec = cls(**CFG).eval()
        sd = {k[len(v) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{v}/sd/")}
        own = dec.state_dict()
        sd.update({k: p for k, p in own.items() if k.startswith("noises.")})
        dec.load_state_dict(sd, strict=True)
        dec = dec.double()
        count = lambda name: len([k for k in z.files if k.startswith(f"{v}/{name}/")])  # noqa: E731
        noise = [torch.from_numpy(z[f"{v}/noise/{i}"]).double() for i in range(count("noise"))]
        cond = [torch.from_numpy(z[f"{v}/cond/{i}"]).double().requires_grad_(True) for i in range(count("cond"))]
        style = torch.from_numpy(z[f"{v}/style"]).double().requires_grad_(True)
        dec.noises = torch.nn.Module()
        for i, n in enumerate(noise):
            dec.noises.register_buffer(f"noise{i}", n)
        y = dec(style, cond, randomize_noise=False)
        assert float((y.detach() - torch.from_numpy(z[f"{v}/out"])).abs().max()) == 0.0, "not the golden's forward"
        G = torch.randn(y.shape, generator=torch.Generator().manual_seed(31 if v == "full" else 32), dtype=torch.float64)
        (y * G).sum().backward()
        out[f"{v}/G"] = G.numpy()
        for k, p in dec.named_parameters():
            assert p.grad is not None and p.grad.dtype == torch.float64, k
            out[f"{v}/grad/sd/{k}"] = _round41(p.grad.numpy())
        out[f"{v}/grad/style"] = _round41(style.grad.numpy())
        for i, c in enumerate(cond):
            out[f"{v}/grad/cond/{i}"] = _round41(c.grad.numpy())
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
