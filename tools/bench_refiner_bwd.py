"""Refiner decoder training-step timings: forward + backward of
StyleDecoder.forward(grad=True) and StyleUNetRunner.rest(grad=True) (guava_renderer_amd/refiner.py: the
glue and its backward in HIP, the convs under torch autograd) against the float32 torch autograd chain
of tests/refiner_ref.py, which is the reference's formulation and the yardstick: the parent commit
raises NotImplementedError here.  GUAVA's shape: out_size 512, channel_scale 1, num_style_feat 512,
num_mlp 8, the `small` decoder (32 -> 16 channels at the last level) at B = 1 and B = 6.  bench_refiner.py's
method: same process, same tensors, fixed noise; the two sides alternate window by window; HIP events
around each window of `--iters` steps after a warm-up, median of `--repeats` windows; kernel launches
per step on each side (torch.profiler's device events); peak memory of one step on each side
(torch.cuda.max_memory_allocated above what is allocated before the step).  Also the four backward
passes alone at the 512 x 512 level against their algorithmic bytes.  Prints one JSON line.

    python tools/bench_refiner_bwd.py [--iters 10] [--repeats 7] [--only decoder:1]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_refiner import launches, stats, timed_pair, window  # noqa: E402


def peak_mib(fn):
    """Peak allocation of one call above the allocation it starts from, MiB."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def pass_kernels(B, iters, repeats, dev):
    """The backward passes at the small decoder's 512 x 512 level (32 -> 16 channels, out_dim 3), and the
    coefficients' backward for the whole small decoder's layer table."""
    from guava_renderer_amd import refiner
    g = torch.Generator(device=dev).manual_seed(3)
    r = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
    x256, s32, g512 = r(B, 32, 256, 256), r(B, 32), r(B, 32, 512, 512)
    y, gy, d16, bias16, nw = r(B, 16, 512, 512), r(B, 16, 512, 512), r(B, 16).abs() + 0.1, r(16), r(1)
    noise, scale, shift = r(B, 1, 512, 512), r(B, 16, 512, 512), r(B, 16, 512, 512)
    w, s16, out, gout = r(3, 16), r(B, 16), torch.sigmoid(r(B, 3, 512, 512)), r(B, 3, 512, 512)
    px = 512 * 512
    cases = [
        # reads g_y and x, writes g_x
        ("upmod_backward", lambda: refiner.style_upmod_backward(g512, x256, s32, up=True), 4 * B * 32 * (px + 2 * px // 4)),
        # reads g_y, x, scale, shift and the noise plane, writes g_x, g_scale, g_shift
        ("epilogue_backward", lambda: refiner.style_epilogue_backward(gy, y, d16, bias16, noise, nw, scale, shift),
         4 * B * (7 * 16 + 1) * px),
        # reads g_out, y and x, writes g_x and the half-size g_skip
        ("torgb_backward", lambda: refiner.style_torgb_backward(gout, y, w, s16, y=out, skip="up"),
         4 * B * (2 * 3 * px + 2 * 16 * px + 3 * px // 4)),
    ]
    ch = [256, 256, 256, 256, 128, 64, 32, 16]  # the small decoder at 512: conv1 and 7 levels
    layers, s_off, d_off, w2_off = [], 0, 0, 0
    for c_in, c_out in zip(ch[:1] + ch[:-1], ch):
        layers.append((s_off, c_in, d_off, c_out, w2_off, 1e-8))
        s_off, d_off, w2_off = s_off + c_in, d_off + c_out, w2_off + c_in * c_out
        layers.append((s_off, c_out, -1, 3, 0, 1e-8))
        s_off += c_out
    gs, gd, sv, dv, w2 = r(B, s_off), r(B, d_off), r(B, s_off), r(B, d_off).abs() + 0.1, r(w2_off).abs()
    cases.append(("coeffs_backward", lambda: refiner.style_coeffs_backward(gs, gd, sv, dv, w2, layers),
                  4 * ((B + 1) * w2_off + 3 * B * (s_off + d_off))))  # w2 read once per frame, g_w2 written once
    res = []
    for name, fn, nbytes in cases:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = stats([window(fn, iters * 5) for _ in range(repeats)])
        res.append({"kernel": name, "B": B, "us": us, "algorithmic_bytes": nbytes,
                    "GBs": round(nbytes / us["median"] / 1e3, 1), "launches": launches(fn)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--only", default=None, help="one case, e.g. decoder:1, runner:6 or kernels")
    a = ap.parse_args()
    import refiner_ref
    from guava_renderer_amd.refiner import StyleUNetRunner
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = "cuda:0"
    out = {"workload": "StyleUNet refiner decoder, forward + backward", "out_size": a.size, "num_style_feat": 512,
           "num_mlp": 8, "channel_scale": 1, "small": True, "iters": a.iters, "repeats": a.repeats, "cases": [],
           "pass_kernels": []}
    torch.manual_seed(1)
    net = refiner_ref.StyleUNetRef(in_size=a.size, out_size=a.size, in_dim=32, out_dim=3, num_style_feat=512,
                                   num_mlp=8, activation=True, channel_scale=1, small=True).eval()
    net = refiner_ref.randomize_noise_params(net, 4).to(dev)
    run = StyleUNetRunner(net)
    params = [(k, p) for k, p in net.named_parameters() if not k.startswith("conv_body_first.")]  # (rest starts behind it)
    dec_params = list(net.stylegan_decoder.named_parameters())
    for what, B in (("decoder", 1), ("decoder", 6), ("runner", 1), ("runner", 6)):
        name = f"{what}:{B}"
        if a.only and a.only != name:
            continue
        g = torch.Generator(device=dev).manual_seed(5)
        feat = torch.nn.functional.leaky_relu(torch.randn((B, 16, a.size, a.size), device=dev, generator=g), 0.2)
        feat.requires_grad_(True)
        noise = [torch.randn((B, 1, n, n), device=dev, generator=g) for n in net.stylegan_decoder.noise_sizes()]
        G = torch.randn((B, 3, a.size, a.size), device=dev, generator=g)
        if what == "runner":
            named = [("feat", feat)] + params
            f_ours = lambda: run.rest(feat, noise=noise, grad=True)  # noqa: E731
            f_ref = lambda: net.rest(feat, noise)  # noqa: E731
        else:
            style = torch.randn((B, 512), device=dev, generator=g).requires_grad_(True)
            ch = refiner_ref.channels(1)
            cond = [(torch.randn((B, ch[2 ** i], 2 ** i, 2 ** i), device=dev, generator=g) * 0.5 + m).requires_grad_(True)
                    for i in range(3, net.log_size + 1) for m in (1.0, 0.0)]
            named = [("style", style)] + [(f"cond/{i}", c) for i, c in enumerate(cond)] + dec_params
            f_ours = lambda: run.decoder.forward(style, cond, noise=noise, sigmoid=True, grad=True)  # noqa: E731
            f_ref = lambda: torch.sigmoid(net.stylegan_decoder(style, cond, noise))  # noqa: E731

        leaves = [p for _, p in named]

        def step(f, leaves=leaves, G=G):
            return torch.autograd.grad((f() * G).sum(), leaves)

        ours, ref = (lambda: step(f_ours)), (lambda: step(f_ref))  # noqa: E731
        ga, gb = ours(), ref()
        diff, where = max((float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)), k)
                          for (k, _), x, y in zip(named, ga, gb))
        del ga, gb
        t_o, t_r = timed_pair(ours, ref, a.iters, a.repeats, warmup=3)
        case = {"case": name, "max_grad_diff_of_scale_vs_torch": diff, "max_grad_diff_tensor": where, "fused_us": t_o, "torch_us": t_r,
                "speedup": round(t_r["median"] / t_o["median"], 2),
                "peak_MiB": {"fused": peak_mib(ours), "torch": peak_mib(ref)}}
        print(json.dumps(case), file=sys.stderr, flush=True)  # (the timings, should the profiler stall)
        case["launches"] = {"fused": launches(ours), "torch": launches(ref)}
        out["cases"].append(case)
    if not a.only or a.only == "kernels":
        for B in (1, 6):
            out["pass_kernels"] += pass_kernels(B, a.iters, a.repeats, dev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
