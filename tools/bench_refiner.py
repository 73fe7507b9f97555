"""Refiner decoder timings: StyleDecoder.forward and StyleUNetRunner.rest
(guava_renderer_amd/refiner.py: the modulated convs as plain convs, the glue in HIP) against the torch
chain of tests/refiner_ref.py, which is the reference's formulation (per-call weight modulation, grouped
conv, separate upsample / noise / bias / LeakyReLU / SFT passes) and the yardstick: the parent commit
has no such operation.  GUAVA's shape: out_size 512, channel_scale 1, num_style_feat 512, num_mlp 8,
the `small` decoder at B = 1 and B = 6, and the two-style-conv decoder at B = 1.  Same process, same
tensors, fixed noise; the two sides alternate window by window; HIP events around each window of
`--iters` calls after a warm-up, median of `--repeats` windows.  Also: kernel launches per call on each
side (torch.profiler's device events), and the three pass kernels alone at the 512 x 512 level against
their algorithmic bytes.  Prints one JSON line.

    python tools/bench_refiner.py [--iters 20] [--repeats 7] [--only decoder:small:1]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def stats(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def timed_pair(fa, fb, iters, repeats, warmup=5):
    """Medians (and ranges) of fa and fb, their windows alternating."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(repeats):
        a.append(window(fa, iters))
        b.append(window(fb, iters))
    return stats(a), stats(b)


def launches(fn):
    """Device kernels of one call (None where the profiler gives no device events)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception:  # noqa: BLE001
        return None


def pass_kernels(B, iters, repeats, dev):
    """The three pass kernels at the small decoder's 512 x 512 level (32 -> 16 channels, out_dim 3)."""
    from guava_renderer_amd import refiner
    g = torch.Generator(device=dev).manual_seed(3)
    r = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
    x256, s32 = r(B, 32, 256, 256), r(B, 32)
    y, d16, bias16, nw = r(B, 16, 512, 512), r(B, 16).abs() + 0.1, r(16), r(1)
    noise, scale, shift = r(B, 1, 512, 512), r(B, 16, 512, 512), r(B, 16, 512, 512)
    w, s16, b3, skip = r(3, 16), r(B, 16), r(3), r(B, 3, 256, 256)
    px = 512 * 512
    cases = (
        ("upmod", lambda: refiner.style_upmod(x256, s32, up=True), 4 * B * 32 * (px // 4 + px)),
        ("epilogue", lambda: refiner.style_epilogue(y, d16, bias16, noise, nw, scale, shift, out=y),
         4 * B * (4 * 16 + 1) * px),
        ("torgb", lambda: refiner.style_torgb(y, w, s16, b3, skip, skip_up=True, sigmoid=True),
         4 * B * (16 * px + 3 * px // 4 + 3 * px)),
    )
    out = []
    for name, fn, nbytes in cases:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = stats([window(fn, iters * 5) for _ in range(repeats)])
        out.append({"kernel": name, "B": B, "us": us, "algorithmic_bytes": nbytes,
                    "GBs": round(nbytes / us["median"] / 1e3, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--only", default=None, help="one case, e.g. decoder:small:1, runner:small:6 or kernels")
    a = ap.parse_args()
    import refiner_ref
    from guava_renderer_amd.refiner import StyleUNetRunner
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = "cuda:0"
    out = {"workload": "StyleUNet refiner decoder", "out_size": a.size, "num_style_feat": 512, "num_mlp": 8,
           "channel_scale": 1, "iters": a.iters, "repeats": a.repeats, "cases": [], "pass_kernels": []}
    nets = {}
    for small in (True, False):
        torch.manual_seed(1 if small else 2)
        net = refiner_ref.StyleUNetRef(in_size=a.size, out_size=a.size, in_dim=32, out_dim=3, num_style_feat=512,
                                       num_mlp=8, activation=True, channel_scale=1, small=small).eval()
        nets[small] = refiner_ref.randomize_noise_params(net, 4).to(dev).requires_grad_(False)
    with torch.no_grad():
        for what, small, B in (("decoder", True, 1), ("decoder", True, 6), ("decoder", False, 1),
                               ("runner", True, 1), ("runner", True, 6)):
            name = f"{what}:{'small' if small else 'full'}:{B}"
            if a.only and a.only != name:
                continue
            net = nets[small]
            run = StyleUNetRunner(net)
            g = torch.Generator(device=dev).manual_seed(5)
            feat = torch.nn.functional.leaky_relu(torch.randn((B, 16, a.size, a.size), device=dev, generator=g), 0.2)
            noise = [torch.randn((B, 1, n, n), device=dev, generator=g) for n in net.stylegan_decoder.noise_sizes()]
            if what == "runner":
                ours, ref = (lambda: run.rest(feat, noise=noise)), (lambda: net.rest(feat, noise))
            else:
                style = torch.randn((B, 512), device=dev, generator=g)
                ch = refiner_ref.channels(1)
                cond = [torch.randn((B, ch[2 ** i], 2 ** i, 2 ** i), device=dev, generator=g) * 0.5 + m
                        for i in range(3, net.log_size + 1) for m in (1.0, 0.0)]
                ours = lambda: run.decoder.forward(style, cond, noise=noise, sigmoid=True)  # noqa: E731
                ref = lambda: torch.sigmoid(net.stylegan_decoder(style, cond, noise))  # noqa: E731
            diff = float((ours() - ref()).abs().max())
            t_o, t_r = timed_pair(ours, ref, a.iters, a.repeats)
            case = {"case": name, "max_abs_diff_vs_torch": diff, "fused_us": t_o, "torch_us": t_r,
                    "speedup": round(t_r["median"] / t_o["median"], 2)}
            print(json.dumps(case), file=sys.stderr, flush=True)  # (the timings, should the profiler stall)
            case["launches"] = {"fused": launches(ours), "torch": launches(ref)}
            out["cases"].append(case)
        if not a.only or a.only == "kernels":
            for B in (1, 6):
                out["pass_kernels"] += pass_kernels(B, a.iters, a.repeats, dev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
