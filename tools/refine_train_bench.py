"""Timings of training through the refiner head (conv_body_first 32 -> 16 + leaky ReLU) at config 4's
shape: B = 6 views of the 100k-Gaussian C2 cloud at 512 x 512, head 16/4.  Each item is forward + head
+ backward down to the gradients of the shared attributes, the weight and the bias:

  fused      forward(refine=head), then backward_refine(shared=True): the 32-channel feature image is
             never written, the head's backward is the two kernels of refine_bwd.hip;
  unfused    what a caller composes without it: the plain forward writing 32 channels, torch conv2d +
             leaky_relu, torch autograd back to the 32-channel image gradient (and the conv's weight
             and bias gradients), then backward(shared=True).

    python tools/refine_train_bench.py --mode time
    rocprofv3 --kernel-trace --stats -- python tools/refine_train_bench.py --mode profile

Both run from the same build in one session, in alternating blocks; the gradients of the two are
compared before timing (they differ by f32 reassociation, and at the few pixels whose pre-activation
rounds to the other side of zero in one of the two forwards).  Prints one JSON line per measurement;
times are device-event times of blocks of `--reps` calls."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from guava_renderer_amd import scenes  # noqa: E402
from guava_renderer_amd.batch import BatchRasterizer, RefineHead  # noqa: E402

DEV = torch.device("cuda:0")
P, W = 100000, 512
N_OUT, KEEP, SLOPE = 16, 4, 0.2
NAMES = ("means3D", "colors", "opacity", "scales", "rotations", "weight", "bias")


def t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def timed_blocks(fns, reps, rounds, warmup):
    """Alternating blocks: per function the list of per-call milliseconds of each block."""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return out


def setup(B):
    scene = scenes.avatar_cloud(P, seed=0)
    cams = scenes.frame_cameras(B, W, W, seed=1000)
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    rng = np.random.default_rng(5)
    bgs = t(rng.uniform(0, 1, (B, 32)).astype(np.float32))
    args = tuple(t(scene[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")) + (views, projs, tanf,
                                                                                                    bgs)
    probe = BatchRasterizer(B, P, W, W, R_capacity=24 * P * B, device=DEV)
    probe.forward(*args)
    R, ovf = probe.status()
    assert not ovf
    del probe
    torch.cuda.empty_cache()
    rast = BatchRasterizer(B, P, W, W, R_capacity=int(R * 1.25) + 1024, device=DEV)
    w = t(rng.normal(0, 0.2, (N_OUT, 32)).astype(np.float32))
    b = t(rng.normal(0, 0.1, N_OUT).astype(np.float32))
    head = RefineHead(w, b, SLOPE, KEEP)
    gen = torch.Generator(device=DEV).manual_seed(9)
    dLr = torch.randn((B, N_OUT, W, W), device=DEV, generator=gen)
    dLraw = torch.randn((B, KEEP, W, W), device=DEV, generator=gen)

    def fused():
        rast.forward(*args, refine=head)
        return rast.backward_refine(head, *args, dLr, dL_draw=dLraw, shared=True)

    w4 = w.reshape(N_OUT, 32, 1, 1)

    def unfused():
        col = rast.forward(*args)[0]
        x = col.detach().requires_grad_(True)
        wl, bl = w4.detach().requires_grad_(True), b.detach().requires_grad_(True)
        y = F.leaky_relu(F.conv2d(x, wl, bl), SLOPE)
        dx, dw, db = torch.autograd.grad(y, (x, wl, bl), dLr)
        dx[:, :KEEP] += dLraw
        g = rast.backward(*args, dx, shared=True)
        g["weight"], g["bias"] = dw.reshape(N_OUT, 32), db
        return g
    return rast, {"fused": fused, "unfused": unfused}


def compare(fns):
    f, u = fns["fused"](), fns["unfused"]()
    torch.cuda.synchronize()
    errs = {}
    for k in NAMES:
        errs[k] = float((f[k] - u[k].reshape(f[k].shape)).abs().max() / u[k].abs().max().clamp_min(1e-30))
        assert errs[k] <= 1e-3, (k, errs[k])
    return errs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "profile"), required=True)
    ap.add_argument("--B", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rast, fns = setup(a.B)
    errs = compare(fns)
    print(json.dumps({"measurement": "fused vs unfused gradients, max error of scale", "B": a.B, **errs}), flush=True)
    if a.mode == "time":
        blocks = timed_blocks(fns, a.reps, a.rounds, a.warmup)
        row = {"measurement": "forward + head + backward", "B": a.B, "P": P, "W": W, "n_out": N_OUT, "keep": KEEP}
        for k, v in blocks.items():
            row[k + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
        print(json.dumps(row), flush=True)
    else:
        for _ in range(a.warmup + a.reps):
            fns["fused"]()
        torch.cuda.synchronize()
        print(json.dumps({"measurement": "profile run", "B": a.B, "fused_calls": a.warmup + a.reps + 1}), flush=True)
    assert not rast.status()[1]
