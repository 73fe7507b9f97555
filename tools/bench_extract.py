"""UV Gaussian extraction timings: decoder maps -> Gaussian tables at U = 512,
C = 32, with the mask density of the template's texels-per-face counts, for B = 1 and B = 6 (config 4's
batch per GPU), in both layouts --
  raw    planar raw heads [B,k,U,U]: activations + permute + gather + RGB sigmoid fused
  rows   the decoder's activated [B,U,U,k] maps: gather + RGB sigmoid
  prune  B = 1, raw: the above plus opacity > 0.001 pruning with binding_face / face_bary
-- forward alone (no_grad) and forward plus backward (autograd on the five maps), each against the torch
chain of the reference's lines (feature_decoder.py:120-135, ubody_gaussian.py:150-156, :186-187,
:229-243) on the same GPU tensors in the same process.  The chain's boolean gathers each run a nonzero
and make the host wait for the device: 5 per forward (7 with binding_face / face_bary, which the fused
path builds once at construction), 7 more when pruning; the fused extract() has none, extract_pruned()
one (the count).  The two sides alternate window by window; HIP events around each window of `--iters`
calls after a warm-up, median of `--repeats` windows.  Prints one JSON line.

    python tools/bench_extract.py [--iters 50] [--repeats 7] [--only raw:6]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("colors", "opacities", "scales", "rotations", "local_pos")


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


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
    s = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}  # noqa: E731
    return s(a), s(b)


def torch_chain(maps, uv_mask_flat, raw, binding=None, threshold=None):
    """The reference's glue on the five maps (a dict); binding = (f_idx [T,1], f_bary [T,3]) or None."""
    r = dict(maps)
    if raw:
        r["opacities"] = torch.sigmoid(r["opacities"])
        r["scales"] = torch.exp(r["scales"])
        r["rotations"] = torch.nn.functional.normalize(r["rotations"])
        for k in r:
            r[k] = r[k].permute(0, 2, 3, 1).contiguous()
    B = r["colors"].shape[0]
    out = {k: v.reshape(B, uv_mask_flat.shape[0], -1)[:, uv_mask_flat, :] for k, v in r.items()}
    if binding is not None:
        out["binding_face"] = binding[0].clone().reshape(1, uv_mask_flat.shape[0], -1)[:, uv_mask_flat, :]
        out["face_bary"] = binding[1].clone().reshape(1, uv_mask_flat.shape[0], -1)[:, uv_mask_flat, :]
    out["colors"] = torch.cat([torch.sigmoid(out["colors"][..., :3]), out["colors"][..., 3:]], -1)
    if threshold is not None:
        m = (out["opacities"] > threshold).squeeze(-1)[0].bool()
        for k in KEYS:
            out[k] = out[k][:, m]
        out["binding_face"] = out["binding_face"][0].squeeze(-1)[m]
        out["face_bary"] = out["face_bary"][0][m]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--colors", type=int, default=32)
    ap.add_argument("--only", default=None, help="one case, e.g. raw:6, rows:1 or prune:1")
    a = ap.parse_args()
    from guava_renderer_amd import avatar
    from guava_renderer_amd.gaussian_extract import UVGaussianExtractor
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = "cuda:0"
    _, faces, texel_count = avatar.template_mesh()
    U, C, F = a.size, a.colors, faces.shape[0]
    T = U * U
    rng = np.random.default_rng(0)
    n_placed = int(min(int(np.sum(texel_count)) * T // (512 * 512), T))
    placed = np.sort(rng.choice(T, n_placed, replace=False))
    mask = np.zeros(T, np.float32)
    mask[placed] = 1.0
    f_idx = rng.integers(0, F, T).astype(np.int64)
    f_bary = rng.dirichlet((1.0, 1.0, 1.0), T).astype(np.float32)
    ex = UVGaussianExtractor(mask.reshape(U, U), f_idx.reshape(U, U), f_bary.reshape(U, U, 3), color_dim=C, device=dev)
    N = ex.N
    flat = torch.from_numpy(mask != 0).to(dev)
    t_idx, t_bary = torch.from_numpy(f_idx).to(dev).reshape(T, 1), torch.from_numpy(f_bary).to(dev)
    widths = (C, 1, 3, 4, 3)
    out = {"workload": "UV Gaussian extraction", "U": U, "C": C, "N": N, "mask_density": round(N / T, 4),
           "iters": a.iters, "repeats": a.repeats, "cases": []}
    for name, B in (("raw", 1), ("raw", 6), ("rows", 1), ("rows", 6), ("prune", 1)):
        if a.only and a.only != f"{name}:{B}":
            continue
        raw = name != "rows"
        g = torch.Generator(device=dev).manual_seed(1)
        heads = {k: torch.randn((B, w, U, U), device=dev, generator=g) * s + m for k, w, (m, s) in
                 zip(KEYS, widths, ((0, 1.5), (0, 3.0), (-4, 1.0), (0, 1.0), (0, 0.01)))}
        if raw:
            maps = heads
        else:
            maps = {k: v.permute(0, 2, 3, 1).contiguous() for k, v in
                    dict(heads, opacities=torch.sigmoid(heads["opacities"]), scales=torch.exp(heads["scales"]),
                         rotations=torch.nn.functional.normalize(heads["rotations"])).items()}
        leaves = {k: v.clone().requires_grad_(True) for k, v in maps.items()}
        douts = [torch.randn((B, N, w), device=dev, generator=g) for w in widths]
        prune = name == "prune"

        def ours(m):
            args = [m[k] for k in KEYS]
            return ex.extract_pruned(*args, raw=raw) if prune else ex.extract(*args, raw=raw)

        def ref(m):
            return torch_chain(m, flat, raw, (t_idx, t_bary) if prune else None, 0.001 if prune else None)

        with torch.no_grad():
            o, r = ours(maps), ref(maps)
        assert all(o[k].shape == r[k].shape for k in KEYS)
        err = max(float((o[k] - r[k]).abs().max()) for k in KEYS)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(maps)
            return run

        def fwd_bwd(fn):
            def run():
                for l in leaves.values():
                    l.grad = None
                res = fn(leaves)
                torch.autograd.backward([res[k] for k in KEYS], douts)
            return run
        f_o, f_t = timed_pair(fwd(ours), fwd(ref), a.iters, a.repeats)
        case = {"case": name, "B": B, "max_abs_diff_vs_torch": err, "rows_out": int(o["colors"].shape[1]),
                "forward_us": f_o, "torch_forward_us": f_t, "forward_speedup": round(f_t["median"] / f_o["median"], 2),
                "host_waits": {"fused": 1 if prune else 0, "torch": 14 if prune else 5}}
        min_bytes = 4 * (C + 11) * N * B  # each way
        if prune:
            min_bytes += 4 * T  # the count pass reads the opacity plane
        case["min_bytes_each_way"] = min_bytes
        # read + written by the fused forward: kept planes / rows in, rows out, the mask and the scan
        moved = 2 * min_bytes + T + 4 * (T // 64 + 1)
        case["forward_GBs_at_minimum"] = round(moved / f_o["median"] / 1e3, 1)
        if not prune:
            b_o, b_t = timed_pair(fwd_bwd(ours), fwd_bwd(ref), a.iters, a.repeats)
            bwd_us = max(b_o["median"] - f_o["median"], 1e-3)
            # backward: table gradients in, the 11 (raw) or 3 activated planes re-read, every map element out
            bwd_bytes = min_bytes + 4 * B * ((11 if raw else 3) * N + (C + 11) * T)
            case.update({"forward_backward_us": b_o, "torch_forward_backward_us": b_t,
                         "forward_backward_speedup": round(b_t["median"] / b_o["median"], 2),
                         "backward_us_by_difference": round(bwd_us, 1), "backward_bytes": bwd_bytes,
                         "backward_GBs": round(bwd_bytes / bwd_us / 1e3, 1)})
        out["cases"].append(case)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
