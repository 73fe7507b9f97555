"""Mesh visibility rasterizer timings: the template mesh (V = 10,475, F = 20,908)
at 512 x 512 for B = 1, 6, 32 under the canonical camera orbit, and the distance-4 close-up at B = 6.
HIP events around the whole call (five launches), median of `--repeats` windows of `--iters` calls
after a warm-up.  For scale only, the Gaussian rasterizer's single-frame forward (drop-in call,
P = 100,000 avatar cloud) at the same image size.  Prints one JSON line.

    python tools/bench_mesh_raster.py [--iters 200] [--repeats 7] [--only orbit:32]
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


def timed(fn, iters, repeats, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)  # us per call
    return statistics.median(out), min(out), max(out)


def posed(verts, B, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([verts + rng.normal(0, 0.002, 3).astype(np.float32) for _ in range(B)]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--only", default=None, help="one case, e.g. orbit:32 or closeup:6 (for a profiler run)")
    a = ap.parse_args()
    from guava_renderer_amd import avatar, camera
    from guava_renderer_amd.mesh_raster import MeshRasterizer
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = "cuda:0"
    verts, faces, _ = avatar.template_mesh()
    V, F, S = verts.shape[0], faces.shape[0], a.size
    out = {"workload": "mesh visibility rasterizer, SMPL-X template", "V": V, "F": F, "W": S, "H": S,
           "iters": a.iters, "repeats": a.repeats, "cases": []}
    for name, B, dist in (("orbit", 1, 22.0), ("orbit", 6, 22.0), ("orbit", 32, 22.0), ("closeup", 6, 4.0)):
        if a.only and a.only != f"{name}:{B}":
            continue
        w2c = np.stack([camera.look_at_w2c(2 * np.pi * b / B, 0.1, dist) for b in range(B)])
        dv, dm = torch.from_numpy(posed(verts, B)).to(dev), torch.from_numpy(w2c).to(dev)
        fov = torch.full((B,), 1.0 / 24.0, device=dev)
        r = MeshRasterizer(faces, S, S, B, dev)
        med, lo, hi = timed(lambda: r(dv, dm, fov, fov), a.iters, a.repeats)
        st = r.stats()
        read = B * 12 * V + 12 * F + B * 64
        written = B * S * S * (8 + 4 + 4 + 12)
        out["cases"].append({"case": name, "B": B, "distance": dist, "us_per_call": round(med, 2),
                             "us_per_call_min": round(lo, 2), "us_per_call_max": round(hi, 2),
                             "us_per_frame": round(med / B, 2), **st,
                             "algorithmic_bytes_read": read, "algorithmic_bytes_written": written,
                             "GBs_algorithmic": round((read + written) / (med * 1e-6) / 1e9, 1)})
    if a.only:
        print(json.dumps(out), flush=True)
        return
    # for scale: the Gaussian rasterizer's single-frame forward at the same size
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import make_scene, torch_inputs
    from diff_gaussian_rasterization_32 import GaussianRasterizationSettings, GaussianRasterizer_32
    d = make_scene("avatar", 100000, S, S, seed=0)
    t = torch_inputs(d, device=dev)
    s = GaussianRasterizationSettings(
        image_height=S, image_width=S, tanfovx=d["tanfovx"], tanfovy=d["tanfovy"], bg=t["bg"], scale_modifier=1.0,
        viewmatrix=t["viewmatrix"], projmatrix=t["projmatrix"], sh_degree=0, campos=t["campos"], prefiltered=False,
        debug=False, antialiasing=False)
    rast = GaussianRasterizer_32(s)
    m2 = torch.zeros_like(t["means3D"])
    with torch.no_grad():
        med, lo, hi = timed(lambda: rast(means3D=t["means3D"], means2D=m2, opacities=t["opacities"],
                                         colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"]),
                            a.iters, a.repeats)
    out["gaussian_forward_single_frame_us"] = {"P": 100000, "median": round(med, 1), "min": round(lo, 1),
                                               "max": round(hi, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
