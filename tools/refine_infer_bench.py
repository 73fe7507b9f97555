"""Timings of inference through the refiner head (conv_body_first 32 -> 16 + leaky ReLU, head 16/4)
at the C2 shape: the 100k-Gaussian avatar at 512 x 512.

  --mode b1       one frame per call, BatchRasterizer(1, ...):
                    fused     forward(refine=head, forward_only=True) -- the head in the render epilogue;
                    unfused   forward(forward_only=True) writing 32 channels, then torch conv2d 1x1 +
                              leaky_relu_ on them.
  --mode fused32  32 frames per call of the avatar pipeline with the head:
                    two_step  AvatarPipeline.render(refine=head): deform, then the refine forward;
                    fused     AvatarPipeline.render(fused=True, refine=head): the Gaussian assembly
                              inside the projection kernel.

Everything of a mode runs from one build in one session, in alternating blocks of `--reps` calls timed
with device events; one JSON line per mode with every block's per-call microseconds.  The library's
own answer to which compositing kernel the call takes (gsr_render_variant) is printed where the
build has it."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from guava_renderer_amd import _lib, avatar, camera, scenes  # noqa: E402
from guava_renderer_amd.batch import BatchRasterizer, RefineHead  # noqa: E402

DEV = torch.device("cuda:0")
P, W, C = 100000, 512, 32
N_OUT, KEEP, SLOPE = 16, 4, 0.2


def t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def timed_blocks(fns, reps, rounds, warmup):
    """Alternating blocks: per function the per-call microseconds of each block."""
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
            out[k].append(round(1e3 * a.elapsed_time(b) / reps, 2))
    return out


def make_head():
    rng = np.random.default_rng(5)  # random-init conv_body_first (nn.Conv2d(32, 16, 1))
    w = t(rng.uniform(-0.18, 0.18, (N_OUT, C)).astype(np.float32))
    b = t(rng.uniform(-0.18, 0.18, N_OUT).astype(np.float32))
    return RefineHead(w, b, negative_slope=SLOPE, keep_channels=KEEP), w, b


def variant(B, refine):
    fn = getattr(_lib, "render_variant", None)
    return fn(B, _lib.FORWARD_ONLY, refine) if fn else None


def mode_b1(a):
    sc = scenes.avatar_cloud(P, seed=0)
    cam = camera.camera(W, W)
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    args += [t(cam["viewmatrix"].reshape(1, 16)), t(cam["projmatrix"].reshape(1, 16)),
             t(np.array([[cam["tanfovx"], cam["tanfovy"]]], np.float32)), torch.zeros((1, C), device=DEV)]
    n = args[0].shape[0]
    head, w, b = make_head()
    r = BatchRasterizer(1, n, W, W, R_capacity=24 * n, device=DEV)
    w4 = w.reshape(N_OUT, C, 1, 1)

    def fused():
        r.forward(*args, refine=head, forward_only=True)

    def unfused():
        col, _, _ = r.forward(*args, forward_only=True)
        return F.leaky_relu_(F.conv2d(col, w4, b), SLOPE)

    # the two agree to f32 reassociation of the 32-term contraction
    fused()
    got, ref = head.out.clone(), unfused()
    torch.cuda.synchronize()
    assert not r.status()[1]
    err = float((got - ref).abs().max())
    assert err < 1e-3, err
    blocks = timed_blocks({"fused": fused, "unfused": unfused}, a.reps, a.rounds, a.warmup)
    print(json.dumps({"mode": "b1", "P": n, "W": W, "head": [N_OUT, KEEP], "us_per_frame": blocks,
                      "variant_with_head": variant(1, True), "variant_without": variant(1, False),
                      "max_abs_diff": err}))


def mode_fused32(a):
    from guava_renderer_amd.pipeline import AvatarPipeline
    B = 32
    body, flame, extra = avatar.ehm_assets(seed=0)
    verts, faces, tex = avatar.template_mesh()
    g = avatar.gaussians(verts, faces, tex, P=P, seed=0)
    bp, fp = avatar.ehm_params(B, seed=1000)
    bpt, fpt = {k: t(v) for k, v in bp.items()}, {k: t(v) for k, v in fp.items()}
    cams = scenes.frame_cameras(B, W, W, seed=1000)
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    pipe = AvatarPipeline(body, flame, extra, g, B, W, W, R_capacity=24 * P * B, device=DEV)
    head, _, _ = make_head()

    def two_step():
        pipe.render(bpt, fpt, views, projs, tanf, refine=head)

    def fused():
        pipe.render(bpt, fpt, views, projs, tanf, refine=head, fused=True)

    two_step()
    ref = (head.out.clone(), pipe.rast.out_color[:, :KEEP].clone())
    fused()
    torch.cuda.synchronize()
    assert not pipe.rast.status()[1]
    assert torch.equal(ref[0], head.out) and torch.equal(ref[1], pipe.rast.out_color[:, :KEEP])
    blocks = timed_blocks({"two_step": two_step, "fused": fused}, a.reps, a.rounds, a.warmup)
    print(json.dumps({"mode": "fused32", "P": pipe.P, "W": W, "B": B, "us_per_call": blocks,
                      "variant": variant(B, True)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="b1", choices=["b1", "fused32"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    {"b1": mode_b1, "fused32": mode_fused32}[a.mode](a)
