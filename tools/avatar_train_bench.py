"""Timings of the posed-avatar training path at the C2 avatar (100k Gaussians, 512 x 512):

  backward   BatchRasterizer.backward_deformed (gsr_backward_batch_deformed) against the composed
             path with the existing entry points -- backward(shared=False), then
             gsr_deform_gaussians_backward, then the frame sums of the colour and opacity gradients
             -- on the same forward, in alternating blocks;
  step       train.AvatarTrainer.step against train.SplatTrainer.step (the parent's training step,
             config 4) in alternating blocks: the difference is the price of posing;
  profile    a few AvatarTrainer steps and standalone assembly backwards, for a
             `rocprofv3 --kernel-trace --stats -- python tools/avatar_train_bench.py --mode profile`
             run (kernel times of k_preprocess_bwd_deformed and k_deform_gaussians_bwd);
  --guava-loss   (instead of --mode) GUAVA's mask / head and hand crop / regulariser loss terms at
             config 4's shape (B=6, 512 x 512, crops resampled to 256): the loss stage, fused kernels
             against the torch-autograd chain of the same terms, and the whole step with and without
             the terms.

    python tools/avatar_train_bench.py --mode backward --B 6
Prints one JSON line per measurement.  Times are device-event times of blocks of `--reps` calls."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from guava_renderer_amd import _lib, avatar, deform, scenes  # noqa: E402
from guava_renderer_amd.batch import BatchRasterizer  # noqa: E402
from guava_renderer_amd.train import AvatarTrainer, SplatTrainer  # noqa: E402

DEV = torch.device("cuda:0")
P, W = 100000, 512


def t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def cameras(B):
    cams = scenes.frame_cameras(B, W, W, seed=1000)
    return (t(np.stack([c["viewmatrix"].reshape(16) for c in cams])),
            t(np.stack([c["projmatrix"].reshape(16) for c in cams])),
            t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32)))


def posed_avatar(B):
    """(vertex assets, UV assets, faces, verts [B,V,3], vert_transforms [B,V,4,4]) of bench.py's avatar."""
    body, flame, extra = avatar.ehm_assets(seed=0)
    verts, faces, tex = avatar.template_mesh()
    g = avatar.gaussians(verts, faces, tex, P=P, seed=0)
    bp, fp = avatar.ehm_params(B, seed=1000)
    ehm = deform.EHMDeformer(body, flame, extra["smplx2flame_ind"], extra["l_eyelid"], extra["r_eyelid"], device=DEV)
    e = ehm({k: t(v) for k, v in bp.items()}, {k: t(v) for k, v in fp.items()})
    V = body["v_template"].shape[0]
    va = {"rotations": t(g["vtx_rotations"]), "scales": t(g["vtx_scales"]), "opacities": t(g["opacities"][:V]),
          "colors": t(g["colors"][:V])}
    ua = {"rotations": t(g["uv_rotations"]), "scales": t(g["uv_scales"]), "opacities": t(g["opacities"][V:]),
          "colors": t(g["colors"][V:]), "local_pos": t(g["local_xyz"]), "binding_face": t(g["binding_face"]),
          "face_bary": t(g["face_bary"])}
    return va, ua, t(extra["faces"]), e["vertices"].clone(), e["ver_transform_mat"].clone()


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


def report(what, B, blocks):
    row = {"measurement": what, "B": B, "P": P, "W": W}
    for k, v in blocks.items():
        row[k + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(json.dumps(row), flush=True)


def composed_backward(rast, dfm, verts, T, d, cam, dL, dinv, stream):
    per = rast.backward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], *cam, dL, dinv, shared=False)
    B = verts.shape[0]
    di, keep = deform.deform_inputs(B, verts, T, dfm.faces, dfm.bind, dfm.bary,
                                    (dfm.v_rot, dfm.v_scale, dfm.u_local, dfm.u_rot, dfm.u_scale), dfm.bad)
    outs = [torch.empty_like(a) for a in (dfm.v_rot, dfm.v_scale, dfm.u_local, dfm.u_rot, dfm.u_scale)]
    dgr = _lib.DeformGrads(*[o.data_ptr() for o in outs])
    _lib.check(rast.L.gsr_deform_gaussians_backward(B, ctypes.byref(di), per["means3D"].data_ptr(),
                                                    per["rotations"].data_ptr(), per["scales"].data_ptr(),
                                                    ctypes.byref(dgr), stream), "gsr_deform_gaussians_backward")
    return outs, per["colors"].sum(0), per["opacity"].sum(0)


def bench_backward(B, a):
    va, ua, faces, verts, T = posed_avatar(B)
    dfm = deform.GaussianDeformer(va, ua, faces, apply_rgb_sigmoid=False)
    views, projs, tanf = cameras(B)
    cam = (views, projs, tanf, torch.zeros((B, 32), device=DEV))
    probe = BatchRasterizer(B, P, W, W, R_capacity=24 * P * B, device=DEV)
    d = dfm(verts, T)
    probe.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], *cam)
    R, ovf = probe.status()
    assert not ovf
    del probe
    torch.cuda.empty_cache()
    rast = BatchRasterizer(B, P, W, W, R_capacity=int(R * 1.25) + 1024, device=DEV)
    rast.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], *cam)
    gen = torch.Generator(device=DEV).manual_seed(9)
    dL = torch.randn((B, 32, W, W), device=DEV, generator=gen)
    dinv = torch.randn((B, W, W), device=DEV, generator=gen)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    fns = {"fused": lambda: rast.backward_deformed(dfm, verts, T, d, dfm.colors, dfm.opacity, *cam, dL, dinv),
           "composed": lambda: composed_backward(rast, dfm, verts, T, d, cam, dL, dinv, stream)}
    # the two paths compute the same gradients (render_bwd's atomics: last bits)
    f, (c_outs, c_col, c_op) = fns["fused"](), fns["composed"]()
    torch.cuda.synchronize()
    for name, ref in zip(("vtx_rotations", "vtx_scales", "local_pos", "uv_rotations", "uv_scales", "colors", "opacity"),
                         c_outs + [c_col, c_op]):
        err = float((f[name] - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        assert err <= 1e-4, (name, err)
    report("backward_deformed vs composed", B, timed_blocks(fns, a.reps, a.rounds, a.warmup))


def avatar_trainer(B, reg=None):
    va, ua, faces, verts, T = posed_avatar(B)
    views, projs, tanf = cameras(B)
    dfm = deform.GaussianDeformer(va, ua, faces, apply_rgb_sigmoid=False)
    probe = BatchRasterizer(B, P, W, W, R_capacity=24 * P * B, device=DEV)
    d = dfm(verts, T)
    probe.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], views, projs, tanf,
                  torch.zeros((B, 32), device=DEV))
    R, ovf = probe.status()
    assert not ovf
    del probe, d
    torch.cuda.empty_cache()
    tr = AvatarTrainer(va, ua, faces, B, W, W, R_capacity=int(R * 2) + 1024, device=DEV, lr=1e-5,
                       apply_rgb_sigmoid=False, reg=reg)
    target = torch.rand((B, 3, W, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    return tr, lambda: tr.step(verts, T, views, projs, tanf, target)


def splat_trainer(B):
    """bench.py's config-4 trainer."""
    scene = scenes.avatar_cloud(P, seed=0)
    views, projs, tanf = cameras(B)
    params = {k: t(scene[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    probe = BatchRasterizer(B, P, W, W, R_capacity=24 * P * B, device=DEV)
    probe.forward(params["means3D"], params["colors"], params["opacities"], params["scales"], params["rotations"],
                  views, projs, tanf, torch.zeros((B, 32), device=DEV))
    R, ovf = probe.status()
    assert not ovf
    del probe
    torch.cuda.empty_cache()
    tr = SplatTrainer(params, B, W, W, R_capacity=int(R * 2) + 1024, device=DEV, lr=1e-5)
    target = torch.rand((B, 3, W, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    return tr, lambda: tr.step(views, projs, tanf, target)


def bench_step(B, a):
    at, a_step = avatar_trainer(B)
    st, s_step = splat_trainer(B)
    report("AvatarTrainer.step vs SplatTrainer.step", B,
           timed_blocks({"avatar_step": a_step, "splat_step": s_step}, a.reps, a.rounds, a.warmup))
    assert at.skipped_steps == 0 and st.skipped_steps == 0


def profile(B, a):
    tr, step = avatar_trainer(B)
    dfm = tr.deformer
    va, ua, faces, verts, T = posed_avatar(B)
    Pn = dfm.V + dfm.N
    gen = torch.Generator(device=DEV).manual_seed(4)
    ups = [torch.randn((B, Pn, k), device=DEV, generator=gen) for k in (3, 4, 3)]
    attrs = (dfm.v_rot.detach(), dfm.v_scale.detach(), dfm.u_local.detach(), dfm.u_rot.detach(), dfm.u_scale.detach())
    di, keep = deform.deform_inputs(B, verts, T, dfm.faces, dfm.bind, dfm.bary, attrs, dfm.bad)
    outs = [torch.empty_like(x) for x in attrs]
    dgr = _lib.DeformGrads(*[o.data_ptr() for o in outs])
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for _ in range(a.warmup + a.reps):
        step()
        _lib.check(_lib.load().gsr_deform_gaussians_backward(B, ctypes.byref(di), ups[0].data_ptr(),
                                                             ups[1].data_ptr(), ups[2].data_ptr(),
                                                             ctypes.byref(dgr), stream), "deform backward")
    torch.cuda.synchronize()
    assert tr.skipped_steps == 0
    print(json.dumps({"measurement": "profile run", "B": B, "steps": a.warmup + a.reps}), flush=True)


def guava_batch(B):
    """The fields of a GUAVA batch beside the poses: image, a soft foreground mask (an ellipse with a
    feathered edge) and the three boxes of plausible size, jittered per frame (int64 [3,B,4], as the
    reference's loader gives them): head ~150 x 150, each hand ~60 x 60."""
    gen = torch.Generator(device=DEV).manual_seed(0)
    target = torch.rand((B, 3, W, W), device=DEV, generator=gen)
    y, x = torch.meshgrid(torch.arange(W, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    r = (((x - W / 2) / (0.28 * W)) ** 2 + ((y - W / 2) / (0.45 * W)) ** 2).sqrt()
    mask = ((1.15 - r) / 0.3).clamp(0, 1).expand(B, 1, W, W).contiguous()
    rng = np.random.default_rng(0)
    boxes = np.zeros((3, B, 4), np.int64)
    for g, (cx, cy, size) in enumerate(((256, 110, 150), (130, 330, 60), (380, 340, 60))):
        for b in range(B):
            jx, jy, js = rng.integers(-12, 13), rng.integers(-12, 13), rng.integers(-6, 7)
            half = (size + js) // 2
            boxes[g, b] = (cx + jx - half, cx + jx + half, cy + jy - half, cy + jy + half)
    return target, mask, torch.from_numpy(boxes)


def bench_guava_loss(B, a):
    """--guava-loss: (1) the loss stage alone on one rendered batch -- the fused path
    (gsr_guava_loss_forward / _backward + fused_ssim) against the torch-autograd chain of the same
    terms (SplatTrainer.loss: a Python loop of slices, F.interpolate, cat, with the same fused_ssim)
    -- and (2) AvatarTrainer.step with and without the mask, crop and regulariser terms."""
    target, mask, boxes = guava_batch(B)
    tr, plain_step = avatar_trainer(B)
    tg, _ = avatar_trainer(B, reg=AvatarTrainer.GUAVA_REG)
    va, ua, faces, verts, T = posed_avatar(B)
    views, projs, tanf = cameras(B)
    boxes_dev = boxes.to(DEV)
    tg.gradients(verts, T, views, projs, tanf, target)
    col = tg.rast.out_color.detach().clone()
    torch.cuda.synchronize()

    def fused():
        return tg._guava_loss_and_image_grad(col, target, mask, boxes_dev, True)

    def chain():
        feat = col.detach().requires_grad_(True)
        loss = tg.loss(feat, target, mask=mask, boxes=boxes, mask_refined=True)  # (boxes on the host: no sync)
        loss.backward()
        return loss.detach(), feat.grad

    (lf, gf), (lc, gc) = fused(), chain()
    torch.cuda.synchronize()
    # (two float32 evaluations of W . feat may put a difference on either side of L1's kink: a
    # handful of elements may differ by a whole sign, so the agreement is a fraction of elements)
    err = float(((gf - gc).abs() > 1e-3 * gc.abs().max()).float().mean())
    assert abs(lf.item() - lc.item()) <= 1e-4 * abs(lc.item()) and err <= 1e-4, (lf.item(), lc.item(), err)
    row = {"loss_fused": lf.item(), "loss_torch_chain": lc.item(), "grad_fraction_off_by_1e-3_of_max": err}
    print(json.dumps({"measurement": "guava loss agreement", **row}), flush=True)
    report("guava loss stage: fused vs torch chain", B,
           timed_blocks({"fused_loss": fused, "torch_chain_loss": chain}, a.reps, a.rounds, a.warmup))

    def guava_step():
        return tg.step(verts, T, views, projs, tanf, target, mask=mask, boxes=boxes_dev, mask_refined=True)
    report("AvatarTrainer.step: guava loss terms vs whole-frame loss", B,
           timed_blocks({"guava_step": guava_step, "plain_step": plain_step}, a.reps, a.rounds, a.warmup))
    assert tr.skipped_steps == 0 and tg.skipped_steps == 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("backward", "step", "profile"))
    ap.add_argument("--guava-loss", action="store_true",
                    help="time GUAVA's mask / crop / regulariser loss terms (instead of --mode)")
    ap.add_argument("--B", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.guava_loss == (a.mode is not None):
        ap.error("give --mode or --guava-loss")
    assert torch.cuda.is_available(), "needs a HIP device"
    if a.guava_loss:
        bench_guava_loss(a.B, a)
    else:
        {"backward": bench_backward, "step": bench_step, "profile": profile}[a.mode](a.B, a)
