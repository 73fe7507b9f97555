"""BASELINE config 4 (the training step) at full size: 100k-Gaussian avatar, 512x512.

* render backward + projection backward of ONE config-2 frame through the drop-in `_C` API, and
  of a 6-frame batch (BatchRasterizer.backward, the training step's path, per-frame views) for
  frames 0 and 5, against the CPU oracle's backward (reference backward.cu:147-638 restated):
  every gradient within 1e-4 of its own max magnitude;
* SplatTrainer.gradients (fwd -> (1-l) L1 + l (1 - SSIM) on RGB -> bwd, summed over frames; the
  reference's main/trainer.py:82-102 rasterizer side) against a CPU recomputation: the image
  gradient from torch autograd of an L1 + conv2d-SSIM loss in float64 on the same rendered frames,
  then oracle.backward per frame, summed;
* capacity overflow: NaN frames, CapacityError on the next call, and the trainer skipping the
  overflowing step on the device (fused Adam found_inf) and growing its workspace.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import grad_check, torch_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations")
TOL = 1e-4  # of each gradient's max |oracle| (DESIGN.md numerics contract)


def _rel_err(a, b):
    return float(np.abs(a.reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-20))


def _scene_c2(cams=1, seed=0):
    from guava_renderer_amd import scenes
    sc = scenes.avatar_cloud(100000, seed=seed)
    return sc, scenes.frame_cameras(max(cams, 2), 512, 512, seed=1000)


def _oracle_grads(sc, cam, dL, dLinv, W=512, noise=False):
    """The oracle's gradients; noise=True: also the same gradients accumulated in reverse order (the
    reference's own f32 reordering noise, grad_check's per-element yardstick) -> (grads, reordered)."""
    import oracle
    oracle.set_threads(16)
    bg = np.zeros(32, np.float32)
    _, _, _, st = oracle.forward(sc["means3D"], sc["colors"], sc["opacities"], sc["scales"], sc["rotations"],
                                 None, cam["viewmatrix"], cam["projmatrix"], W, W, cam["tanfovx"],
                                 cam["tanfovy"], bg)
    args = (st, sc["means3D"], sc["colors"], sc["opacities"], sc["scales"], sc["rotations"], None,
            cam["viewmatrix"], cam["projmatrix"], W, W, cam["tanfovx"], cam["tanfovy"], bg, dL, dLinv)
    g = oracle.backward(*args)
    return (g, oracle.backward(*args, reverse_order=True)) if noise else g


def test_fullsize_backward_single_frame_drop_in():
    """Config 4 gradients of one frame through _C.rasterize_gaussians(_backward)."""
    from guava_renderer_amd.diff_gaussian_rasterization_32 import _C
    sc, cams = _scene_c2()
    cam = cams[1]
    d = dict(sc, **cam, bg=np.zeros(32, np.float32))
    t = torch_inputs(d)
    empty = torch.Tensor([])
    R, color, radii, gb, bb, ib, invd = _C.rasterize_gaussians(
        t["bg"], t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], 1.0, empty,
        t["viewmatrix"], t["projmatrix"], cam["tanfovx"], cam["tanfovy"], 512, 512, empty, 0,
        t["campos"], False, False, False)
    rng = np.random.default_rng(11)
    dL = rng.normal(size=(32, 512, 512)).astype(np.float32)
    dLinv = rng.normal(size=(1, 512, 512)).astype(np.float32)
    grads = _C.rasterize_gaussians_backward(
        t["bg"], t["means3D"], radii, t["colors"], t["opacities"], t["scales"], t["rotations"], 1.0, empty,
        t["viewmatrix"], t["projmatrix"], cam["tanfovx"], cam["tanfovy"], torch.tensor(dL, device=DEV),
        torch.tensor(dLinv, device=DEV), empty, 0, t["campos"], gb, R, bb, ib, False, False)
    torch.cuda.synchronize()
    o, o_rev = _oracle_grads(sc, cam, dL, dLinv, noise=True)
    for name, a, b, bn in zip(NAMES, grads, o, o_rev):
        if b.size:
            grad_check(name, a.cpu().numpy(), b, noise=bn)


def test_config5_backward_single_frame():
    """Config 5 (300k Gaussians, 3 per UV texel, 1024^2): one frame's gradients through the batched
    entry vs the oracle, 1e-4 of each gradient's scale."""
    from guava_renderer_amd import scenes
    from guava_renderer_amd.batch import BatchRasterizer
    P, W = 300000, 1024
    sc = scenes.avatar_cloud(P, seed=0, gaussians_per_texel=3)
    cam = scenes.frame_cameras(2, W, W, seed=1000)[1]
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(cam["viewmatrix"].reshape(1, 16))
    projs = t(cam["projmatrix"].reshape(1, 16))
    tanf = t(np.array([[cam["tanfovx"], cam["tanfovy"]]], np.float32))
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    r = BatchRasterizer(1, P, W, W, R_capacity=40 * P, device=DEV)
    r.forward(*args, views, projs, tanf, torch.zeros((1, 32), device=DEV))
    rng = np.random.default_rng(13)
    dL = rng.normal(size=(1, 32, W, W)).astype(np.float32)
    dLinv = rng.normal(size=(1, W, W)).astype(np.float32)
    g = r.backward(*args, views, projs, tanf, torch.zeros((1, 32), device=DEV), t(dL), t(dLinv))
    torch.cuda.synchronize()
    assert not r.status()[1]
    gpu = {k: v[0].cpu().numpy() for k, v in g.items() if v is not None}
    o, o_rev = _oracle_grads(sc, cam, dL[0], dLinv, W=W, noise=True)
    mine = {"means2D": gpu["mean2D"], "colors": gpu["colors"], "opacity": gpu["opacity"], "means3D": gpu["means3D"],
            "cov3D": gpu["cov3D"], "scales": gpu["scales"], "rotations": gpu["rotations"]}
    for name, b, bn in zip(NAMES, o, o_rev):
        if name in mine:
            grad_check(name, mine[name], b, noise=bn)


@pytest.mark.parametrize("split,per_frame_colors", [(False, False), (True, False), (True, True)])
def test_fullsize_backward_batch6(split, per_frame_colors):
    """BatchRasterizer.backward at the training batch (6 per-frame views): frames 0 and 5 vs the
    oracle, per-frame gradient tensors.  split: the split-bf16 switch, whose g contraction takes the
    batch-shared pre-split feature table, or splits per-frame features ([B, P, 32]) in the kernel."""
    from guava_renderer_amd import _lib
    from guava_renderer_amd.batch import BatchRasterizer
    sc, cams = _scene_c2(cams=6)
    cams = cams[:6]
    B = 6
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    bgs = torch.zeros((B, 32), device=DEV)
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    if per_frame_colors:
        args[1] = args[1][None].repeat(B, 1, 1).contiguous()
    r = BatchRasterizer(B, 100000, 512, 512, R_capacity=12 * 100000 * B, device=DEV,
                        numerics=_lib.numerics(split_bf16=split))
    r.forward(*args, views, projs, tanf, bgs)
    rng = np.random.default_rng(12)
    dL = rng.normal(size=(B, 32, 512, 512)).astype(np.float32)
    dLinv = rng.normal(size=(B, 512, 512)).astype(np.float32)
    g = r.backward(*args, views, projs, tanf, bgs, t(dL), t(dLinv))
    torch.cuda.synchronize()
    assert not r.status()[1]
    gpu = {k: v.cpu().numpy() for k, v in g.items() if v is not None}
    for f in (0, 5):
        o, o_rev = _oracle_grads(sc, cams[f], dL[f], dLinv[f][None], noise=True)
        mine = {"means2D": gpu["mean2D"][f], "colors": gpu["colors"][f], "opacity": gpu["opacity"][f],
                "means3D": gpu["means3D"][f], "cov3D": gpu["cov3D"][f], "scales": gpu["scales"][f],
                "rotations": gpu["rotations"][f]}
        print(f"frame {f} (split {split}, per-frame colours {per_frame_colors}):")
        for name, b, bn in zip(NAMES, o, o_rev):
            if name in mine:
                # split-bf16 g (≤ 3e-5 relative per product) cancels over the 32
                # channels of a random dL: the per-element tail is looser than the exact mode's,
                # p99.9 <= 5e-4 instead of 1e-4 (max and scale bars unchanged)
                grad_check(f"frame {f} {name}", mine[name], b, noise=bn, p999_tol=5e-4 if split else None)


def _ssim64(img, tgt):
    g = torch.tensor([np.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float64)
    g = g / g.sum()
    ch = img.shape[1]
    w = (g[:, None] @ g[None, :]).expand(ch, 1, 11, 11).contiguous()
    mu1 = F.conv2d(img, w, padding=5, groups=ch)
    mu2 = F.conv2d(tgt, w, padding=5, groups=ch)
    s1 = F.conv2d(img * img, w, padding=5, groups=ch) - mu1 ** 2
    s2 = F.conv2d(tgt * tgt, w, padding=5, groups=ch) - mu2 ** 2
    s12 = F.conv2d(img * tgt, w, padding=5, groups=ch) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean()


def test_trainer_gradients_match_cpu_recomputation():
    from guava_renderer_amd import scenes
    from guava_renderer_amd.train import SplatTrainer
    B, W = 2, 512
    sc = scenes.avatar_cloud(100000, seed=0)
    cams = scenes.frame_cameras(B, W, W, seed=1000)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    params = {k: t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    tr = SplatTrainer(params, B, W, W, R_capacity=12 * 100000 * B, device=DEV)
    target = torch.rand((B, 3, W, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    loss, grads = tr.gradients(views, projs, tanf, target)
    torch.cuda.synchronize()
    feat = tr.rast.out_color.detach().cpu().double().requires_grad_(True)
    img = feat[:, :3]
    tgt = target.cpu().double()
    lam = tr.lambda_ssim
    refined = torch.einsum("oc,bchw->bohw", tr.refine_w.cpu().double(), feat)
    ref_loss = (1 - lam) * (img - tgt).abs().mean() + lam * (1 - _ssim64(img, tgt)) + (refined - tgt).abs().mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * abs(ref_loss.item()) + 1e-6
    dfeat = feat.grad.float().numpy()
    assert np.abs(dfeat[:, 3:]).max() > 0  # every channel carries a gradient
    acc = None
    for f in range(B):
        dL = np.ascontiguousarray(dfeat[f])
        o = _oracle_grads(sc, cams[f], dL, np.zeros((1, W, W), np.float32))
        o = {"means3D": o[3], "colors": o[1], "opacities": o[2], "scales": o[6], "rotations": o[7]}
        acc = o if acc is None else {k: acc[k] + o[k] for k in acc}
    for k, b in acc.items():  # (frame sums of gradients of a float64 loss: 2e-4 of scale)
        grad_check(k, grads[k].cpu().numpy(), b, scale_tol=2e-4)


def test_overflow_nan_frames_and_capacity_error():
    from guava_renderer_amd import _lib, scenes
    from guava_renderer_amd.batch import BatchRasterizer
    sc = scenes.avatar_cloud(20000, seed=1)
    cams = scenes.frame_cameras(2, 256, 256, seed=1000)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    bgs = torch.zeros((2, 32), device=DEV)
    r = BatchRasterizer(2, 20000, 256, 256, R_capacity=1000, device=DEV)
    col, inv, _ = r.forward(*args, views, projs, tanf, bgs)
    torch.cuda.synchronize()
    assert torch.isnan(col).all() and torch.isnan(inv).all()
    assert int(r.overflow_flag()) == 1
    with pytest.raises(_lib.CapacityError):
        r.poll(wait=True)
    r.poll(wait=True)  # acknowledged: cleared
    # a large enough workspace renders the same batch
    r2 = BatchRasterizer(2, 20000, 256, 256, R_capacity=20 * 20000 * 2, device=DEV)
    col2, _, _ = r2.forward(*args, views, projs, tanf, bgs)
    r2.poll(wait=True)
    assert torch.isfinite(col2).all()
    assert r2.max_instances_seen() > 1000


def test_trainer_skips_overflowing_step():
    from guava_renderer_amd import scenes
    from guava_renderer_amd.train import SplatTrainer
    sc = scenes.avatar_cloud(20000, seed=2)
    cams = scenes.frame_cameras(2, 256, 256, seed=1000)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    params = {k: t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    tr = SplatTrainer(params, 2, 256, 256, R_capacity=1000, device=DEV)
    target = torch.rand((2, 3, 256, 256), device=DEV)
    before = {k: v.detach().clone() for k, v in tr.p.items()}
    loss = tr.step(views, projs, tanf, target)
    torch.cuda.synchronize()
    assert torch.isnan(loss)
    for k, v in tr.p.items():  # the update was skipped on the device
        assert torch.equal(v.detach(), before[k]), k
    with pytest.warns(UserWarning):
        loss2 = tr.step(views, projs, tanf, target)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 1 and tr.rast.R_capacity > 1000
    assert torch.isfinite(loss2)
    assert any(not torch.equal(v.detach(), before[k]) for k, v in tr.p.items())


def test_shared_backward_equals_summed_per_frame_backward():
    """gsr_backward_batch_shared (frame sums inside the kernels) vs the per-frame gradients of
    gsr_backward_batch summed over the frames, with and without an inverse-depth gradient."""
    from guava_renderer_amd import scenes
    from guava_renderer_amd.batch import BatchRasterizer
    B, W, P = 4, 256, 20000
    sc = scenes.avatar_cloud(P, seed=4)
    cams = scenes.frame_cameras(B, W, W, seed=1000)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    bgs = torch.zeros((B, 32), device=DEV)
    r = BatchRasterizer(B, P, W, W, R_capacity=24 * P * B, device=DEV)
    r.forward(*args, views, projs, tanf, bgs)
    gen = torch.Generator(device=DEV).manual_seed(9)
    dL = torch.randn((B, 32, W, W), device=DEV, generator=gen)
    dinv = torch.randn((B, W, W), device=DEV, generator=gen)
    for di in (None, dinv):
        per = r.backward(*args, views, projs, tanf, bgs, dL, di)
        sh = r.backward(*args, views, projs, tanf, bgs, dL, di, shared=True)
        torch.cuda.synchronize()
        for k in ("means3D", "colors", "opacity", "scales", "rotations"):
            ref = per[k].sum(0).cpu().numpy()
            err = _rel_err(sh[k].cpu().numpy(), ref)
            assert err <= 1e-5, f"{k} (invdepth {di is not None}): {err:.3g}"


def test_image_loss_kernel_matches_autograd():
    """gsr_image_loss (the trainer's two L1 terms + the SSIM gradient's addition, one pass) vs torch
    autograd of SplatTrainer.loss's L1 terms on the same features (float64)."""
    import ctypes
    from guava_renderer_amd import _lib
    gen = torch.Generator(device=DEV).manual_seed(21)
    B, H, W = 2, 64, 96
    feat = torch.rand((B, 32, H, W), device=DEV, generator=gen)
    tgt = torch.rand((B, 3, H, W), device=DEV, generator=gen)
    extra = torch.randn((B, 3, H, W), device=DEV, generator=gen) * 1e-3
    rw = (torch.rand((3, 32), device=DEV, generator=gen) * 2 - 1) / 32 ** 0.5
    L = _lib.load()
    for use_rw in (True, False):
        part = torch.empty((L.gsr_image_loss_partials(B, H, W),), device=DEV)
        dL = torch.empty_like(feat)
        _lib.check(L.gsr_image_loss(B, H, W, feat.data_ptr(), tgt.data_ptr(), rw.data_ptr() if use_rw else None,
                                    0.8, 1.0 if use_rw else 0.0, extra.data_ptr(), dL.data_ptr(), part.data_ptr(),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gsr_image_loss")
        f = feat.double().cpu().requires_grad_(True)
        t = tgt.double().cpu()
        ref = 0.8 * (f[:, :3] - t).abs().mean()
        if use_rw:
            ref = ref + (torch.einsum("oc,bchw->bohw", rw.double().cpu(), f) - t).abs().mean()
        ref.backward()
        g = f.grad.clone()
        g[:, :3] += extra.double().cpu()
        torch.cuda.synchronize()
        assert abs(part.sum().item() - ref.item()) <= 1e-5 * abs(ref.item())
        np.testing.assert_allclose(dL.cpu().double().numpy(), g.numpy(), atol=1e-9, rtol=1e-5)


def _image_loss_inputs(B, H, W):
    """CPU float32 inputs of gsr_image_loss at a ragged size (seeded by the shape)."""
    gen = torch.Generator().manual_seed(1000 * B + 37 * H + W)
    feat = torch.rand((B, 32, H, W), generator=gen)
    tgt = torch.rand((B, 3, H, W), generator=gen)
    extra = torch.randn((B, 3, H, W), generator=gen) * 1e-3
    rw = (torch.rand((3, 32), generator=gen) * 2 - 1) / 32 ** 0.5
    return feat, tgt, extra, rw


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 15, 17), (1, 1, 257), (3, 37, 53)])
@pytest.mark.parametrize("use_rw", [True, False])
@pytest.mark.parametrize("use_extra", [True, False])
def test_image_loss_kernel_ragged_sizes(B, H, W, use_rw, use_extra):
    """gsr_image_loss where H*W is no multiple of the 256-thread workgroup (1, 255, 257, 1961): the
    last workgroup's idle lanes add nothing to its partial and write nothing.  Outputs start as NaN;
    bars and float64 reference as test_image_loss_kernel_matches_autograd."""
    import ctypes
    from guava_renderer_amd import _lib
    feat, tgt, extra, rw = _image_loss_inputs(B, H, W)
    f = feat.double().requires_grad_(True)
    t = tgt.double()
    diffs = [f[:, :3] - t]
    if use_rw:
        diffs.append(torch.einsum("oc,bchw->bohw", rw.double(), f) - t)
    margin = min(d.abs().min().item() for d in diffs)
    assert margin >= 1e-6, f"inputs: a difference of {margin:.3g} sits on L1's kink (pick another seed)"
    ref = 0.8 * diffs[0].abs().mean() + (diffs[1].abs().mean() if use_rw else 0.0)
    ref.backward()
    g = f.grad.clone()
    if use_extra:
        g[:, :3] += extra.double()
    L = _lib.load()
    n_part = L.gsr_image_loss_partials(B, H, W)
    assert n_part == B * ((H * W + 255) // 256)
    d_feat, d_tgt, d_extra, d_rw = (x.to(DEV) for x in (feat, tgt, extra, rw))
    part = torch.full((n_part,), float("nan"), device=DEV)
    dL = torch.full_like(d_feat, float("nan"))
    _lib.check(L.gsr_image_loss(B, H, W, d_feat.data_ptr(), d_tgt.data_ptr(), d_rw.data_ptr() if use_rw else None,
                                0.8, 1.0 if use_rw else 0.0, d_extra.data_ptr() if use_extra else None,
                                dL.data_ptr(), part.data_ptr(),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gsr_image_loss")
    torch.cuda.synchronize()
    assert part.numel() == n_part and bool(torch.isfinite(part).all())
    assert abs(part.sum().item() - ref.item()) <= 1e-5 * abs(ref.item())
    np.testing.assert_allclose(dL.cpu().double().numpy(), g.numpy(), atol=1e-9, rtol=1e-5)
