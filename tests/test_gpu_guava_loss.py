"""GPU tests of GUAVA's further loss terms (include/gsr_loss.h, csrc/loss.hip): the foreground mask,
the head / hand crop losses with their deterministic gather backward, the UV-Gaussian regularisers,
and the trainers' mask / boxes / reg arguments.

Reference of every comparison: tests/guava_loss_ref.py in float64 on the CPU with autograd.  Bars, as
test_gpu_train.py::test_image_loss_kernel_matches_autograd: loss within 1e-5 relative, gradient
rtol 1e-5 / atol 1e-9.  L1's sign is discontinuous, so every comparison first asserts on the float64
reference that no difference an absolute value is taken of is below 1e-6 (a condition on the inputs:
the seeds of the small shapes were picked so that it holds; the production-size inputs are
constructed with a margin, see _production_inputs)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guava_loss_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W = 2, 48, 64
GW3 = (0.25, 0.1, 0.1)


@functools.lru_cache(maxsize=None)
def _inputs(seed, B=B, H=H, W=W):
    """CPU float32 inputs, made once per seed and never modified."""
    g = torch.Generator().manual_seed(seed)
    return dict(feat=torch.rand((B, 32, H, W), generator=g), tgt=torch.rand((B, 3, H, W), generator=g),
                mask=torch.rand((B, 1, H, W), generator=g),  # soft
                rw=(torch.rand((3, 32), generator=g) * 2 - 1) / 32 ** 0.5,
                extra=torch.randn((B, 3, H, W), generator=g) * 1e-3)


def _boxes(rows):
    """[G][B] of (l, r, t, b) -> int32 [G,B,4]."""
    return torch.tensor(rows, dtype=torch.int32)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run(inp, use_rw=True, l1w=0.8, rfw=1.0, mask=False, bg=0.0, mr=False, boxes=None, gw=None, S=16, extra=False,
         crops_grad=None, want_crops=False):
    """gsr_guava_loss_forward + gsr_guava_loss_backward -> dict of CPU results."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    feat, tgt = inp["feat"].to(DEV), inp["tgt"].to(DEV)
    Bn, _, Hn, Wn = feat.shape
    rw = inp["rw"].to(DEV) if use_rw else None
    m = inp["mask"].to(DEV) if mask else None
    ex = inp["extra"].to(DEV) if extra else None
    G = 0 if boxes is None else boxes.shape[0]
    K = 2 if use_rw else 1
    bx = boxes.to(DEV).contiguous() if G else None
    gwt = torch.tensor(gw, dtype=torch.float32, device=DEV) if G else None
    n_ws = L.gsr_guava_loss_workspace_bytes(Bn, Hn, Wn, G, S)
    n_part = L.gsr_guava_loss_partials(Bn, Hn, Wn, G, S)
    assert n_ws > 0 and n_part > 0
    ws = torch.empty((n_ws // 4,), device=DEV)
    part = torch.full((n_part,), float("nan"), device=DEV)
    dL = torch.full_like(feat, float("nan"))
    crops = torch.full((K, G, Bn, 3, S, S), float("nan"), device=DEV) if want_crops else None
    crops_t = torch.full((G, Bn, 3, S, S), float("nan"), device=DEV) if want_crops else None
    n_valid = torch.full((max(G, 1),), -1, dtype=torch.int32, device=DEV)
    cg = crops_grad.to(DEV).contiguous() if crops_grad is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.gsr_guava_loss_forward(Bn, Hn, Wn, feat.data_ptr(), tgt.data_ptr(), _ptr(rw), l1w, rfw, _ptr(m), bg,
                                        int(mr), G, S, _ptr(bx), _ptr(gwt), _ptr(crops), _ptr(crops_t),
                                        n_valid.data_ptr(), part.data_ptr(), ws.data_ptr(), stream),
               "gsr_guava_loss_forward")
    _lib.check(L.gsr_guava_loss_backward(Bn, Hn, Wn, _ptr(rw), l1w, rfw, _ptr(m), int(mr), G, S, _ptr(bx), _ptr(cg),
                                         _ptr(ex), dL.data_ptr(), ws.data_ptr(), stream), "gsr_guava_loss_backward")
    torch.cuda.synchronize()
    n_frame = L.gsr_image_loss_partials(Bn, Hn, Wn)
    return dict(loss=part.double().sum().item(), dL=dL.cpu(), part=part.cpu(), n_frame=n_frame,
                crops=None if crops is None else crops.cpu(), crops_t=None if crops_t is None else crops_t.cpu(),
                n_valid=n_valid.cpu())


def _reference(inp, use_rw=True, l1w=0.8, rfw=1.0, mask=False, bg=0.0, mr=False, boxes=None, gw=None, S=16,
               extra=False):
    """(loss, gradient [B,32,H,W] float64 with extra added) of the float64 restatement; asserts the
    sign margin."""
    f = inp["feat"].double().requires_grad_(True)
    diffs = []
    loss = ref.image_loss(f, inp["tgt"].double(), inp["rw"].double() if use_rw else None, l1w, rfw,
                          mask=inp["mask"].double() if mask else None, bg=bg, mask_refined=mr,
                          boxes=None if boxes is None else boxes.tolist(), group_weight=gw, S=S, diffs=diffs)
    margin = min(d.abs().min().item() for d in diffs)
    assert margin >= 1e-6, f"inputs: a difference of {margin:.3g} sits on L1's kink (pick another seed)"
    loss.backward()
    g = f.grad.clone()
    if extra:
        g[:, :3] += inp["extra"].double()
    return loss.item(), g


def _compare(got, want):
    loss, g = want
    print(f"  loss {got['loss']:.9g} ref {loss:.9g}; max |dL - ref| "
          f"{(got['dL'].double() - g).abs().max().item():.3g} of max {g.abs().max().item():.3g}")
    assert torch.isfinite(got["dL"]).all() and torch.isfinite(got["part"]).all()
    assert abs(got["loss"] - loss) <= 1e-5 * abs(loss)
    np.testing.assert_allclose(got["dL"].double().numpy(), g.numpy(), atol=1e-9, rtol=1e-5)


def _both(inp, **kw):
    got = _run(inp, **kw)
    _compare(got, _reference(inp, **kw))
    return got


# ---- 1. mask only

@pytest.mark.parametrize("use_rw", [True, False])
@pytest.mark.parametrize("mr", [False, True])
@pytest.mark.parametrize("bg", [0.0, 0.3])
def test_mask_only(bg, mr, use_rw):
    _both(_inputs(2), use_rw=use_rw, mask=True, bg=bg, mr=mr, extra=True)


@pytest.mark.parametrize("use_rw", [True, False])
def test_without_mask_and_boxes_equals_image_loss_bit_for_bit(use_rw):
    from guava_renderer_amd import _lib
    L = _lib.load()
    inp = _inputs(1)
    got = _run(inp, use_rw=use_rw, rfw=1.0 if use_rw else 0.0, extra=True, mr=True)
    feat, tgt, rw, ex = (inp[k].to(DEV) for k in ("feat", "tgt", "rw", "extra"))
    part = torch.empty((L.gsr_image_loss_partials(B, H, W),), device=DEV)
    dL = torch.empty_like(feat)
    _lib.check(L.gsr_image_loss(B, H, W, feat.data_ptr(), tgt.data_ptr(), rw.data_ptr() if use_rw else None, 0.8,
                                1.0 if use_rw else 0.0, ex.data_ptr(), dL.data_ptr(), part.data_ptr(),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gsr_image_loss")
    torch.cuda.synchronize()
    assert got["part"].shape == part.shape
    assert torch.equal(got["part"], part.cpu()) and torch.equal(got["dL"], dL.cpu())


# ---- 2. crop geometry, one box per case

GEOMETRY = {"upscale 9x7": ((10, 19, 5, 12), 16), "downscale 40x37": ((3, 43, 2, 39), 16),
            "one pixel wide": ((20, 21, 4, 30), 16), "one pixel high": ((5, 50, 17, 18), 16),
            "full frame": ((0, W, 0, H), 16), "right and bottom border": ((50, W, 30, H), 16),
            "out of range": ((-7, 1000, 20, 100), 16), "identity 32x32": ((16, 48, 8, 40), 32)}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_crop_geometry(case):
    box, S = GEOMETRY[case]
    inp = _inputs(2)
    kw = dict(boxes=_boxes([[box] * B]), gw=(0.25,), S=S)
    got = _both(inp, **kw)
    assert got["n_valid"].tolist() == [B]
    # where the crop term adds no gradient it adds exact zeros: dL_dfeat keeps the bits of the call
    # without boxes outside the (clamped) box, and inside it at the pixels that no sample reads
    none = _run(inp)
    changed = got["dL"] != none["dL"]
    l, r, t, b = ref.clamp_box(box, H, W)
    inside = torch.zeros((B, 32, H, W), dtype=torch.bool)
    inside[:, :, t:b, l:r] = True
    assert changed[inside].any() and not changed[~inside].any()
    if case == "downscale 40x37":
        y0, y1, _, _ = ref.axis_taps(b - t, S)
        x0, x1, _, _ = ref.axis_taps(r - l, S)
        read = torch.zeros((H, W), dtype=torch.bool)
        for ys in (y0, y1):
            for xs in (x0, x1):
                read[(t + ys)[:, None], (l + xs)[None, :]] = True
        unread = inside[0, 0] & ~read
        assert unread.sum().item() > 100
        assert not changed[:, :, unread].any()


# ---- 3. skipped crops

def test_one_frames_box_is_empty():
    boxes = _boxes([[(8, 30, 6, 31), (12, 12, 3, 20)], [(70, 90, 0, 5), (5, 40, 9, 33)]])
    got = _both(_inputs(2), boxes=boxes, gw=(0.25, 0.1))
    assert got["n_valid"].tolist() == [1, 1]  # the mean of each group is over its one kept crop


def test_group_empty_in_every_frame_adds_exact_zeros():
    inp = _inputs(2)
    boxes = _boxes([[(30, 8, 6, 31), (12, 40, 20, 20)]])
    got = _both(inp, boxes=boxes, gw=(0.25,), mask=True, mr=True)
    none = _run(inp, mask=True, mr=True)
    assert got["n_valid"].tolist() == [0]
    assert torch.equal(got["dL"], none["dL"])
    nf = got["n_frame"]
    assert torch.equal(got["part"][:nf], none["part"]) and got["part"][nf:].abs().max().item() == 0.0
    # beside a kept group
    both = _both(inp, boxes=_boxes([[(30, 8, 6, 31), (12, 40, 20, 20)], [(8, 30, 6, 31), (5, 40, 9, 33)]]),
                 gw=(0.25, 0.1))
    assert both["n_valid"].tolist() == [0, 2]


# ---- 4. overlap, both images, all 32 channels

OVERLAP = [[(5, 40, 4, 30), (10, 50, 8, 44)], [(20, 60, 10, 40), (0, 33, 0, 21)], [(30, 45, 20, 35), (25, 64, 15, 48)]]


def test_overlapping_boxes_both_images_extra_grad():
    got = _both(_inputs(5), boxes=_boxes(OVERLAP), gw=GW3, mask=True, bg=0.3, mr=True, extra=True)
    assert got["dL"][:, 3:].abs().max().item() > 0
    _both(_inputs(5), boxes=_boxes(OVERLAP), gw=GW3, mask=True, bg=0.3, mr=False, use_rw=False, rfw=0.0)


# ---- 5. crop buffers

def test_crop_buffers_and_destination_gradient():
    inp = _inputs(5)
    S = 16
    rows = [OVERLAP[0], [(20, 60, 10, 40), (33, 33, 0, 21)], OVERLAP[2]]
    boxes = _boxes(rows)
    kw = dict(boxes=boxes, gw=GW3, S=S, mask=True, bg=0.3, mr=False)
    got = _run(inp, want_crops=True, **kw)
    feat, tgt, m, rw = inp["feat"], inp["tgt"], inp["mask"], inp["rw"]
    t = tgt * m + (1 - m) * 0.3
    images = [feat[:, :3], torch.einsum("oc,bchw->bohw", rw, feat)]
    for g in range(3):
        for b in range(B):
            bx = ref.clamp_box(rows[g][b], H, W)
            for k in range(2):
                want = torch.zeros((3, S, S)) if bx is None else \
                    F.interpolate(images[k][b:b + 1, :, bx[2]:bx[3], bx[0]:bx[1]], (S, S), mode="bilinear")[0]
                assert (got["crops"][k, g, b] - want).abs().max().item() <= 1e-6, (k, g, b)
            want = torch.zeros((3, S, S)) if bx is None else \
                F.interpolate(t[b:b + 1, :, bx[2]:bx[3], bx[0]:bx[1]], (S, S), mode="bilinear")[0]
            assert (got["crops_t"][g, b] - want).abs().max().item() <= 1e-6, (g, b)
    # <adjoint(g), x> = <g, resample(x)>: the destination gradient's share of dL_dfeat is the
    # difference of two calls; through the refine head W for the refined image's crops
    gen = torch.Generator().manual_seed(55)
    cg = torch.randn((2, 3, B, 3, S, S), generator=gen)
    x = torch.randn((B, 32, H, W), generator=gen, dtype=torch.float64)
    with_g = _run(inp, crops_grad=cg, **kw)
    adj = with_g["dL"].double() - got["dL"].double()
    lhs = (adj * x).sum().item()
    xs = [x[:, :3], torch.einsum("oc,bchw->bohw", rw.double(), x)]
    rhs = 0.0
    for k in range(2):
        for g in range(3):
            for b, c in enumerate(ref.crops(xs[k], rows[g], S)):
                if c is not None:  # (the gradient of a skipped slot is ignored)
                    rhs += (cg[k, g, b].double() * c).sum().item()
    print(f"  <adjoint(g), x> {lhs:.9g}  <g, resample(x)> {rhs:.9g}")
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs)


# ---- 6. determinism

def test_two_runs_give_identical_bits():
    inp = _inputs(5)
    cg = torch.randn((2, 3, B, 3, 16, 16), generator=torch.Generator().manual_seed(6)) * 1e-4
    kw = dict(boxes=_boxes(OVERLAP), gw=GW3, mask=True, bg=0.3, mr=True, extra=True, crops_grad=cg, want_crops=True)
    a, b = _run(inp, **kw), _run(inp, **kw)
    for k in ("dL", "part", "crops", "crops_t"):
        assert torch.equal(a[k], b[k]), k


# ---- 7. regularisers

@pytest.mark.parametrize("N", [1000, 1])
def test_uv_regularizers(N):
    from guava_renderer_amd import _lib
    L = _lib.load()
    g = torch.Generator().manual_seed(7)
    lp = torch.randn((N, 3), generator=g) * 2.2  # norms on both sides of 3.0
    sc = torch.rand((N, 3), generator=g) * 1.2  # components on both sides of 0.6
    if N > 1:
        lp[5] = 0.0
        sc[9] = torch.tensor([0.1, 0.59, 0.3])
        assert ((lp.norm(dim=-1) > 3.0).sum() > 50) and ((lp.norm(dim=-1) < 3.0).sum() > 50)
    else:
        lp[0] = torch.tensor([2.0, -2.0, 2.0])
        sc[0] = torch.tensor([0.9, 0.2, 0.7])
    th = (3.0, 0.01, 0.6, 1.0)
    n_part = L.gsr_uv_regularizers_partials(N)
    part = torch.full((2 * n_part,), float("nan"), device=DEV)
    d_lp, d_sc = torch.full((N, 3), float("nan"), device=DEV), torch.full((N, 3), float("nan"), device=DEV)
    lpd, scd = lp.to(DEV), sc.to(DEV)
    _lib.check(L.gsr_uv_regularizers(N, lpd.data_ptr(), scd.data_ptr(), *th, part.data_ptr(), d_lp.data_ptr(),
                                     d_sc.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "gsr_uv_regularizers")
    torch.cuda.synchronize()
    a, b = lp.double().requires_grad_(True), sc.double().requires_grad_(True)
    la, lb = ref.regularizers(a, b, *th)
    (la + lb).backward()
    got = part.cpu().double().view(2, n_part).sum(1)
    assert la.item() > 0 and lb.item() > 0
    assert abs(got[0].item() - la.item()) <= 1e-5 * la.item() and abs(got[1].item() - lb.item()) <= 1e-5 * lb.item()
    np.testing.assert_allclose(d_lp.cpu().double().numpy(), a.grad.numpy(), atol=1e-9, rtol=1e-5)
    np.testing.assert_allclose(d_sc.cpu().double().numpy(), b.grad.numpy(), atol=1e-9, rtol=1e-5)
    if N > 1:
        assert d_lp[5].abs().max().item() == 0.0 and d_sc[9].abs().max().item() == 0.0


# ---- 8. production size

PROD_BOXES = [[(180, 330, 40, 190), (170, 322, 52, 201)], [(100, 160, 300, 360), (90, 151, 310, 368)],
              [(350, 410, 310, 370), (360, 419, 296, 357)]]


def _production_inputs():
    """B=2, 512 x 512.  ~5.5M differences would put ~10 of them within 1e-6 of L1's kink for any
    seed, so these inputs carry a margin by construction: every difference has magnitude >= 0.01,
    with a sign that is random per pixel and channel outside the boxes and constant per (frame, box,
    image, channel) inside one (a resampled difference is a convex combination of its taps'), which
    leaves the sample positions and weights -- what this size is about -- fully exercised."""
    Bn, Hn = 2, 512
    g = torch.Generator().manual_seed(8)
    f64 = dict(dtype=torch.float64, generator=g)
    tgt = torch.rand((Bn, 3, Hn, Hn), **f64).float()
    m = (0.2 + 0.8 * torch.rand((Bn, 1, Hn, Hn), **f64)).float()
    rw = ((torch.rand((3, 32), **f64) * 2 - 1) / 32 ** 0.5).float()
    bg = 0.3
    t = (tgt * m + (1 - m) * bg).double()
    sign = [torch.where(torch.rand((Bn, 3, Hn, Hn), **f64) < 0.5, -1.0, 1.0) for _ in range(2)]
    for rows in PROD_BOXES:
        for b, (l, r, top, bo) in enumerate(rows):
            for s in sign:
                s[b, :, top:bo, l:r] = torch.where(torch.rand((3, 1, 1), **f64) < 0.5, -1.0, 1.0)
    mag = [0.05 + 0.45 * torch.rand((Bn, 3, Hn, Hn), **f64) for _ in range(2)]
    feat = torch.rand((Bn, 32, Hn, Hn), **f64)
    feat[:, :3] = t + sign[0] * mag[0]
    # the refined image before the mask: r = tgt + sign * mag, by solving W . feat = r for channels 3-5
    want_r = tgt.double() + sign[1] * mag[1]
    rest = torch.einsum("oc,bchw->bohw", rw.double()[:, [0, 1, 2] + list(range(6, 32))],
                        feat[:, [0, 1, 2] + list(range(6, 32))])
    feat[:, 3:6] = torch.einsum("oc,bchw->bohw", torch.linalg.inv(rw.double()[:, 3:6]), want_r - rest)
    return dict(feat=feat.float(), tgt=tgt, mask=m, rw=rw, extra=torch.zeros((Bn, 3, Hn, Hn)))


def test_production_size():
    inp = _production_inputs()
    assert inp["feat"][:, 3:6].abs().max().item() < 1e3
    _both(inp, boxes=_boxes(PROD_BOXES), gw=GW3, S=256, mask=True, bg=0.3, mr=True)


# ---- 9. trainers

def _splat_scene():
    from helpers import make_scene
    Wt, P = 64, 400
    ds = [make_scene("avatar", P=P, W=Wt, H=Wt, seed=5, yaw=y) for y in (0.0, 0.4)]
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(np.stack([d["viewmatrix"].reshape(16) for d in ds]).astype(np.float32))
    projs = t(np.stack([d["projmatrix"].reshape(16) for d in ds]).astype(np.float32))
    tanf = t(np.array([[d["tanfovx"], d["tanfovy"]] for d in ds], np.float32))
    params = {k: t(ds[0][k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    return params, views, projs, tanf, Wt, P


def test_splat_trainer_mask_and_boxes():
    from helpers import grad_check
    from guava_renderer_amd.train import SplatTrainer
    params, views, projs, tanf, Wt, P = _splat_scene()
    tr = SplatTrainer(params, 2, Wt, Wt, R_capacity=64 * P * 2, device=DEV, crop_size=16, loss_bg=0.3)
    gen = torch.Generator(device=DEV).manual_seed(9)
    target = torch.rand((2, 3, Wt, Wt), device=DEV, generator=gen)
    mask = torch.rand((2, 1, Wt, Wt), device=DEV, generator=gen)
    boxes = {"head_box": torch.tensor([[10, 50, 4, 40], [12, 52, 6, 44]]),  # int64, as GUAVA's loader gives
             "left_hand_box": torch.tensor([[5, 20, 30, 47], [7, 7, 30, 47]]),
             "right_hand_box": torch.tensor([[40, 60, 35, 64], [38, 70, 33, 60]])}
    for mr in (True, False):
        loss, grads = tr.gradients(views, projs, tanf, target, mask=mask, boxes=boxes, mask_refined=mr)
        torch.cuda.synchronize()
        feat = tr.rast.out_color.detach().clone().requires_grad_(True)
        want = tr.loss(feat, target, mask=mask, boxes=boxes, mask_refined=mr)
        want.backward()
        print(f"  mask_refined {mr}: loss {loss.item():.9g} restated {want.item():.9g}")
        assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
        assert feat.grad[:, 3:].abs().max().item() > 0
        p = tr.p
        g = tr.rast.backward(p["means3D"].detach(), p["colors"].detach(), p["opacities"].detach(),
                             p["scales"].detach(), p["rotations"].detach(), views, projs, tanf, tr.bg,
                             feat.grad.contiguous(), tr.dinv, shared=True)
        torch.cuda.synchronize()
        g["opacities"] = g.pop("opacity")
        for k in grads:
            grad_check(k, grads[k].cpu().numpy(), g[k].cpu().numpy(), scale_tol=2e-4)
    # a [G,B,4] tensor is the dict in BOX_KEYS order
    loss2, _ = tr.gradients(views, projs, tanf, target, mask=mask, mask_refined=False,
                            boxes=torch.stack([boxes[k] for k in tr.BOX_KEYS]))
    assert abs(loss2.item() - loss.item()) <= 1e-6 * abs(loss.item())
    step_loss = tr.step(views, projs, tanf, target, mask=mask, boxes=boxes)
    assert torch.isfinite(step_loss)


def test_splat_trainer_defaults_run_the_unchanged_path():
    """With mask, boxes left at None the step is the parent's: the loss and the image gradient are
    gsr_image_loss's, bit for bit (the attribute gradients come from render_bwd's float atomics, whose
    last bits differ run to run, so those are held to the scale bar)."""
    from helpers import GRAD_SCALE_TOL, scale_err
    from guava_renderer_amd import _lib
    from guava_renderer_amd.fused_ssim import fused_ssim
    from guava_renderer_amd.train import SplatTrainer
    params, views, projs, tanf, Wt, P = _splat_scene()
    target = torch.rand((2, 3, Wt, Wt), device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    tr = SplatTrainer(params, 2, Wt, Wt, R_capacity=64 * P * 2, device=DEV, crop_weights=(0.25, 0.1, 0.1),
                      crop_size=256, crop_ssim=True)
    loss, grads = tr.gradients(views, projs, tanf, target, mask=None, boxes=None, mask_refined=False)
    torch.cuda.synchronize()
    assert tr._guava_bufs is None  # the new kernels did not run
    col = tr.rast.out_color
    img = col[:, :3].detach().requires_grad_(True)
    ssim_term = tr.lambda_ssim * (1.0 - fused_ssim(img, target))
    ssim_term.backward()
    L = _lib.load()
    part = torch.empty((L.gsr_image_loss_partials(2, Wt, Wt),), device=DEV)
    dL = torch.empty_like(col)
    _lib.check(L.gsr_image_loss(2, Wt, Wt, col.data_ptr(), target.data_ptr(), tr.refine_w.data_ptr(),
                                1.0 - tr.lambda_ssim, 1.0, img.grad.contiguous().data_ptr(), dL.data_ptr(),
                                part.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "gsr_image_loss")
    torch.cuda.synchronize()
    assert torch.equal(loss, (ssim_term.detach() + part.sum()).detach())
    assert torch.equal(tr._loss_bufs[1], dL)
    tr0 = SplatTrainer(params, 2, Wt, Wt, R_capacity=64 * P * 2, device=DEV)
    loss0, grads0 = tr0.gradients(views, projs, tanf, target)
    torch.cuda.synchronize()
    assert tr0._guava_bufs is None and abs(loss0.item() - loss.item()) <= 1e-6 * abs(loss.item())
    for k in grads:
        assert scale_err(grads[k].cpu().numpy(), grads0[k].cpu().numpy()) <= GRAD_SCALE_TOL, k


def test_avatar_trainer_regularizers():
    import deform_cases
    from guava_renderer_amd import _lib, scenes
    from guava_renderer_amd.train import AvatarTrainer
    c = deform_cases.make_case(3, 400, 600, 1500, 3)
    Bn, V, Wt = c["B"], c["V"], 64
    P = V + c["N"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    va = {"rotations": t(c["vtx_rotations"]), "scales": t(c["vtx_scales"]), "opacities": t(c["opacities"][:V]),
          "colors": t(c["colors"][:V])}
    ua = {"rotations": t(c["uv_rotations"]), "scales": t(c["uv_scales"]), "opacities": t(c["opacities"][V:]),
          "colors": t(c["colors"][V:]), "local_pos": t(c["local_xyz"]), "binding_face": t(c["binding_face"]),
          "face_bary": t(c["face_bary"])}
    cams = scenes.frame_cameras(Bn, Wt, Wt, seed=5)
    views = t(np.stack([cm["viewmatrix"].reshape(16) for cm in cams]))
    projs = t(np.stack([cm["projmatrix"].reshape(16) for cm in cams]))
    tanf = t(np.array([[cm["tanfovx"], cm["tanfovy"]] for cm in cams], np.float32))
    verts, T = t(c["verts"]), t(c["vert_transforms"])
    target = torch.rand((Bn, 3, Wt, Wt), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    # thresholds at this avatar's medians, so both regularisers are active on about half of the rows
    reg = dict(lambda_local_xyz=0.01, threshold_local_xyz=float(np.median(np.linalg.norm(c["local_xyz"], axis=-1))),
               lambda_local_scale=1.0, threshold_scale=float(np.median(c["uv_scales"])))
    mk = lambda r: AvatarTrainer(va, ua, t(c["faces"]), Bn, Wt, Wt, R_capacity=64 * P * Bn, device=DEV,  # noqa: E731
                                 apply_rgb_sigmoid=False, reg=r)
    assert set(AvatarTrainer.GUAVA_REG) == set(reg) and AvatarTrainer.GUAVA_REG["threshold_local_xyz"] == 3.0
    plain, with_reg = mk(None), mk(reg)
    loss0, g0 = plain.gradients(verts, T, views, projs, tanf, target)
    loss1, g1 = with_reg.gradients(verts, T, views, projs, tanf, target)
    # the regulariser kernel alone
    L = _lib.load()
    lp, sc = t(c["local_xyz"]), t(c["uv_scales"])
    n_part = L.gsr_uv_regularizers_partials(lp.shape[0])
    part = torch.empty((2 * n_part,), device=DEV)
    d_lp, d_sc = torch.empty_like(lp), torch.empty_like(sc)
    _lib.check(L.gsr_uv_regularizers(lp.shape[0], lp.data_ptr(), sc.data_ptr(), reg["threshold_local_xyz"],
                                     reg["lambda_local_xyz"], reg["threshold_scale"], reg["lambda_local_scale"],
                                     part.data_ptr(), d_lp.data_ptr(), d_sc.data_ptr(),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gsr_uv_regularizers")
    torch.cuda.synchronize()
    assert d_lp.abs().max().item() > 0 and d_sc.abs().max().item() > 0
    assert abs(loss1.item() - (loss0.item() + part.sum().item())) <= 1e-6 * abs(loss1.item())
    for name, d in (("local_pos", d_lp), ("uv_scales", d_sc)):
        want = g0[name].reshape(d.shape) + d
        err = ((g1[name].reshape(d.shape) - want).abs().max() / want.abs().max()).item()
        print(f"  {name}: {err:.3g} of max")
        assert err <= 1e-6, name
        assert (g1[name].reshape(d.shape) - g0[name].reshape(d.shape)).abs().max().item() > 0
    for name in plain.LEAVES:
        if name not in ("local_pos", "uv_scales"):
            # (untouched by reg; two backward runs differ in the last bits of render_bwd's atomics)
            assert ((g1[name] - g0[name]).abs().max() / g0[name].abs().max().clamp_min(1e-30)).item() <= 1e-4, name
    # mask and boxes reach the posed trainer too
    mask = torch.rand((Bn, 1, Wt, Wt), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    boxes = torch.tensor([[[10, 50, 4, 40]] * Bn, [[5, 20, 30, 47]] * Bn, [[40, 60, 35, 64]] * Bn])
    tr = AvatarTrainer(va, ua, t(c["faces"]), Bn, Wt, Wt, R_capacity=64 * P * Bn, device=DEV, apply_rgb_sigmoid=False,
                       reg=reg, crop_size=16)
    loss2, g2 = tr.gradients(verts, T, views, projs, tanf, target, mask=mask, boxes=boxes, mask_refined=True)
    feat = tr.rast.out_color.detach()
    want = tr.loss(feat, target, mask=mask, boxes=boxes, mask_refined=True) + part.sum()
    assert abs(loss2.item() - want.item()) <= 1e-5 * abs(want.item())
    assert torch.isfinite(tr.step(verts, T, views, projs, tanf, target, mask=mask, boxes=boxes))
