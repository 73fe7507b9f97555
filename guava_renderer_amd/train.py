"""Rasterizer training step (BASELINE config 4): forward + backward raster + fused-SSIM loss.

One step over the B frames of this rank (main/trainer.py:82-102 does, per iteration: render the
batch, Optimization_Loss, fabric.backward -> DDP gradient all-reduce, Adam step):
  1. BatchRasterizer.forward of the shared Gaussian attributes for B cameras (one launch set);
  2. loss = (1 - lambda) * L1 + lambda * (1 - fused_ssim) of the raw RGB channels + L1 of a refined image
     made from ALL 32 channels (the reference's `renders` term, :92; its StyleUNet refiner is out
     of scope, so a fixed random 1x1 conv 32 -> 3 stands in), so every feature channel carries a
     gradient into the rasterizer backward as in the reference's training; the L1 terms and the
     gradient assembly are one gfx950 pass (gsr_image_loss).  The reference's raw_renders term
     (utils/loss_utils.py:116-119) is lambda_l1 * L1 + an LPIPS perceptual term; LPIPS (AlexNet with
     weights fetched from a URL) is out of scope, and fused-SSIM -- the reference's own native loss
     kernel, BASELINE config 4 -- stands in for that perceptual term;
  3. BatchRasterizer.backward(shared=True) (render_bwd + cov/preprocess backward kernels) -> the
     shared attributes' gradients [P,k], summed over the frames inside the kernels (no [B,P,k]
     buffers);
  4. world > 1: ONE flat RCCL all-reduce of those gradients (parallel.reduce_shared_grads; the
     reference's DDP all-reduce, trainer.py:40-43,95), averaged over ranks;
  5. Adam on the attributes (fused Adam).
Capacity overflow (more Gaussian-tile instances than the workspace holds, e.g. after the attributes
drifted under the optimizer) needs no host synchronisation to stay harmless: the overflowing
forward renders NaN frames (so the step's loss is NaN), the backward produces no gradient, and the
workspace's overflow flag is the optimizer's `found_inf`, so Adam skips that step on the device
(as GradScaler does for an inf).  The next step sees the flag through the asynchronous status copy,
grows the workspace and counts the step in `skipped_steps`.
The reference trains networks that predict the Gaussians; those networks are out of scope here
(SURVEY.md 2.1), so the trainable parameters are the Gaussian attributes themselves -- the
rasterizer-side work of the step (fwd, bwd, SSIM, all-reduce, update) is the same.
AvatarTrainer is the posed-avatar counterpart: its leaves are GUAVA's canonical attributes, seen
through B poses (deform -> forward -> the same loss -> BatchRasterizer.backward_deformed -> the same
all-reduce, overflow handling and Adam).
GUAVA's further loss terms (utils/loss_utils.py:89-159) are optional arguments of gradients() / step():
`mask` (the target, and with mask_refined the refined image, become x * mask + (1 - mask) * loss_bg),
`boxes` (the head / left-hand / right-hand crops, resampled to crop_size and weighted by
crop_weights; each image's crop term carries the same L1 / SSIM weights as its frame term) and, for
AvatarTrainer, `reg` (the UV-Gaussian regularisers).  They run in csrc/loss.hip (include/gsr_loss.h);
with all of them left at None the step is the code path above, unchanged.
"""
import ctypes
import os
import warnings

import torch
import torch.distributed as dist

from . import _lib, parallel
from .batch import BatchRasterizer
from .fused_ssim import FusedSSIMMap, fused_ssim

C = 32


class SplatTrainer:
    def __init__(self, params, B, W, H, R_capacity, device="cuda", lr=1e-3, lambda_ssim=0.2, refine_head=True,
                 numerics=0, crop_weights=(0.25, 0.1, 0.1), crop_size=256, crop_ssim=True, loss_bg=0.0):
        """World-space Gaussians, identical in all B frames (a posed avatar: AvatarTrainer).
        params: dict of float32 device tensors means3D [P,3], colors [P,32], opacities [P,1], scales [P,3], rotations [P,4] (made leaves with requires_grad).  refine_head=False: the loss
        sees the RGB channels only.  numerics: the rasterizer calls' GSR_NUMERICS_* flags.
        crop_weights / crop_size / crop_ssim / loss_bg: the crop groups' weights (GUAVA's lambda_l1 *
        lambda_head_crop, lambda_l1 * lambda_hand_crop twice), the crops' resampled size, whether
        lambda_ssim applies to the raw image's crops as it does to its frame, and the mask's background."""
        self.dev = torch.device(device)
        self.p = {k: v.detach().clone().contiguous().requires_grad_(True) for k, v in params.items()}
        P = self.p["means3D"].shape[0]
        self.numerics = int(numerics)
        self.rast = BatchRasterizer(B, P, W, H, R_capacity=R_capacity, device=self.dev, numerics=self.numerics)
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr, fused=True)
        self.skipped_steps = 0
        self.B, self.W, self.H = B, W, H
        self.lambda_ssim = lambda_ssim
        self.bg = torch.zeros((B, C), dtype=torch.float32, device=self.dev)
        self.dinv = torch.zeros((B, H, W), dtype=torch.float32, device=self.dev)  # materialised, as autograd does
        g = torch.Generator().manual_seed(11)
        self.refine_w = ((torch.rand((3, C), generator=g) * 2 - 1) / C ** 0.5).to(self.dev) if refine_head else None
        self.shared_backward = os.environ.get("GSR_TRAIN_PERFRAME") != "1"  # "1": per-frame grads + sum (A/B)
        self._loss_bufs = None  # (per-workgroup loss partials, dL/dfeatures [B,32,H,W])
        self._init_guava_loss(crop_weights, crop_size, crop_ssim, loss_bg)

    def _init_guava_loss(self, crop_weights, crop_size, crop_ssim, loss_bg):
        self.crop_weights_host = tuple(float(w) for w in crop_weights)
        self.crop_weights = torch.tensor(self.crop_weights_host, dtype=torch.float32, device=self.dev)
        self.crop_size, self.crop_ssim, self.loss_bg = int(crop_size), bool(crop_ssim), float(loss_bg)
        self._guava_bufs = None

    def _grow(self, err):
        """An earlier step overflowed (and was skipped on the device): grow the workspace to 1.5x the
        instance count that step needed (at least double)."""
        self.skipped_steps += 1
        old = self.rast
        cap = max(int(old.max_instances_seen() * 1.5), 2 * old.R_capacity) + 1024
        warnings.warn(f"{type(self).__name__}: {err}; step skipped, R capacity {old.R_capacity} -> {cap}")
        self.rast = BatchRasterizer(old.B, old.P, old.W, old.H, R_capacity=cap, device=self.dev,
                                    numerics=self.numerics)
        del old

    def _begin_step(self, target):
        """Check the target and fold an earlier step's overflow report into a larger workspace."""
        want = (self.B, 3, self.H, self.W)
        if tuple(target.shape) != want or target.device != self.dev:
            raise ValueError(f"target: expected {list(want)} on {self.dev}, got {list(target.shape)} on {target.device}")
        try:
            self.rast.poll()
        except _lib.CapacityError as e:
            self._grow(e)

    def _loss_and_image_grad(self, col, target):
        """(loss, dL/dfeatures [B,32,H,W]) of the rendered features `col`: the SSIM term through
        autograd (fused_ssim kernels); the two L1 terms, their gradient and the SSIM gradient's
        addition in one pass over the 32-channel frames (gsr_image_loss)."""
        img = col[:, :3].detach().requires_grad_(True)
        ssim_term = self.lambda_ssim * (1.0 - fused_ssim(img, target))
        ssim_term.backward()
        tgt = target.detach().to(torch.float32).contiguous()
        B, _, H, W = col.shape
        L = _lib.load()
        n_part = L.gsr_image_loss_partials(B, H, W)
        if self._loss_bufs is None or self._loss_bufs[0].shape[0] != n_part:
            self._loss_bufs = (torch.empty((n_part,), dtype=torch.float32, device=self.dev),
                               torch.empty_like(col))
        part, dL = self._loss_bufs
        _lib.check(L.gsr_image_loss(B, H, W, col.data_ptr(), tgt.data_ptr(),
                                    self.refine_w.data_ptr() if self.refine_w is not None else None,
                                    1.0 - self.lambda_ssim, 1.0 if self.refine_w is not None else 0.0,
                                    img.grad.contiguous().data_ptr(), dL.data_ptr(), part.data_ptr(),
                                    ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)),
                   "gsr_image_loss")
        return (ssim_term.detach() + part.sum()).detach(), dL

    BOX_KEYS = ("head_box", "left_hand_box", "right_hand_box")  # a GUAVA batch's fields, in crop_weights' order

    def _check_guava_args(self, mask, boxes):
        """(mask float32 [B,1,H,W] or None, boxes int32 [G,B,4] on the device or None)."""
        if mask is not None:
            if tuple(mask.shape) != (self.B, 1, self.H, self.W) or mask.device != self.dev:
                raise ValueError(f"mask: expected {[self.B, 1, self.H, self.W]} on {self.dev}, got "
                                 f"{list(mask.shape)} on {mask.device}")
            mask = mask.detach().to(torch.float32).contiguous()
        if boxes is not None:
            if isinstance(boxes, dict):
                boxes = torch.stack([torch.as_tensor(boxes[k]).to(self.dev) for k in self.BOX_KEYS])
            G = self.crop_weights.shape[0]
            if tuple(boxes.shape) != (G, self.B, 4) or boxes.dtype.is_floating_point:
                raise ValueError(f"boxes: expected integers {[G, self.B, 4]} (one group per crop weight), got "
                                 f"{boxes.dtype} {list(boxes.shape)}")
            # (the kernels clamp to the image; this clamp only keeps an int64 inside int32)
            boxes = boxes.to(self.dev).clamp(0, max(self.H, self.W)).to(torch.int32).contiguous()
        return mask, boxes

    def _guava_loss_and_image_grad(self, col, target, mask, boxes, mask_refined):
        """_loss_and_image_grad with GUAVA's mask and crop terms (include/gsr_loss.h): the forward
        passes, the SSIM terms on the frame and on the raw image's resampled crops (fused_ssim), then
        the one pass that writes dL/dfeatures."""
        mask, boxes = self._check_guava_args(mask, boxes)
        L = _lib.load()
        B, _, H, W = col.shape
        G, S = (0, 0) if boxes is None else (boxes.shape[0], self.crop_size)
        K = 2 if self.refine_w is not None else 1
        key = (B, H, W, G, S, K)
        if self._guava_bufs is None or self._guava_bufs[0] != key:
            f32 = dict(dtype=torch.float32, device=self.dev)
            n_ws = L.gsr_guava_loss_workspace_bytes(B, H, W, G, S) // 4
            n_part = L.gsr_guava_loss_partials(B, H, W, G, S)
            if n_ws == 0 or n_part == 0:
                raise ValueError(f"loss sizes out of range: B {B} H {H} W {W} groups {G} crop_size {S}")
            self._guava_bufs = (key, torch.empty((n_ws,), **f32), torch.empty((n_part,), **f32),
                                torch.empty_like(col), torch.zeros((K, G, B, 3, S, S), **f32),
                                torch.zeros((G, B, 3, S, S), **f32),
                                torch.zeros((K, G, B, 3, S, S), **f32),
                                torch.zeros((max(G, 1),), dtype=torch.int32, device=self.dev))
        _, ws, part, dL, crops, crops_t, crops_g, n_valid = self._guava_bufs
        use_crops = G > 0 and self.crop_ssim and self.lambda_ssim != 0.0
        tgt = target.detach().to(torch.float32).contiguous()
        rw = self.refine_w.data_ptr() if self.refine_w is not None else None
        l1w, rfw = 1.0 - self.lambda_ssim, 1.0 if self.refine_w is not None else 0.0
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        _lib.check(L.gsr_guava_loss_forward(B, H, W, col.data_ptr(), tgt.data_ptr(), rw, l1w, rfw, ptr(mask),
                                            self.loss_bg, int(bool(mask_refined)), G, S, ptr(boxes),
                                            self.crop_weights.data_ptr(), crops.data_ptr() if use_crops else None,
                                            crops_t.data_ptr() if use_crops else None,
                                            n_valid.data_ptr() if use_crops else None, part.data_ptr(),
                                            ws.data_ptr(), stream), "gsr_guava_loss_forward")
        t = tgt if mask is None else ws[:B * 9 * H * W].view(B, 9, H, W)[:, 6:9].contiguous()
        img = col[:, :3].detach().requires_grad_(True)
        ssim_term = self.lambda_ssim * (1.0 - fused_ssim(img, t))
        if use_crops:
            ci = crops[0].reshape(G * B, 3, S, S).requires_grad_(True)
            smap = FusedSSIMMap.apply(0.01 ** 2, 0.03 ** 2, ci, crops_t.view(G * B, 3, S, S), "same", True)
            # a skipped slot is zero against zero: its map is 1, so it adds nothing to the sum
            per_group = (1.0 - smap.view(G, B, -1).mean(-1)).sum(-1) / n_valid.clamp_min(1).to(torch.float32)
            ssim_term = ssim_term + self.lambda_ssim * (self.crop_weights * per_group).sum()
        ssim_term.backward()
        if use_crops:
            crops_g[0].copy_(ci.grad.view(G, B, 3, S, S))
        _lib.check(L.gsr_guava_loss_backward(B, H, W, rw, l1w, rfw, ptr(mask), int(bool(mask_refined)), G, S,
                                             ptr(boxes), crops_g.data_ptr() if use_crops else None,
                                             img.grad.contiguous().data_ptr(), dL.data_ptr(), ws.data_ptr(), stream),
                   "gsr_guava_loss_backward")
        return (ssim_term.detach() + part.sum()).detach(), dL

    def _step_loss(self, col, target, mask, boxes, mask_refined):
        if mask is None and boxes is None:
            return self._loss_and_image_grad(col, target)
        return self._guava_loss_and_image_grad(col, target, mask, boxes, mask_refined)

    def gradients(self, views, projs, tanf, target, mask=None, boxes=None, mask_refined=False):
        """Forward + loss + backward of one step: (loss, dict of the attributes' gradients summed
        over this rank's frames), before any all-reduce or update.  mask [B,1,H,W], boxes (a dict
        with BOX_KEYS or an integer tensor [G,B,4] of left, right, top, bottom) and mask_refined:
        GUAVA's mask and crop terms (the module's docstring); None: the whole-frame loss alone."""
        self._begin_step(target)
        p = self.p
        col, _, _ = self.rast.forward(p["means3D"].detach(), p["colors"].detach(), p["opacities"].detach(),
                                      p["scales"].detach(), p["rotations"].detach(), views, projs, tanf,
                                      self.bg)
        loss, dL = self._step_loss(col, target, mask, boxes, mask_refined)
        g = self.rast.backward(p["means3D"].detach(), p["colors"].detach(), p["opacities"].detach(),
                               p["scales"].detach(), p["rotations"].detach(), views, projs, tanf, self.bg,
                               dL, self.dinv, shared=self.shared_backward)
        if not self.shared_backward:
            g = {k: v.sum(0) for k, v in g.items() if v is not None and v.dim() == 3}
        grads = {"means3D": g["means3D"], "colors": g["colors"], "opacities": g["opacity"],
                 "scales": g["scales"], "rotations": g["rotations"]}
        return loss, grads

    def rgb_loss(self, img, target):
        """(1 - lambda) L1 + lambda (1 - SSIM) of the raw RGB channels [B,3,H,W]."""
        return (1.0 - self.lambda_ssim) * (img - target).abs().mean() + \
            self.lambda_ssim * (1.0 - fused_ssim(img, target))

    def _host_boxes(self, boxes):
        """boxes (dict or [G,B,4]) as nested lists of clamped (left, right, top, bottom), None where
        skipped (the torch restatement reads the boxes on the host; boxes given on the CPU cost no sync)."""
        if isinstance(boxes, dict):
            boxes = torch.stack([torch.as_tensor(boxes[k]).cpu() for k in self.BOX_KEYS])
        out = []
        for rows in boxes.cpu().tolist():
            out.append([])
            for l, r, t, bo in rows:
                l, r = min(max(l, 0), self.W), min(max(r, 0), self.W)
                t, bo = min(max(t, 0), self.H), min(max(bo, 0), self.H)
                out[-1].append((l, r, t, bo) if r > l and bo > t else None)
        return out

    def _crop_pairs(self, image, target, rows):
        """The resampled cuts (image, target), each [n_valid,3,S,S], of one group's boxes (a row of
        _host_boxes), as the reference's cal_box_loss makes them; None when every box is skipped."""
        import torch.nn.functional as F
        S = (self.crop_size, self.crop_size)
        a, b = [], []
        for i, bx in enumerate(rows):
            if bx is not None:
                l, r, t, bo = bx
                a.append(F.interpolate(image[i:i + 1, :, t:bo, l:r], S, mode="bilinear"))
                b.append(F.interpolate(target[i:i + 1, :, t:bo, l:r], S, mode="bilinear"))
        return (torch.cat(a), torch.cat(b)) if a else None

    def loss(self, feat, target, mask=None, boxes=None, mask_refined=False):
        """The step's loss of rendered features [B,32,H,W] against RGB targets [B,3,H,W] (with the
        optional terms of gradients()), in torch."""
        if mask is None and boxes is None:
            loss = self.rgb_loss(feat[:, :3], target)
            if self.refine_w is not None:
                loss = loss + (torch.einsum("oc,bchw->bohw", self.refine_w, feat) - target).abs().mean()
            return loss
        t = target if mask is None else target * mask + (1.0 - mask) * self.loss_bg
        raw = feat[:, :3]
        loss = self.rgb_loss(raw, t)
        refined = None
        if self.refine_w is not None:
            refined = torch.einsum("oc,bchw->bohw", self.refine_w, feat)
            if mask is not None and mask_refined:
                refined = refined * mask + (1.0 - mask) * self.loss_bg
            loss = loss + (refined - t).abs().mean()
        for g, rows in enumerate([] if boxes is None else self._host_boxes(boxes)):
            w = float(self.crop_weights_host[g])
            pair = self._crop_pairs(raw, t, rows)
            if pair is None:
                continue
            loss = loss + w * (1.0 - self.lambda_ssim) * (pair[0] - pair[1]).abs().mean()
            if self.crop_ssim and self.lambda_ssim != 0.0:
                loss = loss + w * self.lambda_ssim * (1.0 - fused_ssim(pair[0], pair[1]))
            if refined is not None:
                pair = self._crop_pairs(refined, t, rows)
                loss = loss + w * (pair[0] - pair[1]).abs().mean()
        return loss

    def step(self, views, projs, tanf, target, mask=None, boxes=None, mask_refined=False):
        return self._update(*self.gradients(views, projs, tanf, target, mask=mask, boxes=boxes,
                                            mask_refined=mask_refined))

    def _update(self, loss, grads):
        """All-reduce (world > 1), this step's overflow as found_inf, fused Adam."""
        p = self.p
        # this step's capacity overflow, as the optimizer's found_inf (read on the device)
        ovf = self.rast.overflow_flag().to(torch.float32).reshape(1)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            grads["~overflow"] = ovf  # any rank's overflow skips the step on every rank
            parallel.reduce_shared_grads(grads)
            ovf = grads.pop("~overflow")
            for v in grads.values():
                v.div_(dist.get_world_size())
        for k, v in grads.items():
            p[k].grad = v.reshape(p[k].shape)
        self.opt.found_inf = (ovf > 0).to(torch.float32).reshape(())
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        return loss


class AvatarTrainer(SplatTrainer):
    """SplatTrainer's posed-avatar counterpart: the leaves are GUAVA's CANONICAL attributes -- vertex
    rotations and scales, UV local offsets, rotations and scales -- plus the colours and opacities,
    shared by the B frames of a step and seen through B poses.  A step is: EHM output in (verts
    [B,V,3], vert_transforms [B,V,4,4]), gsr_deform_gaussians, BatchRasterizer.forward, SplatTrainer's
    loss, BatchRasterizer.backward_deformed (the canonical gradients straight from the projection
    backward, no [B,P,k] attribute gradients), then SplatTrainer's all-reduce, overflow-as-found_inf
    and fused Adam.  The mesh gets no gradient (include/gsr_deform.h)."""

    LEAVES = ("vtx_rotations", "vtx_scales", "local_pos", "uv_rotations", "uv_scales", "colors", "opacities")
    # configs/train/ubody_512.yaml:46-58
    GUAVA_REG = dict(lambda_local_xyz=0.01, threshold_local_xyz=3.0, lambda_local_scale=1.0, threshold_scale=0.6)

    def __init__(self, vertex_gaussian_assets, uv_gaussian_assets, faces, B, W, H, R_capacity, device="cuda",
                 lr=1e-3, lambda_ssim=0.2, refine_head=True, numerics=0, apply_rgb_sigmoid=True,
                 crop_weights=(0.25, 0.1, 0.1), crop_size=256, crop_ssim=True, loss_bg=0.0, reg=None):
        """reg: None, or the UV-Gaussian regularisers' settings (GUAVA_REG holds GUAVA's: the keys
        lambda_local_xyz, threshold_local_xyz, lambda_local_scale, threshold_scale)."""
        from .deform import GaussianDeformer
        clone = lambda d: {k: v.detach().clone() for k, v in d.items()}  # noqa: E731 (the leaves are ours)
        dfm = GaussianDeformer(clone(vertex_gaussian_assets), clone(uv_gaussian_assets), faces,
                               apply_rgb_sigmoid=apply_rgb_sigmoid)
        self.deformer = dfm
        # the deformer's own tensors are the leaves: Adam updates them in place, the kernels read them
        leaves = dict(vtx_rotations=dfm.v_rot, vtx_scales=dfm.v_scale, local_pos=dfm.u_local,
                      uv_rotations=dfm.u_rot, uv_scales=dfm.u_scale, colors=dfm.colors, opacities=dfm.opacity)
        self.dev = torch.device(device)
        self.p = {k: leaves[k].requires_grad_(True) for k in self.LEAVES}
        P = dfm.V + dfm.N
        self.numerics = int(numerics)
        self.rast = BatchRasterizer(B, P, W, H, R_capacity=R_capacity, device=self.dev, numerics=self.numerics)
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr, fused=True)
        self.skipped_steps = 0
        self.B, self.W, self.H = B, W, H
        self.lambda_ssim = lambda_ssim
        self.bg = torch.zeros((B, C), dtype=torch.float32, device=self.dev)
        self.dinv = torch.zeros((B, H, W), dtype=torch.float32, device=self.dev)
        g = torch.Generator().manual_seed(11)
        self.refine_w = ((torch.rand((3, C), generator=g) * 2 - 1) / C ** 0.5).to(self.dev) if refine_head else None
        self._loss_bufs = None
        self._init_guava_loss(crop_weights, crop_size, crop_ssim, loss_bg)
        if reg is not None and set(reg) != set(self.GUAVA_REG):
            raise ValueError(f"reg: expected the keys {sorted(self.GUAVA_REG)}, got {sorted(reg)}")
        self.reg = None if reg is None else {k: float(v) for k, v in reg.items()}
        self._reg_bufs = None

    def _regularizers(self):
        """(loss, d local_pos, d uv_scales) of the UV-Gaussian regularisers (gsr_uv_regularizers)."""
        L = _lib.load()
        lp, sc = self.p["local_pos"].detach(), self.p["uv_scales"].detach()
        N = lp.shape[0]
        if self._reg_bufs is None:
            self._reg_bufs = (torch.empty((2 * L.gsr_uv_regularizers_partials(N),), dtype=torch.float32,
                                          device=self.dev), torch.empty_like(lp), torch.empty_like(sc))
        part, d_lp, d_sc = self._reg_bufs
        r = self.reg
        _lib.check(L.gsr_uv_regularizers(N, lp.data_ptr(), sc.data_ptr(), r["threshold_local_xyz"],
                                         r["lambda_local_xyz"], r["threshold_scale"], r["lambda_local_scale"],
                                         part.data_ptr(), d_lp.data_ptr(), d_sc.data_ptr(),
                                         ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)),
                   "gsr_uv_regularizers")
        return part.sum(), d_lp, d_sc

    def gradients(self, verts, vert_transforms, views, projs, tanf, target, mask=None, boxes=None,
                  mask_refined=False):
        """Deform + forward + loss + fused backward of one step: (loss, dict of the seven leaves'
        gradients summed over this rank's frames), before any all-reduce or update.  mask, boxes,
        mask_refined: as SplatTrainer.gradients; with `reg` set the regularisers' loss and their
        gradients of local_pos and uv_scales are added here (so before the all-reduce)."""
        self._begin_step(target)
        dfm = self.deformer
        with torch.no_grad():
            d = dfm(verts.detach(), vert_transforms.detach())
            col, _, _ = self.rast.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], views,
                                          projs, tanf, self.bg)
        loss, dL = self._step_loss(col, target, mask, boxes, mask_refined)
        g = self.rast.backward_deformed(dfm, verts, vert_transforms, d, dfm.colors.detach(), dfm.opacity.detach(),
                                        views, projs, tanf, self.bg, dL, self.dinv)
        g["opacities"] = g.pop("opacity")
        if self.reg is not None:
            reg_loss, d_lp, d_sc = self._regularizers()
            loss = loss + reg_loss
            g["local_pos"] = g["local_pos"] + d_lp.reshape(g["local_pos"].shape)
            g["uv_scales"] = g["uv_scales"] + d_sc.reshape(g["uv_scales"].shape)
        return loss, {k: g[k] for k in self.LEAVES}

    def step(self, verts, vert_transforms, views, projs, tanf, target, mask=None, boxes=None, mask_refined=False):
        return self._update(*self.gradients(verts, vert_transforms, views, projs, tanf, target, mask=mask,
                                            boxes=boxes, mask_refined=mask_refined))
