"""Batched multi-frame rasterization (gsr_forward_batch / gsr_backward_batch).

Replaces the per-frame Python loop of models/UbodyAvatar/gaussian_render.py:37-67: B frames
(views / poses) of one avatar go through one launch per stage with a preallocated workspace and
no host synchronisation, so a whole batch can also be captured in a HIP graph.  Per-frame
attributes may be shared (stride 0: a [P,k] tensor) or per frame (a [B,P,k] tensor).
"""
import ctypes
import weakref

import torch

from . import _lib

C = 32
STAGES = ("preprocess", "scan", "depth_sort", "chunk_count", "tile_scan", "ordered_scatter", "render_fwd",
          "render_bwd", "preprocess_bwd")


def _frame_arg(t, B, P, per, name, device, align16=False):
    """(tensor, element stride between frames) of a shared [P,per] or per-frame [B,P,per] float32
    input on `device`.  The frame stride is the tensor's own stride(0) -- 0 for an expanded tensor,
    whose frames all read one [P,per] table (deform.py's features_color / opacity); rows that are
    not dense in memory are made contiguous first.  align16: every frame's rows start 16-byte
    aligned (the render kernels' feature loads)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.device != device:
        raise ValueError(f"{name} must be on {device} (got {t.device})")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if t.dim() == 2:
        if tuple(t.shape) != (P, per):
            raise ValueError(f"{name}: expected [{P},{per}] or [{B},{P},{per}], got {list(t.shape)}")
        t = t.contiguous()
        return t, 0
    if t.dim() != 3 or tuple(t.shape) != (B, P, per):
        raise ValueError(f"{name}: expected [{P},{per}] or [{B},{P},{per}], got {list(t.shape)}")
    if t.stride(0) == 0:  # one table for every frame (expand)
        row = t[0]
        if not row.is_contiguous():
            row = row.contiguous()
        return row, 0
    dense_rows = t.stride(2) == 1 and (t.stride(1) == per or P == 1)
    fs = t.stride(0)
    if not dense_rows or fs < P * per or (align16 and (fs % 4 or t.data_ptr() % 16)):
        t = t.contiguous()
        fs = P * per
    return t, fs


def _frame_mat(t, B, n, name, device):
    """[B,n] float32 per-frame matrix (viewmatrices / projmatrices [B,16], tanfov [B,2])."""
    if t.device != device or t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 on {device}")
    if t.numel() != B * n:
        raise ValueError(f"{name}: expected {B}x{n} floats, got shape {list(t.shape)}")
    return t.contiguous()


class BatchRasterizer:
    """Holds the workspace for B frames of P Gaussians at W x H with room for R_capacity
    Gaussian-tile instances.

    Capacity: a forward whose batch needs more than R_capacity instances renders nothing (its
    images are NaN) and sets the workspace's sticky overflow word.  No host synchronisation is
    needed to notice it: after every forward the sticky words are copied asynchronously to pinned
    memory, and the next forward/backward (or poll()) raises CapacityError once that copy has
    landed; poll(wait=True) or status() check at once.

    numerics: the flag word of this rasterizer's calls (include/gsr.h GSR_NUMERICS_*, built by
    _lib.numerics()); 0, the default, is bit-identical to the CPU oracle.  A call may override it
    (forward / backward `numerics=`); nothing is process-wide."""

    def __init__(self, B, P, W, H, R_capacity=None, device="cuda", numerics=0):
        self.B, self.P, self.W, self.H = int(B), int(P), int(W), int(H)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.R_capacity = int(R_capacity if R_capacity is not None else 16 * P * B)
        self.numerics = int(numerics)
        self.L = _lib.load()
        nbytes = self.L.gsr_batch_workspace_bytes(self.B, self.P, self.W, self.H, self.R_capacity)
        soff = self.L.gsr_batch_status_offset(self.B, self.P, self.W, self.H, self.R_capacity)
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        self._sticky = self.workspace[soff:soff + 16].view(torch.int32)  # include/gsr.h sticky words
        self._sticky.zero_()
        self._overflow = self.workspace[4:8].view(torch.int32).reshape(())  # this call's flag (kCtrlOverflow)
        self._status_host = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        self._status_ev = None
        self._fwd_count = 0  # forwards enqueued on the (single-use) workspace
        self.out_color = torch.empty((self.B, C, self.H, self.W), dtype=torch.float32, device=self.device)
        self.out_invdepth = torch.empty((self.B, self.H, self.W), dtype=torch.float32, device=self.device)
        self.radii = torch.empty((self.B, self.P), dtype=torch.int32, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _inputs(self, means3D, colors, opacities, scales, rotations, viewmatrices, projmatrices,
                tanfov, backgrounds):
        B, P, dev = self.B, self.P, self.device
        none = (None, 0)  # geometry the fused avatar forward assembles on the device
        m, sm = none if means3D is None else _frame_arg(means3D, B, P, 3, "means3D", dev)
        c, sc = _frame_arg(colors, B, P, C, "colors", dev, align16=True)
        o, so = _frame_arg(opacities, B, P, 1, "opacities", dev)
        s, ss = none if scales is None else _frame_arg(scales, B, P, 3, "scales", dev)
        r, sr = none if rotations is None else _frame_arg(rotations, B, P, 4, "rotations", dev)
        v = _frame_mat(viewmatrices, B, 16, "viewmatrices", dev)
        pm = _frame_mat(projmatrices, B, 16, "projmatrices", dev)
        tf = _frame_mat(tanfov, B, 2, "tanfov", dev)
        if backgrounds.device != dev or backgrounds.dtype != torch.float32:
            raise ValueError(f"backgrounds must be float32 on {dev}")
        if backgrounds.dim() == 2:
            if tuple(backgrounds.shape) != (B, C):
                raise ValueError(f"backgrounds: expected [{C}] or [{B},{C}], got {list(backgrounds.shape)}")
            bg = backgrounds.contiguous() if backgrounds.stride(0) != 0 else backgrounds[0].contiguous()
            bs = C if backgrounds.stride(0) != 0 else 0
        elif tuple(backgrounds.shape) == (C,):
            bg, bs = backgrounds.contiguous(), 0
        else:
            raise ValueError(f"backgrounds: expected [{C}] or [{B},{C}], got {list(backgrounds.shape)}")
        keep = (m, c, o, s, r, v, pm, tf, bg)  # alive until the launches are enqueued
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        args = (B, P, self.W, self.H, ptr(m), sm, c.data_ptr(), sc, o.data_ptr(), so, ptr(s), ss, ptr(r), sr)
        return keep, args, (v.data_ptr(), pm.data_ptr(), tf.data_ptr(), bg.data_ptr(), bs)

    def _after_forward(self):
        """Queue the asynchronous copy of the sticky status words (no host synchronisation)."""
        self._fwd_count += 1
        self._status_host.copy_(self._sticky, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._status_ev = ev

    def poll(self, wait=False):
        """Raise CapacityError if a forward enqueued so far overflowed the capacity.  Without
        `wait` this only reads the status copy of the forwards that have already completed."""
        ev = self._status_ev
        if ev is None:
            return
        if wait:
            ev.synchronize()
        elif not ev.query():
            return
        if int(self._status_host[0]):
            rmax = int(self._status_host[1]) & 0xFFFFFFFF
            self.overflow_need = max(getattr(self, "overflow_need", 0), rmax)
            self._sticky.zero_()
            self._status_host.zero_()
            raise _lib.CapacityError(
                f"batch needed {rmax} Gaussian-tile instances, workspace holds {self.R_capacity} "
                f"(that forward's images are NaN); allocate a BatchRasterizer with a larger R_capacity")

    def max_instances_seen(self):
        """Largest batch instance count of the forwards whose status copy has landed (including
        the overflowing ones poll() reported)."""
        return max(int(self._status_host[1]) & 0xFFFFFFFF, getattr(self, "overflow_need", 0))

    def overflow_flag(self):
        """0-dim int32 device tensor: 1 if the last forward overflowed (read on the device, e.g. as an
        optimizer's found_inf), no host synchronisation."""
        return self._overflow

    def forward(self, means3D, colors, opacities, scales, rotations, viewmatrices, projmatrices,
                tanfov, backgrounds, scale_modifier=1.0, antialiasing=False, refine=None, numerics=None,
                forward_only=False):
        """Render B frames.  refine: optional RefineHead -- the refiner's first 1x1 conv + leaky ReLU
        fused into the render epilogue (include/gsr.h gsr_refine_epilogue); its output is
        refine.out [B,n_out,H,W] and only out_color[:, :refine.keep_channels] is written.
        forward_only: no backward() will follow (inference; include/gsr.h GSR_FORWARD_ONLY): the
        workspace skips the rows only the backward reads; the images are the same."""
        self.poll()
        nm = self.numerics if numerics is None else int(numerics)
        if forward_only:
            nm |= _lib.FORWARD_ONLY
        self._fwd_only = bool(forward_only)
        keep, head, (v, pm, tf, bg, bs) = self._inputs(means3D, colors, opacities, scales, rotations,
                                                       viewmatrices, projmatrices, tanfov, backgrounds)
        args = head + (float(scale_modifier), v, pm, tf, bg, bs, self.workspace.data_ptr(), self.R_capacity,
                       self.out_color.data_ptr(), self.out_invdepth.data_ptr(), self.radii.data_ptr(),
                       int(bool(antialiasing)))
        if refine is None:
            _lib.check(self.L.gsr_forward_batch(*args, nm, self._stream()), "gsr_forward_batch")
        else:
            # composite the pre-contracted rows (include/gsr.h gsr_refine_prepare): features and
            # backgrounds both go through the head's 32 -> keep + n_out map
            pc = refine.prepare(keep[1], self._stream())
            bgrows = keep[8].reshape(-1, C)
            pb = refine.prepare(bgrows, self._stream(), cache=False)
            args = list(args)
            args[6] = pc.data_ptr()
            args[18] = pb.data_ptr()
            ep = refine.epilogue(self.B, self.H, self.W)
            _lib.check(self.L.gsr_forward_batch_refine(*args, ctypes.byref(ep), nm, self._stream()),
                       "gsr_forward_batch_refine")
        del keep
        self._after_forward()
        return self.out_color, self.out_invdepth, self.radii

    def forward_deformed(self, deformer, verts, vert_transforms, viewmatrices, projmatrices, tanfov, backgrounds,
                         scale_modifier=1.0, antialiasing=False, numerics=None, refine=None):
        """The avatar pipeline's fused forward (include/gsr_deform.h gsr_forward_batch_deformed): the
        B frames of `deformer` (deform.GaussianDeformer) on the deformed mesh verts [B,V,3] /
        vert_transforms [B,V,4,4], rendered without materialising the deformed Gaussians (their
        assembly feeds the projection in registers).  Same images as deformer.forward() + forward();
        forward-only (a backward() after it raises).  refine: optional RefineHead, as forward()'s
        (gsr_forward_batch_deformed_refine): its output is refine.out and only
        out_color[:, :refine.keep_channels] is written."""
        self.poll()
        nm = self.numerics if numerics is None else int(numerics)
        self._fwd_only = True
        dfm = deformer
        B, P = self.B, self.P
        if dfm.V + dfm.N != P:
            raise ValueError(f"deformer has {dfm.V + dfm.N} Gaussians, the rasterizer {P}")
        if tuple(verts.shape) != (B, dfm.V, 3) or tuple(vert_transforms.shape) != (B, dfm.V, 4, 4):
            raise ValueError("verts / vert_transforms: expected [B,V,3] / [B,V,4,4]")
        # every pointer below goes straight to the kernel: a host (or other-device) tensor must not
        # reach it
        for name, t_ in (("verts", verts), ("vert_transforms", vert_transforms), ("deformer.faces", dfm.faces),
                         ("deformer.colors", dfm.colors), ("deformer.bind", dfm.bind)):
            if t_.device != self.device:
                raise ValueError(f"{name} is on {t_.device}, the rasterizer on {self.device}")
        vb = verts.detach().to(torch.float32).contiguous()
        vt = vert_transforms.detach().to(torch.float32).contiguous()
        keep, head, (v, pm, tf, bg, bs) = self._inputs(None, dfm.colors, dfm.opacity, None, None, viewmatrices,
                                                       projmatrices, tanfov, backgrounds)
        di = _lib.DeformInputs(dfm.V, dfm.faces.shape[0], dfm.N, 0, vb.data_ptr(), vt.data_ptr(),
                               dfm.faces.data_ptr(), dfm.v_rot.data_ptr(), 0, dfm.v_scale.data_ptr(), 0,
                               dfm.bind.data_ptr(), dfm.bary.data_ptr(), dfm.u_local.data_ptr(), 0,
                               dfm.u_rot.data_ptr(), 0, dfm.u_scale.data_ptr(), 0, dfm.bad.data_ptr())
        args = (B, self.W, self.H, ctypes.byref(di), head[6], head[7], head[8], head[9], float(scale_modifier),
                v, pm, tf, bg, bs, self.workspace.data_ptr(), self.R_capacity, self.out_color.data_ptr(),
                self.out_invdepth.data_ptr(), self.radii.data_ptr(), int(bool(antialiasing)))
        if refine is None:
            _lib.check(self.L.gsr_forward_batch_deformed(*args, nm, self._stream()), "gsr_forward_batch_deformed")
        else:
            # the pre-contracted rows, features and backgrounds alike (as forward(refine=head))
            pc = refine.prepare(keep[1], self._stream())
            pb = refine.prepare(keep[8].reshape(-1, C), self._stream(), cache=False)
            args = list(args)
            args[4] = pc.data_ptr()
            args[12] = pb.data_ptr()
            ep = refine.epilogue(B, self.H, self.W)
            _lib.check(self.L.gsr_forward_batch_deformed_refine(*args, ctypes.byref(ep), nm, self._stream()),
                       "gsr_forward_batch_deformed_refine")
        del keep, vb, vt
        self._after_forward()
        return self.out_color, self.out_invdepth, self.radii

    def backward(self, means3D, colors, opacities, scales, rotations, viewmatrices, projmatrices,
                 tanfov, backgrounds, dL_dcolor, dL_dinvdepth=None, scale_modifier=1.0,
                 antialiasing=False, shared=False, numerics=None):
        """Gradients of the last forward, per frame: dict of [B,P,k] tensors (all zero when that
        forward overflowed the capacity; the overflow is reported by the next forward / poll).
        shared=True (attributes shared by every frame, e.g. one avatar under B cameras): the
        attribute gradients summed over the frames instead, dict of [P,k] tensors (means3D, colors,
        opacity, scales, rotations) -- gsr_backward_batch_shared, no [B,P,k] buffers."""
        B, P = self.B, self.P
        if getattr(self, "_fwd_only", False):
            raise _lib.GsrError("backward after forward(forward_only=True): the workspace holds no backward rows")
        nm = self.numerics if numerics is None else int(numerics)
        o = dict(dtype=torch.float32, device=self.device)
        keep, head, (v, pm, tf, bg, bs) = self._inputs(means3D, colors, opacities, scales, rotations,
                                                       viewmatrices, projmatrices, tanfov, backgrounds)
        if tuple(dL_dcolor.shape) != (B, C, self.H, self.W):
            raise ValueError(f"dL_dcolor: expected [{B},{C},{self.H},{self.W}], got {list(dL_dcolor.shape)}")
        dLc = dL_dcolor.to(torch.float32).contiguous()
        dLi = None
        if dL_dinvdepth is not None:
            if dL_dinvdepth.numel() != B * self.H * self.W:
                raise ValueError("dL_dinvdepth: expected [B,H,W]")
            dLi = dL_dinvdepth.to(torch.float32).contiguous()
        if shared:
            # the frame-reduced kernels read ONE attribute row set: per-frame inputs would come back
            # as a single sum over distinct tensors, so they are refused here
            strides = head[5::2]  # means3D, colors, opacities, scales, rotations frame strides
            if any(st_ != 0 for st_ in strides):
                raise ValueError("backward(shared=True) needs attributes shared by every frame "
                                 "([P,k] tensors or frame stride 0); got per-frame inputs")
            g = dict(colors=torch.zeros((P, C), **o), opacity=torch.empty((P, 1), **o),
                     means3D=torch.empty((P, 3), **o), scales=torch.empty((P, 3), **o),
                     rotations=torch.empty((P, 4), **o))
            rc = self.L.gsr_backward_batch_shared(
                *head, float(scale_modifier), v, pm, tf, bg, bs, self.workspace.data_ptr(), self.R_capacity,
                dLc.data_ptr(), dLi.data_ptr() if dLi is not None else None, g["opacity"].data_ptr(),
                g["colors"].data_ptr(), g["means3D"].data_ptr(), g["scales"].data_ptr(),
                g["rotations"].data_ptr(), int(bool(antialiasing)), nm, self._stream())
            _lib.check(rc, "gsr_backward_batch_shared")
            del keep
            return g
        g = dict(mean2D=torch.zeros((B, P, 3), **o), conic=torch.zeros((B, P, 4), **o),
                 opacity=torch.zeros((B, P, 1), **o), colors=torch.zeros((B, P, C), **o),
                 invdepth=torch.zeros((B, P, 1), **o) if dL_dinvdepth is not None else None,
                 means3D=torch.zeros((B, P, 3), **o), cov3D=torch.zeros((B, P, 6), **o),
                 scales=torch.zeros((B, P, 3), **o), rotations=torch.zeros((B, P, 4), **o))
        rc = self.L.gsr_backward_batch(
            *head, float(scale_modifier), v, pm, tf, bg, bs, self.workspace.data_ptr(), self.R_capacity,
            dLc.data_ptr(), dLi.data_ptr() if dLi is not None else None,
            g["mean2D"].data_ptr(), g["conic"].data_ptr(), g["opacity"].data_ptr(),
            g["colors"].data_ptr(), g["invdepth"].data_ptr() if g["invdepth"] is not None else None,
            g["means3D"].data_ptr(), g["cov3D"].data_ptr(), g["scales"].data_ptr(),
            g["rotations"].data_ptr(), int(bool(antialiasing)), nm, self._stream())
        _lib.check(rc, "gsr_backward_batch")
        del keep
        return g

    def _bg_arg(self, backgrounds):
        """(rows [B,32] or [1,32], element stride between frames) of a [32] or [B,32] background."""
        if backgrounds.device != self.device or backgrounds.dtype != torch.float32:
            raise ValueError(f"backgrounds must be float32 on {self.device}")
        if tuple(backgrounds.shape) == (C,):
            return backgrounds.contiguous().reshape(1, C), 0
        if backgrounds.dim() != 2 or tuple(backgrounds.shape) != (self.B, C):
            raise ValueError(f"backgrounds: expected [{C}] or [{self.B},{C}], got {list(backgrounds.shape)}")
        if backgrounds.stride(0) == 0:
            return backgrounds[0].contiguous().reshape(1, C), 0
        return backgrounds.contiguous(), C

    def refine_backward_image(self, head, dL_drefined, dL_draw=None, out_refine=None):
        """The image end of the refine backward (include/gsr.h gsr_refine_backward_image): from
        dL/d(refined) [B,n_out,H,W] and optionally dL/d(kept raw channels) [B,keep,H,W] the gradient
        image in prepared channel space [B,32,H,W], the dL_dcolor of a backward() on head.prepare'd
        rows.  out_refine: the forward's refined output (default head.out, the last forward's).
        Returns (image, scratch); scratch goes to refine_backward_rows."""
        B, P, H, W = self.B, self.P, self.H, self.W
        if getattr(self, "_fwd_only", False):
            raise _lib.GsrError("backward after a forward-only forward: the workspace holds no backward rows")
        out = head.out if out_refine is None else out_refine
        if out is None or tuple(out.shape) != (B, head.n_out, H, W):
            raise ValueError(f"out_refine: expected the refine forward's [{B},{head.n_out},{H},{W}] output")
        if tuple(dL_drefined.shape) != (B, head.n_out, H, W):
            raise ValueError(f"dL_drefined: expected [{B},{head.n_out},{H},{W}], got {list(dL_drefined.shape)}")
        if out.device != self.device or dL_drefined.device != self.device:
            raise ValueError(f"out_refine / dL_drefined must be on {self.device}")
        out = out.to(torch.float32).contiguous()
        dout = dL_drefined.to(torch.float32).contiguous()
        dkeep = None
        if dL_draw is not None and head.keep_channels > 0:
            if tuple(dL_draw.shape) != (B, head.keep_channels, H, W) or dL_draw.device != self.device:
                raise ValueError(f"dL_draw: expected [{B},{head.keep_channels},{H},{W}] on {self.device}")
            dkeep = dL_draw.to(torch.float32).contiguous()
        # one scratch for both ends, whichever row layout (frame-reduced or per frame) follows
        nbytes = max(self.L.gsr_refine_backward_scratch_bytes(B, W, H, P, 1),
                     self.L.gsr_refine_backward_scratch_bytes(B, W, H, B * P, B))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        G = torch.empty((B, C, H, W), dtype=torch.float32, device=self.device)
        desc = _lib.RefineBackwardDesc(head.weight.data_ptr(), head.n_out, head.keep_channels, head.slope, 0,
                                       out.data_ptr(), dout.data_ptr(),
                                       dkeep.data_ptr() if dkeep is not None else None, G.data_ptr(),
                                       scratch.data_ptr())
        _lib.check(self.L.gsr_refine_backward_image(B, P, W, H, self.workspace.data_ptr(), self.R_capacity,
                                                    ctypes.byref(desc), self._stream()),
                   "gsr_refine_backward_image")
        del out, dout, dkeep
        return G, scratch

    def refine_backward_rows(self, head, d_prepared, raw_rows, backgrounds, scratch):
        """The row end of the refine backward (gsr_refine_backward_rows): d_prepared is the colour
        gradient of the backward on the prepared rows ([P,32] frame-reduced or [B,P,32]), raw_rows the
        raw features ([P,32] or [B,P,32]), backgrounds the raw ones.  Returns (gradient of the raw
        rows, shaped as d_prepared; weight gradient [n_out,32]; bias gradient [n_out])."""
        B, P, dev = self.B, self.P, self.device
        raw, rs = _frame_arg(raw_rows, B, P, C, "raw_rows", dev, align16=True)
        if d_prepared.dtype != torch.float32 or d_prepared.device != dev or \
                tuple(d_prepared.shape) not in ((P, C), (B, P, C)):
            raise ValueError(f"d_prepared: expected float32 [{P},{C}] or [{B},{P},{C}] on {dev}")
        frames = 1 if d_prepared.dim() == 2 else B
        if frames == 1 and rs != 0:
            raise ValueError("frame-reduced d_prepared [P,32] needs raw rows shared by every frame")
        dp = d_prepared.contiguous()
        bg, bs = self._bg_arg(backgrounds)
        need = self.L.gsr_refine_backward_scratch_bytes(B, self.W, self.H, dp.numel() // C, frames)
        if scratch.numel() < need:
            raise ValueError("scratch is not the one refine_backward_image returned for this rasterizer")
        o = dict(dtype=torch.float32, device=dev)
        rows = torch.empty_like(dp)
        dW = torch.empty((head.n_out, C), **o)
        db = torch.empty((head.n_out,), **o)
        desc = _lib.RefineBackwardDesc(head.weight.data_ptr(), head.n_out, head.keep_channels, head.slope, 0,
                                       None, None, None, None, scratch.data_ptr())
        _lib.check(self.L.gsr_refine_backward_rows(dp.numel() // C, frames, dp.data_ptr(), raw.data_ptr(), rs, B,
                                                   scratch.data_ptr(), bg.data_ptr(), bs, ctypes.byref(desc),
                                                   rows.data_ptr(), dW.data_ptr(), db.data_ptr(), self._stream()),
                   "gsr_refine_backward_rows")
        del raw, bg, dp
        return rows, dW, db

    def _prepared(self, head, colors, backgrounds):
        """(prepared colours, prepared backgrounds as backward() takes them) -- head.prepare's cached
        rows when `colors` is the tensor the forward prepared."""
        raw, _ = _frame_arg(colors, self.B, self.P, C, "colors", self.device, align16=True)
        bg, bs = self._bg_arg(backgrounds)
        pc = head.prepare(raw, self._stream())
        pb = head.prepare(bg, self._stream(), cache=False)
        return pc, (pb if bs else pb[0])

    def backward_refine(self, head, means3D, colors, opacities, scales, rotations, viewmatrices, projmatrices,
                        tanfov, backgrounds, dL_drefined, dL_draw=None, dL_dinvdepth=None, scale_modifier=1.0,
                        antialiasing=False, shared=False, numerics=None, out_refine=None):
        """Gradients of the last forward(..., refine=head): the arguments of backward() with the image
        gradient split into dL_drefined [B,n_out,H,W] (of head.out) and the optional dL_draw
        [B,keep,H,W] (of out_color[:, :keep]).  Returns backward()'s dict with `colors` the gradient of
        the RAW features, plus `weight` [n_out,32] and `bias` [n_out] of the head.  The 32-channel
        feature image is never formed: the image gradient is mapped into the prepared channel space
        (refine_backward_image), the ordinary backward runs on the prepared rows, and
        refine_backward_rows maps its colour gradient back and contracts the weight gradient."""
        G, scratch = self.refine_backward_image(head, dL_drefined, dL_draw, out_refine)
        pc, pb = self._prepared(head, colors, backgrounds)
        g = self.backward(means3D, pc, opacities, scales, rotations, viewmatrices, projmatrices, tanfov, pb, G,
                          dL_dinvdepth, scale_modifier=scale_modifier, antialiasing=antialiasing, shared=shared,
                          numerics=numerics)
        g["colors"], g["weight"], g["bias"] = self.refine_backward_rows(head, g["colors"], colors, backgrounds,
                                                                        scratch)
        return g

    def backward_deformed(self, deformer, verts, vert_transforms, deformed, colors, opacities, viewmatrices,
                          projmatrices, tanfov, backgrounds, dL_dcolor=None, dL_dinvdepth=None, scale_modifier=1.0,
                          antialiasing=False, numerics=None, refine=None, dL_drefined=None, dL_draw=None):
        """Gradients of the last forward() of a posed avatar with respect to its CANONICAL attributes
        (include/gsr_deform.h gsr_backward_batch_deformed): `deformer` (deform.GaussianDeformer) holds
        the shared canonical attributes, `deformed` is the dict its forward(verts, vert_transforms)
        returned and forward() rendered from ('xyz', 'rotation', 'scaling' [B,P,k]); colors [P,32] and
        opacities [P,1] are shared by the frames.  Returns a dict of the seven gradients summed over
        the frames: vtx_rotations [V,4], vtx_scales [V,3], local_pos [N,3], uv_rotations [N,4],
        uv_scales [N,3], colors [P,32], opacity [P,1].  The per-frame [B,P,k] attribute gradients are
        never written.  verts / vert_transforms get no gradient.
        refine=head, dL_drefined= (and optionally dL_draw=) instead of dL_dcolor: the forward was
        forward(..., refine=head); as backward_refine, `colors` comes back as the gradient of the raw
        features and `weight`, `bias` of the head are added."""
        if refine is not None:
            if dL_drefined is None or dL_dcolor is not None:
                raise ValueError("backward_deformed(refine=head) takes dL_drefined (and dL_draw), not dL_dcolor")
            G, scratch = self.refine_backward_image(refine, dL_drefined, dL_draw)
            pc, pb = self._prepared(refine, colors, backgrounds)
            g = self.backward_deformed(deformer, verts, vert_transforms, deformed, pc, opacities, viewmatrices,
                                       projmatrices, tanfov, pb, G, dL_dinvdepth, scale_modifier=scale_modifier,
                                       antialiasing=antialiasing, numerics=numerics)
            g["colors"], g["weight"], g["bias"] = self.refine_backward_rows(refine, g["colors"], colors, backgrounds,
                                                                            scratch)
            return g
        if dL_dcolor is None:
            raise ValueError("backward_deformed needs dL_dcolor (or refine= and dL_drefined=)")
        B, P, dfm = self.B, self.P, deformer
        if getattr(self, "_fwd_only", False):
            raise _lib.GsrError("backward after a forward-only forward: the workspace holds no backward rows")
        if dfm.V + dfm.N != P:
            raise ValueError(f"deformer has {dfm.V + dfm.N} Gaussians, the rasterizer {P}")
        if tuple(verts.shape) != (B, dfm.V, 3) or tuple(vert_transforms.shape) != (B, dfm.V, 4, 4):
            raise ValueError("verts / vert_transforms: expected [B,V,3] / [B,V,4,4]")
        for name, t_ in (("verts", verts), ("vert_transforms", vert_transforms), ("deformer.faces", dfm.faces)):
            if t_.device != self.device:
                raise ValueError(f"{name} is on {t_.device}, the rasterizer on {self.device}")
        nm = self.numerics if numerics is None else int(numerics)
        o = dict(dtype=torch.float32, device=self.device)
        keep, head, (v, pm, tf, bg, bs) = self._inputs(deformed["xyz"], colors, opacities, deformed["scaling"],
                                                       deformed["rotation"], viewmatrices, projmatrices, tanfov,
                                                       backgrounds)
        full = (3 * P, 0, 0, 3 * P, 4 * P)  # means3D, colors, opacities, scales, rotations frame strides
        if tuple(head[5::2]) != full:
            raise ValueError("backward_deformed needs deformed attributes [B,P,k] and colors / opacities shared "
                             "by every frame ([P,k] tensors or frame stride 0)")
        if tuple(dL_dcolor.shape) != (B, C, self.H, self.W):
            raise ValueError(f"dL_dcolor: expected [{B},{C},{self.H},{self.W}], got {list(dL_dcolor.shape)}")
        dLc = dL_dcolor.to(torch.float32).contiguous()
        dLi = None
        if dL_dinvdepth is not None:
            if dL_dinvdepth.numel() != B * self.H * self.W:
                raise ValueError("dL_dinvdepth: expected [B,H,W]")
            dLi = dL_dinvdepth.to(torch.float32).contiguous()
        vb = verts.detach().to(torch.float32).contiguous()
        vt = vert_transforms.detach().to(torch.float32).contiguous()
        di = _lib.DeformInputs(dfm.V, dfm.faces.shape[0], dfm.N, 0, vb.data_ptr(), vt.data_ptr(),
                               dfm.faces.data_ptr(), dfm.v_rot.data_ptr(), 0, dfm.v_scale.data_ptr(), 0,
                               dfm.bind.data_ptr(), dfm.bary.data_ptr(), dfm.u_local.data_ptr(), 0,
                               dfm.u_rot.data_ptr(), 0, dfm.u_scale.data_ptr(), 0, dfm.bad.data_ptr())
        g = dict(vtx_rotations=torch.zeros((dfm.V, 4), **o), vtx_scales=torch.zeros((dfm.V, 3), **o),
                 local_pos=torch.zeros((dfm.N, 3), **o), uv_rotations=torch.zeros((dfm.N, 4), **o),
                 uv_scales=torch.zeros((dfm.N, 3), **o), colors=torch.zeros((P, C), **o),
                 opacity=torch.zeros((P, 1), **o))
        dgr = _lib.DeformGrads(g["vtx_rotations"].data_ptr(), g["vtx_scales"].data_ptr(), g["local_pos"].data_ptr(),
                               g["uv_rotations"].data_ptr(), g["uv_scales"].data_ptr())
        rc = self.L.gsr_backward_batch_deformed(
            B, self.W, self.H, ctypes.byref(di), head[4], head[12], head[10], head[6], 0, head[8], 0,
            float(scale_modifier), v, pm, tf, bg, bs, self.workspace.data_ptr(), self.R_capacity, dLc.data_ptr(),
            dLi.data_ptr() if dLi is not None else None, g["opacity"].data_ptr(), g["colors"].data_ptr(),
            ctypes.byref(dgr), int(bool(antialiasing)), nm, self._stream())
        _lib.check(rc, "gsr_backward_batch_deformed")
        del keep, vb, vt
        return g

    def status(self):
        """(R_total, overflow) of the last forward; synchronises the stream."""
        R = ctypes.c_int64(0)
        ovf = ctypes.c_int(0)
        _lib.check(self.L.gsr_batch_status(self.workspace.data_ptr(), self.B, self.P,
                                           ctypes.byref(R), ctypes.byref(ovf), self._stream()),
                   "gsr_batch_status")
        return int(R.value), bool(ovf.value)


class RefineHead:
    """StyleUNet.conv_body_first (nn.Conv2d(32, n_out, 1), styleunet.py:110) + F.leaky_relu_(., 0.2)
    (:178), evaluated inside the render kernel.  weight [n_out,32] or [n_out,32,1,1], bias [n_out]."""

    def __init__(self, weight, bias=None, negative_slope=0.2, keep_channels=4):
        w = weight.detach().reshape(weight.shape[0], -1).to(torch.float32).contiguous()
        assert w.shape[1] == C and 1 <= w.shape[0] <= C, w.shape
        self.weight = w
        self.bias = bias.detach().to(torch.float32).contiguous() if bias is not None else None
        self.n_out = w.shape[0]
        self.slope = float(negative_slope)
        self.keep_channels = int(keep_channels)
        assert self.keep_channels + self.n_out <= C
        self.out = None
        self._outs = {}
        self._prep_key, self._prep = None, None

    @classmethod
    def from_conv(cls, conv, negative_slope=0.2, keep_channels=4):
        return cls(conv.weight, conv.bias, negative_slope, keep_channels)

    def prepare(self, rows, stream, cache=True):
        """[..., 32] feature rows -> the pre-contracted rows the refine epilogue composites.  Cached
        for the same tensor OBJECT at the same version (an avatar's features are static across
        frames): a different tensor -- even one the allocator placed at the same address -- or an
        in-place torch update is recomputed.  Writes that bypass torch's version counter (a HIP
        kernel writing through data_ptr()) need invalidate()."""
        # identity: the tensor that owns the memory (a view's base) -- alive while the weakref is,
        # so its address cannot be reused -- plus the view's address, shape and the version counter
        owner = rows._base if rows._base is not None else rows
        ident = (rows.data_ptr(), tuple(rows.shape), rows._version)
        if cache and self._prep_key is not None:
            ref, key = self._prep_key
            if ref() is owner and key == ident:
                return self._prep
        out = torch.empty_like(rows)
        n = rows.numel() // C
        _lib.check(_lib.load().gsr_refine_prepare(n, rows.data_ptr(), self.weight.data_ptr(), self.n_out,
                                                  self.keep_channels, out.data_ptr(), stream),
                   "gsr_refine_prepare")
        if cache:
            self._prep_key, self._prep = (weakref.ref(owner), ident), out
        return out

    def invalidate(self):
        """Drop the cached pre-contracted features (after writing them outside torch's tracking)."""
        self._prep_key, self._prep = None, None

    def epilogue(self, B, H, W):
        """The C-ABI epilogue block; the output tensor is per (stream, shape), so batches in flight
        on different streams do not share one buffer.  self.out is the one of the last call."""
        shape = (B, self.n_out, H, W)
        key = (torch.cuda.current_stream(self.weight.device).cuda_stream, shape)
        out = self._outs.get(key)
        if out is None:
            out = self._outs[key] = torch.empty(shape, dtype=torch.float32, device=self.weight.device)
        self.out = out
        return _lib.RefineEpilogue(self.weight.data_ptr(),
                                   self.bias.data_ptr() if self.bias is not None else None,
                                   self.n_out, self.slope, out.data_ptr(), self.keep_channels)


class _RenderRefined(torch.autograd.Function):
    """forward(refine=head) + backward_refine as one autograd node (render_refined)."""

    @staticmethod
    def forward(ctx, rast, opts, weight, bias, means3D, colors, opacities, scales, rotations, viewmatrices,
                projmatrices, tanfov, backgrounds):
        slope, keep, scale_modifier, antialiasing, numerics = opts
        # a head per call: its output buffer is this call's own, so `refined` survives later forwards
        head = RefineHead(weight, bias, slope, keep)
        attrs = tuple(t.detach() for t in (means3D, colors, opacities, scales, rotations))
        cams = tuple(t.detach() for t in (viewmatrices, projmatrices, tanfov, backgrounds))
        col, inv, radii = rast.forward(*attrs, *cams, scale_modifier=scale_modifier, antialiasing=antialiasing,
                                       refine=head, numerics=numerics)
        raw, invd, rad = col[:, :keep].clone(), inv.clone(), radii.clone()
        ctx.rast, ctx.head, ctx.opts, ctx.attrs, ctx.cams = rast, head, opts, attrs, cams
        ctx.count = rast._fwd_count
        ctx.shapes = (weight.shape, tuple(t.dim() for t in attrs))
        ctx.mark_non_differentiable(rad)
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not zeros
        return raw, head.out, invd, rad

    @staticmethod
    def backward(ctx, d_raw, d_refined, d_invdepth, _d_radii):
        rast, head = ctx.rast, ctx.head
        if rast._fwd_count != ctx.count:
            raise _lib.GsrError("render_refined: another forward ran on this rasterizer before backward(); the "
                                "workspace holds that forward's state, not this one's")
        _, _, scale_modifier, antialiasing, numerics = ctx.opts
        wshape, dims = ctx.shapes
        if d_refined is None:
            d_refined = torch.zeros_like(head.out)
        shared = all(d == 2 for d in dims)
        g = rast.backward_refine(head, *ctx.attrs, *ctx.cams, d_refined, dL_draw=d_raw, dL_dinvdepth=d_invdepth,
                                 scale_modifier=scale_modifier, antialiasing=antialiasing, shared=shared,
                                 numerics=numerics, out_refine=head.out)
        per = [g["means3D"], g["colors"], g["opacity"], g["scales"], g["rotations"]]
        if not shared:  # an attribute shared by the frames gets the sum of its per-frame gradients
            per = [t.sum(0) if d == 2 else t for t, d in zip(per, dims)]
        need = ctx.needs_input_grad
        grads = [None, None, g["weight"].reshape(wshape), g["bias"] if head.bias is not None else None] + per + \
                [None, None, None, None]
        return tuple(gr if nd else None for gr, nd in zip(grads, need))


def render_refined(rast, weight, bias, means3D, colors, opacities, scales, rotations, viewmatrices, projmatrices,
                   tanfov, backgrounds, negative_slope=0.2, keep_channels=4, scale_modifier=1.0, antialiasing=False,
                   numerics=None):
    """Differentiable render + fused refiner head (conv_body_first + leaky ReLU) on `rast`
    (a BatchRasterizer): returns (raw [B,keep,H,W], refined [B,n_out,H,W], invdepth [B,H,W], radii
    [B,P]) -- tensors of this call's own, so the rest of a StyleUNet chains onto `refined` in ordinary
    torch.  .backward() fills the gradients of weight [n_out,32(,1,1)], bias [n_out] (or None) and of
    the five attributes; attributes all given as [P,k] take the frame-reduced backward.  The
    workspace is single-use: a backward after another forward on `rast` raises GsrError.  viewmatrices,
    projmatrices, tanfov and backgrounds get no gradient."""
    opts = (float(negative_slope), int(keep_channels), float(scale_modifier), bool(antialiasing), numerics)
    return _RenderRefined.apply(rast, opts, weight, bias, means3D, colors, opacities, scales, rotations,
                                viewmatrices, projmatrices, tanfov, backgrounds)


def profile_enable(stages=("render_fwd",)):
    mask = 0
    for s in stages:
        mask |= 1 << STAGES.index(s)
    _lib.load().gsr_profile_enable(mask)


def profile_read():
    n = len(STAGES)
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int * n)()
    _lib.check(_lib.load().gsr_profile_read(ms, cnt, n), "gsr_profile_read")
    return {s: (ms[i], cnt[i]) for i, s in enumerate(STAGES) if cnt[i]}


COUNTERS = ("pairs_evaluated", "pairs_contributing", "strip_pairs_blended", "mfma_ksteps",
            "gaussians_staged", "list_entries", "tiles_rendered", "dead_ksteps")


def render_counters(fn, device="cuda"):
    """Run `fn()` (one or more forwards) with the instrumented render kernel and return the work
    counters of include/gsr.h:gsr_render_counters as a dict."""
    L = _lib.load()
    buf = torch.zeros(len(COUNTERS), dtype=torch.int64, device=device)
    L.gsr_render_counters(buf.data_ptr())
    try:
        fn()
        torch.cuda.synchronize(device)
    finally:
        L.gsr_render_counters(None)
    v = buf.cpu().tolist()
    return {k: int(v[i]) for i, k in enumerate(COUNTERS)}
