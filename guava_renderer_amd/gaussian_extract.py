"""UV Gaussian extraction on gfx950 (csrc/extract.hip through include/gsr_extract.h): from the UV point
decoder's output maps to the reference's uv_point_gs_dict of per-Gaussian tables, fused -- the head
activations (models/modules/net_module/feature_decoder.py:120-135), the permutes, the boolean gathers
and binding_face / face_bary (models/UbodyAvatar/ubody_gaussian.py:150-156), the RGB sigmoid (:186-187)
and the opacity pruning (:229-243).

  UVGaussianExtractor(uvmap_mask [U,U], uvmap_f_idx [U,U], uvmap_f_bary [U,U,3], color_dim=32)
      .extract(colors, opacities, scales, rotations, local_pos, raw=True, rgb_sigmoid=True) -> dict
      .extract_pruned(..., opacity_threshold=0.001) -> dict   (B = 1, no gradient)

raw=True: the heads' raw outputs, planar [B,k,U,U], before sigmoid / exp / normalize.  raw=False: the
decoder's outputs as the reference returns them, [B,U,U,k], activations applied.  Semantics:
include/gsr_extract.h.  The five maps carry gradients (a deterministic HIP backward).
GPU only: CPU tensors raise; there is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib

KEYS = ("colors", "opacities", "scales", "rotations", "local_pos")


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _set(tensors):
    """ExtractSet of five tensors (None or an empty tensor: a null pointer)."""
    return _lib.ExtractSet(*[ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None for t in tensors])


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class _Extract(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ex, layout, flags, *maps):
        B, N, T, C = int(maps[0].shape[0]), ex.N, ex.T, ex.color_dim
        dev = maps[0].device
        tables = [torch.empty((B, N, k), dtype=torch.float32, device=dev) for k in (C, 1, 3, 4, 3)]
        if N:
            with torch.cuda.device(dev):
                _lib.check(_lib.load().gsr_extract_forward(B, T, N, C, layout, flags, _p(ex.mask_u8), _p(ex.tile_base),
                                                           ctypes.byref(_set(maps)), ctypes.byref(_set(tables)), None,
                                                           None, None, None, _stream(dev)), "gsr_extract_forward")
        ctx.ex, ctx.layout, ctx.flags = ex, layout, flags
        ctx.save_for_backward(*maps)
        return tuple(tables)

    @staticmethod
    def backward(ctx, *dtables):
        maps = ctx.saved_tensors
        ex = ctx.ex
        B, N, T, C = int(maps[0].shape[0]), ex.N, ex.T, ex.color_dim
        dev = maps[0].device
        dtables = [None if g is None else g.to(torch.float32).contiguous() for g in dtables]
        dmaps = [torch.empty_like(m) if ctx.needs_input_grad[3 + i] else None for i, m in enumerate(maps)]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gsr_extract_backward(B, T, N, C, ctx.layout, ctx.flags, _p(ex.mask_u8), _p(ex.tile_base),
                                                        ctypes.byref(_set(maps)), ctypes.byref(_set(dtables)),
                                                        ctypes.byref(_set(dmaps)), _stream(dev)), "gsr_extract_backward")
        return (None, None, None) + tuple(dmaps)


class UVGaussianExtractor:
    """The reference inferer's UV-map-to-table glue for one UV layout.  The tile scan of the mask, N,
    binding_face [1,N,1] (int64) and face_bary [1,N,3] are built once here, on the GPU; extract() reads
    nothing back from the device."""

    def __init__(self, uvmap_mask, uvmap_f_idx, uvmap_f_bary, color_dim=32, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("UVGaussianExtractor runs on the GPU only")
        t = lambda a: torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else torch.as_tensor(a)  # noqa: E731
        mask, f_idx, f_bary = t(uvmap_mask), t(uvmap_f_idx), t(uvmap_f_bary)
        if mask.dim() != 2 or mask.shape[0] != mask.shape[1] or mask.shape[0] == 0:
            raise RuntimeError(f"uvmap_mask must have dimensions (U, U), got {tuple(mask.shape)}")
        U = int(mask.shape[0])
        if tuple(f_idx.shape) != (U, U) or tuple(f_bary.shape) != (U, U, 3):
            raise RuntimeError(f"uvmap_f_idx must be ({U}, {U}) and uvmap_f_bary ({U}, {U}, 3), got "
                               f"{tuple(f_idx.shape)} and {tuple(f_bary.shape)}")
        if not bool(((mask == 0) | (mask == 1)).all()):
            raise RuntimeError("uvmap_mask must hold only 0 and 1")
        color_dim = int(color_dim)
        if not 3 <= color_dim <= 64:
            raise RuntimeError(f"color_dim must lie in [3, 64], got {color_dim}")
        self.U, self.T, self.color_dim = U, U * U, color_dim
        self.widths = (color_dim, 1, 3, 4, 3)
        self.N = int((mask != 0).sum())  # on the caller's copy of the mask: the one host-side count
        L = _lib.load()
        self.mask_u8 = (mask != 0).reshape(-1).to(device=self.device, dtype=torch.uint8).contiguous()
        self.texel_face = f_idx.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        self.texel_bary = f_bary.reshape(-1, 3).to(device=self.device, dtype=torch.float32).contiguous()
        self.tile_base = torch.empty((L.gsr_extract_tiles(self.T) + 1,), dtype=torch.int32, device=self.device)
        bind = torch.empty((self.N,), dtype=torch.int32, device=self.device)
        self.face_bary = torch.empty((1, self.N, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.gsr_extract_prepare(self.T, _p(self.mask_u8), _p(self.tile_base), _stream(self.device)),
                       "gsr_extract_prepare")
            if self.N:
                _lib.check(L.gsr_extract_forward(1, self.T, self.N, color_dim, _lib.EXTRACT_PLANAR_RAW, 0, _p(self.mask_u8),
                                                 _p(self.tile_base), None, None, _p(self.texel_face), _p(self.texel_bary),
                                                 _p(bind), _p(self.face_bary), _stream(self.device)),
                           "gsr_extract_forward")
        self.binding_face = bind.to(torch.int64).reshape(1, self.N, 1)

    def _maps(self, maps, raw, what):
        U, out, B = self.U, [], None
        for key, k, m in zip(KEYS, self.widths, maps):
            if not torch.is_tensor(m) or not m.is_cuda:
                raise RuntimeError(f"{what} runs on the GPU only ({key} is not a GPU tensor)")
            want = f"(B, {k}, {U}, {U})" if raw else f"(B, {U}, {U}, {k})"
            ok = m.dim() == 4 and (tuple(m.shape[1:]) == ((k, U, U) if raw else (U, U, k))) and m.shape[0] > 0
            if not ok or (B is not None and m.shape[0] != B):
                raise RuntimeError(f"{key} must have dimensions {want}" + (f" with B = {B}" if B is not None else "") +
                                   f", got {tuple(m.shape)}")
            B = int(m.shape[0])
            out.append(m.to(device=self.device, dtype=torch.float32).contiguous())
        return out, B

    def _dict(self, tables):
        d = dict(zip(KEYS, tables))
        d["binding_face"], d["face_bary"] = self.binding_face, self.face_bary
        return d

    def extract(self, colors, opacities, scales, rotations, local_pos, raw=True, rgb_sigmoid=True):
        """-> the reference's uv_point_gs_dict: colors [B,N,C], opacities [B,N,1], scales [B,N,3],
        rotations [B,N,4], local_pos [B,N,3], binding_face [1,N,1], face_bary [1,N,3].  With
        rgb_sigmoid=True the first three colour channels are final (GaussianDeformer(...,
        apply_rgb_sigmoid=False), deform_gaussians); with False they are left to Ubody_Gaussian."""
        maps, _ = self._maps((colors, opacities, scales, rotations, local_pos), raw, "extract")
        layout = _lib.EXTRACT_PLANAR_RAW if raw else _lib.EXTRACT_ROWS_ACTIVATED
        flags = _lib.EXTRACT_RGB_SIGMOID if rgb_sigmoid else 0
        return self._dict(_Extract.apply(self, layout, flags, *maps))

    def extract_pruned(self, colors, opacities, scales, rotations, local_pos, raw=True, rgb_sigmoid=True,
                       opacity_threshold=0.001):
        """extract() followed by Ubody_Gaussian.prune_gaussians (:229-243): only the Gaussians with
        opacity > opacity_threshold, binding_face and face_bary narrowed alike.  B = 1, no gradient; one
        device word (the count) is read back to narrow the tables."""
        given = (colors, opacities, scales, rotations, local_pos)
        if torch.is_grad_enabled() and any(torch.is_tensor(m) and m.requires_grad for m in given):
            raise RuntimeError("extract_pruned has no gradient: call it under torch.no_grad() or detach the maps")
        maps, B = self._maps(given, raw, "extract_pruned")
        if B != 1:
            raise RuntimeError(f"extract_pruned needs B = 1 (as the reference asserts), got B = {B}")
        N, T, C, dev = self.N, self.T, self.color_dim, self.device
        layout = _lib.EXTRACT_PLANAR_RAW if raw else _lib.EXTRACT_ROWS_ACTIVATED
        flags = _lib.EXTRACT_RGB_SIGMOID if rgb_sigmoid else 0
        tables = [torch.empty((1, N, k), dtype=torch.float32, device=dev) for k in self.widths]
        bind = torch.empty((N,), dtype=torch.int32, device=dev)
        bary = torch.empty((1, N, 3), dtype=torch.float32, device=dev)
        pruned_base = torch.empty_like(self.tile_base)
        L = _lib.load()
        thr = float(opacity_threshold)
        with torch.cuda.device(dev):
            _lib.check(L.gsr_extract_prepare_pruned(T, layout, _p(self.mask_u8), _p(maps[1]), thr, _p(pruned_base),
                                                    _stream(dev)), "gsr_extract_prepare_pruned")
            if N:
                _lib.check(L.gsr_extract_forward_pruned(T, N, C, layout, flags, thr, _p(self.mask_u8), _p(self.tile_base),
                                                        _p(pruned_base), ctypes.byref(_set(maps)),
                                                        ctypes.byref(_set(tables)), _p(self.texel_face),
                                                        _p(self.texel_bary), _p(bind), _p(bary), _stream(dev)),
                           "gsr_extract_forward_pruned")
        count = int(pruned_base[-1])  # the one read
        d = {key: t[:, :count] for key, t in zip(KEYS, tables)}
        d["binding_face"] = bind[:count].to(torch.int64).reshape(1, count, 1)
        d["face_bary"] = bary[:, :count]
        return d
