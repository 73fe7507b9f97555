"""Image-to-avatar feature lifting on gfx950 (csrc/lift.hip through include/gsr_lift.h): the two
projection gathers of the reference's Ubody_Gaussian_inferer (models/UbodyAvatar/ubody_gaussian.py),
under the reference's names and returns.

  FeatureLifter(faces, uvmap_f_idx [U,U], uvmap_f_bary [U,U,3], uvmap_mask [U,U], image_size, focal_length)
      .sample_prj_feature(vertices, feature_map, w2c_cam) -> (features [B,V,C], vertices_img [B,V,2])    :75-83
      .convert_pixel_feature_to_uv(img_features, deformed_vertices, w2c_cam,
                                   visble_faces=None, face_visible=None) -> [B,C,U,U]                  :85-114

Semantics: include/gsr_lift.h.  The feature map carries the gradient (a bilinear
scatter-add in HIP); the sample positions carry none -- every EHM parameter of the reference has
requires_grad = False -- so vertices or cameras that require grad raise NotImplementedError.
GPU only: CPU tensors raise; there is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(B, C, W, H, device):
    n = _lib.load().gsr_lift_backward_workspace_bytes(B, C, W, H)
    if n == 0:
        raise RuntimeError(f"feature lifting: sizes out of range (B={B}, C={C}, {W}x{H})")
    return torch.empty((n,), dtype=torch.uint8, device=device)


class _LiftVertices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, verts, w2c, tx, ty):
        B, C, H, W = feat.shape
        V = verts.shape[1]
        out = torch.empty((B, V, C), dtype=torch.float32, device=feat.device)
        ndc = torch.empty((B, V, 2), dtype=torch.float32, device=feat.device)
        with torch.cuda.device(feat.device):
            _lib.check(_lib.load().gsr_lift_vertices(B, V, C, W, H, _p(verts), _p(w2c), _p(tx), _p(ty), _p(feat), _p(out),
                                                     _p(ndc), _stream(feat.device)), "gsr_lift_vertices")
        ctx.save_for_backward(verts, w2c, tx, ty)
        ctx.dims = (B, V, C, W, H)
        ctx.mark_non_differentiable(ndc)
        return out, ndc

    @staticmethod
    def backward(ctx, dout, _dndc):
        verts, w2c, tx, ty = ctx.saved_tensors
        B, V, C, W, H = ctx.dims
        dout = dout.to(torch.float32).contiguous()
        dfeat = torch.empty((B, C, H, W), dtype=torch.float32, device=dout.device)
        ws = _workspace(B, C, W, H, dout.device)
        with torch.cuda.device(dout.device):
            _lib.check(_lib.load().gsr_lift_vertices_backward(B, V, C, W, H, _p(verts), _p(w2c), _p(tx), _p(ty), _p(dout),
                                                              _p(dfeat), _p(ws), _stream(dout.device)),
                       "gsr_lift_vertices_backward")
        return dfeat, None, None, None, None


class _LiftUV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, verts, faces, texel_face, texel_bary, w2c, tx, ty, face_visible):
        B, C, H, W = feat.shape
        V, F, T = verts.shape[1], faces.shape[0], texel_face.shape[0]
        out = torch.empty((B, C, T), dtype=torch.float32, device=feat.device)
        with torch.cuda.device(feat.device):
            _lib.check(_lib.load().gsr_lift_uv(B, V, F, T, C, W, H, _p(verts), _p(faces), _p(texel_face), _p(texel_bary),
                                               _p(w2c), _p(tx), _p(ty), _p(feat), _p(face_visible), _p(out),
                                               _stream(feat.device)), "gsr_lift_uv")
        ctx.save_for_backward(verts, faces, texel_face, texel_bary, w2c, tx, ty)
        ctx.face_visible = face_visible
        ctx.dims = (B, V, F, T, C, W, H)
        return out

    @staticmethod
    def backward(ctx, dout):
        verts, faces, texel_face, texel_bary, w2c, tx, ty = ctx.saved_tensors
        B, V, F, T, C, W, H = ctx.dims
        dout = dout.to(torch.float32).contiguous()
        dfeat = torch.empty((B, C, H, W), dtype=torch.float32, device=dout.device)
        ws = _workspace(B, C, W, H, dout.device)
        with torch.cuda.device(dout.device):
            _lib.check(_lib.load().gsr_lift_uv_backward(B, V, F, T, C, W, H, _p(verts), _p(faces), _p(texel_face),
                                                        _p(texel_bary), _p(w2c), _p(tx), _p(ty), _p(ctx.face_visible),
                                                        _p(dout), _p(dfeat), _p(ws), _stream(dout.device)),
                       "gsr_lift_uv_backward")
        return (dfeat,) + (None,) * 8


class FeatureLifter:
    """The reference inferer's sample_prj_feature and convert_pixel_feature_to_uv for one mesh topology
    and UV layout.  texel_face = where(uvmap_mask != 0, uvmap_f_idx, -1) is built once."""

    def __init__(self, faces, uvmap_f_idx, uvmap_f_bary, uvmap_mask, image_size=512, focal_length=24, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FeatureLifter runs on the GPU only")
        t = lambda a: torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else torch.as_tensor(a)  # noqa: E731
        faces, f_idx, f_bary, mask = t(faces), t(uvmap_f_idx), t(uvmap_f_bary), t(uvmap_mask)
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
            raise RuntimeError(f"faces must have dimensions (num_faces, 3), got {tuple(faces.shape)}")
        if f_idx.dim() != 2 or f_idx.shape[0] != f_idx.shape[1]:
            raise RuntimeError(f"uvmap_f_idx must have dimensions (U, U), got {tuple(f_idx.shape)}")
        U = int(f_idx.shape[0])
        if tuple(f_bary.shape) != (U, U, 3) or tuple(mask.shape) != (U, U):
            raise RuntimeError(f"uvmap_f_bary must be ({U}, {U}, 3) and uvmap_mask ({U}, {U})")
        if not bool(((mask == 0) | (mask == 1)).all()):
            raise RuntimeError("uvmap_mask must hold only 0 and 1")
        if isinstance(image_size, (tuple, list)):
            H, W = int(image_size[0]), int(image_size[1])
        else:
            H = W = int(image_size)
        self.image_size = (H, W)
        self.focal_length = float(focal_length)
        side = min(H, W)
        # BaseMeshRenderer's rule (PyTorch3D, non-square): the shorter side spans NDC [-1, 1]
        self.tanfovx = (W / side) / self.focal_length
        self.tanfovy = (H / side) / self.focal_length
        if faces.dtype.is_floating_point or bool((faces < 0).any()):
            raise RuntimeError("faces must hold non-negative integer vertex indices")
        self.U, self.F = U, int(faces.shape[0])
        self.v_min = int(faces.max()) + 1  # vertices a call must bring at least
        self.faces = faces.to(device=self.device, dtype=torch.int32).contiguous()
        f_idx = f_idx.to(self.device).reshape(-1).to(torch.int64)
        self.uvmap_f_idx = f_idx.reshape(U, U)
        self.uvmap_mask = mask.to(self.device)
        self.texel_face = torch.where(self.uvmap_mask.reshape(-1) != 0, f_idx,
                                      torch.full_like(f_idx, -1)).to(torch.int32).contiguous()
        self.texel_bary = f_bary.to(device=self.device, dtype=torch.float32).reshape(-1, 3).contiguous()
        self._fov = {}

    def _fov_tensors(self, B):
        if B not in self._fov:
            self._fov[B] = (torch.full((B,), self.tanfovx, dtype=torch.float32, device=self.device),
                            torch.full((B,), self.tanfovy, dtype=torch.float32, device=self.device))
        return self._fov[B]

    def _inputs(self, feature_map, vertices, w2c_cam, what):
        for name, x in (("feature_map", feature_map), ("vertices", vertices), ("w2c_cam", w2c_cam)):
            if not torch.is_tensor(x) or not x.is_cuda:
                raise RuntimeError(f"{what} runs on the GPU only ({name} is not a GPU tensor)")
        if vertices.requires_grad or w2c_cam.requires_grad:
            raise NotImplementedError(f"{what} has no gradient for vertices / w2c_cam (the reference's EHM "
                                      "parameters are frozen); detach them")
        if feature_map.dim() != 4:
            raise RuntimeError(f"feature_map must have dimensions (B, C, H, W), got {tuple(feature_map.shape)}")
        B, C, H, W = (int(x) for x in feature_map.shape)
        if (H, W) != self.image_size:
            raise RuntimeError(f"feature_map is {H}x{W}, this lifter was built for {self.image_size[0]}x"
                               f"{self.image_size[1]}")
        if vertices.dim() != 3 or vertices.shape[0] != B or vertices.shape[2] != 3:
            raise RuntimeError(f"vertices must have dimensions ({B}, num_verts, 3), got {tuple(vertices.shape)}")
        if w2c_cam.dim() != 3 or w2c_cam.shape[0] != B or w2c_cam.shape[2] != 4 or w2c_cam.shape[1] not in (3, 4):
            raise RuntimeError(f"w2c_cam must have dimensions ({B}, 4, 4), got {tuple(w2c_cam.shape)}")
        w2c = w2c_cam.to(device=self.device, dtype=torch.float32)
        if w2c.shape[1] == 3:
            last = torch.tensor([0.0, 0.0, 0.0, 1.0], device=self.device).expand(B, 1, 4)
            w2c = torch.cat([w2c, last], 1)
        feat = feature_map.to(device=self.device, dtype=torch.float32).contiguous()
        verts = vertices.to(device=self.device, dtype=torch.float32).contiguous()
        return feat, verts, w2c.contiguous(), B

    def sample_prj_feature(self, vertices, feature_map, w2c_cam):
        """vertices [B,V,3], feature_map [B,C,H,W], w2c_cam [B,4,4] -> (features [B,V,C] sampled
        bilinearly with border padding at the projected vertices, vertices_img [B,V,2] their NDC)."""
        feat, verts, w2c, B = self._inputs(feature_map, vertices, w2c_cam, "sample_prj_feature")
        tx, ty = self._fov_tensors(B)
        return _LiftVertices.apply(feat, verts, w2c, tx, ty)

    def convert_pixel_feature_to_uv(self, img_features, deformed_vertices, w2c_cam, visble_faces=None,
                                    face_visible=None):
        """img_features [B,C,H,W] -> [B,C,U,U]: every UV texel placed on its face and projected, sampled
        with zeros padding, times uvmap_mask and the visibility.  face_visible: MeshRasterizer's uint8
        [B,F] (the fast path); visble_faces: the reference's packed pix_to_face of render_fragments."""
        feat, verts, w2c, B = self._inputs(img_features, deformed_vertices, w2c_cam, "convert_pixel_feature_to_uv")
        if visble_faces is not None and face_visible is not None:
            raise RuntimeError("pass visble_faces or face_visible, not both")
        if int(verts.shape[1]) < self.v_min:
            raise RuntimeError(f"faces index {self.v_min} vertices, deformed_vertices has {int(verts.shape[1])}")
        if visble_faces is not None:
            if not torch.is_tensor(visble_faces) or not visble_faces.is_cuda:
                raise RuntimeError("convert_pixel_feature_to_uv runs on the GPU only (visble_faces is not a GPU tensor)")
            # mesh_raster.visible_uv_mask's scatter, kept per face
            p = visble_faces.reshape(B, -1).to(torch.int64)
            local = p - torch.arange(B, device=p.device, dtype=torch.int64)[:, None] * self.F
            hit = (p >= 0) & (local >= 0) & (local < self.F)
            vis = torch.zeros((B, self.F + 1), dtype=torch.bool, device=p.device)
            vis.scatter_(1, torch.where(hit, local, torch.full_like(local, self.F)), True)
            face_visible = vis[:, :self.F]
        if face_visible is not None:
            if not torch.is_tensor(face_visible) or not face_visible.is_cuda:
                raise RuntimeError("convert_pixel_feature_to_uv runs on the GPU only (face_visible is not a GPU tensor)")
            if tuple(face_visible.shape) != (B, self.F):
                raise RuntimeError(f"face_visible must have dimensions ({B}, {self.F}), got {tuple(face_visible.shape)}")
            face_visible = face_visible.to(device=self.device, dtype=torch.uint8).contiguous()
        tx, ty = self._fov_tensors(B)
        out = _LiftUV.apply(feat, verts, self.faces, self.texel_face, self.texel_bary, w2c, tx, ty, face_visible)
        return out.reshape(B, feat.shape[1], self.U, self.U)
