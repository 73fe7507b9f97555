"""Mesh visibility rasterizer on gfx950 (csrc/mesh_raster.hip through include/gsr_mesh.h): the
pix_to_face / zbuf / bary_coords that the reference takes from PyTorch3D's rasterize_meshes at
blur_radius = 0, faces_per_pixel = 1, perspective-correct.

  MeshRasterizer(faces, W, H, max_batch)   owns the workspace; call -> MeshFragments
  BaseMeshRenderer(faces, image_size, focal_length)
      .render_fragments(vertices, transform_matrix=..., reverse_camera=True) -> (pix_to_face, Fragments)
                                          the reference's utils/graphics_utils.py:471-492
  visible_uv_mask(pix_to_face, F, uvmap_f_idx, uvmap_mask)
                                          the visibility mask of models/UbodyAvatar/ubody_gaussian.py:102-111

Semantics: include/gsr_mesh.h.  `dists` is not produced (at blur 0 only PyTorch3D's
soft shaders read it): Fragments.dists is None.  No gradients (the reference calls this under no_grad).
GPU only: CPU tensors raise.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

MeshFragments = collections.namedtuple("MeshFragments",
                                       ["pix_to_face", "zbuf", "bary_coords", "face_visible", "texel_visible"])
# PyTorch3D's Fragments, by field name
Fragments = collections.namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords", "dists"])


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class MeshRasterizer:
    """Rasterizes up to `max_batch` posed copies of one mesh topology per call at W x H."""

    def __init__(self, faces, W, H, max_batch, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MeshRasterizer runs on the GPU only")
        faces = torch.from_numpy(np.array(faces)) if isinstance(faces, np.ndarray) else torch.as_tensor(faces)
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
            raise RuntimeError(f"faces must have dimensions (num_faces, 3), got {tuple(faces.shape)}")
        if faces.dtype.is_floating_point or bool((faces < 0).any()):
            raise RuntimeError("faces must hold non-negative integer vertex indices")
        self.W, self.H, self.max_batch = int(W), int(H), int(max_batch)
        if self.W <= 0 or self.H <= 0 or self.max_batch <= 0:
            raise RuntimeError("W, H and max_batch must be positive")
        self.F = int(faces.shape[0])
        self.v_min = int(faces.max()) + 1  # vertices a call must bring at least
        self.faces = faces.to(device=self.device, dtype=torch.int32).contiguous()
        self._ws = None
        self._ws_v = 0
        self._fov = {}

    def _workspace(self, V):
        if self._ws is None or V > self._ws_v:
            n = _lib.load().gsr_mesh_raster_workspace_bytes(self.max_batch, V, self.F, self.W, self.H)
            if n == 0:
                raise RuntimeError(f"mesh rasterizer: sizes out of range (B={self.max_batch}, V={V}, F={self.F}, "
                                   f"{self.W}x{self.H})")
            self._ws = torch.empty((n,), dtype=torch.uint8, device=self.device)
            self._ws_v = V
        return self._ws

    def _fov_tensor(self, t, B, name):
        if torch.is_tensor(t):
            if not t.is_cuda:
                raise RuntimeError(f"{name} must be a float, a sequence of B floats or a GPU tensor")
            t = t.detach().to(device=self.device, dtype=torch.float32).reshape(-1)
            if t.numel() == 1:
                t = t.expand(B)
        else:
            key = (tuple(float(x) for x in t) if hasattr(t, "__len__") else (float(t),) * B)
            if key not in self._fov:
                if len(self._fov) > 64:
                    self._fov.clear()
                self._fov[key] = torch.tensor(key, dtype=torch.float32, device=self.device)
            t = self._fov[key]
        if t.numel() != B:
            raise RuntimeError(f"{name} must have one value per frame ({B}), got {t.numel()}")
        return t.contiguous()

    def __call__(self, verts, w2c, tanfovx, tanfovy, packed=False, binding_face=None):
        """verts [B,V,3], w2c [B,4,4] (world-to-camera, row-major, as camera.look_at_w2c), tanfovx /
        tanfovy a float, B floats or a GPU tensor.  Returns MeshFragments on the current stream:
        pix_to_face int32 [B,H,W] (b*F + face with packed), zbuf [B,H,W], bary_coords [B,H,W,3],
        face_visible uint8 [B,F], texel_visible uint8 [B,N] (None without binding_face [N])."""
        for name, t in (("verts", verts), ("w2c", w2c)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"mesh rasterizer runs on the GPU only ({name} is not a GPU tensor)")
        if verts.dim() != 3 or verts.shape[2] != 3:
            raise RuntimeError(f"verts must have dimensions (B, num_verts, 3), got {tuple(verts.shape)}")
        B, V = int(verts.shape[0]), int(verts.shape[1])
        if B < 1 or B > self.max_batch:
            raise RuntimeError(f"batch of {B} frames outside this rasterizer's 1..{self.max_batch}")
        if V < self.v_min:
            raise RuntimeError(f"faces index {self.v_min} vertices, verts has {V}")
        if tuple(w2c.shape) != (B, 4, 4):
            raise RuntimeError(f"w2c must have dimensions ({B}, 4, 4), got {tuple(w2c.shape)}")
        verts = verts.detach().to(device=self.device, dtype=torch.float32).contiguous()
        w2c = w2c.detach().to(device=self.device, dtype=torch.float32).contiguous()
        tx, ty = self._fov_tensor(tanfovx, B, "tanfovx"), self._fov_tensor(tanfovy, B, "tanfovy")
        if packed and B * self.F >= 2 ** 31:
            raise RuntimeError("packed face indices would overflow int32")
        ws = self._workspace(V)
        H, W, F = self.H, self.W, self.F
        p2f = torch.empty((B, H, W), dtype=torch.int32, device=self.device)
        zbuf = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
        bary = torch.empty((B, H, W, 3), dtype=torch.float32, device=self.device)
        vis = torch.empty((B, F), dtype=torch.uint8, device=self.device)
        L = _lib.load()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            _lib.check(L.gsr_mesh_raster(B, V, F, W, H, _p(verts), _p(self.faces), _p(w2c), _p(tx), _p(ty),
                                         int(bool(packed)), _p(p2f), _p(zbuf), _p(bary), _p(vis), _p(ws), stream),
                       "gsr_mesh_raster")
            tex = None
            if binding_face is not None:
                tex = self.visible_texels(vis, binding_face)
        return MeshFragments(p2f, zbuf, bary, vis, tex)

    def visible_texels(self, face_visible, binding_face):
        """uint8 [B,N] = face_visible[:, binding_face]  (binding_face [N] integer GPU tensor)."""
        if not torch.is_tensor(binding_face) or not binding_face.is_cuda or binding_face.dim() != 1:
            raise RuntimeError("binding_face must be a 1-D GPU tensor")
        bf = binding_face.to(device=self.device, dtype=torch.int32).contiguous()
        B, N = int(face_visible.shape[0]), int(bf.shape[0])
        tex = torch.empty((B, N), dtype=torch.uint8, device=self.device)
        if N:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.load().gsr_mesh_visible_texels(B, self.F, N, _p(face_visible), _p(bf), _p(tex), stream),
                       "gsr_mesh_visible_texels")
        return tex

    def stats(self):
        """Counters of the last call (synchronises): dict(lane_faces, wide_faces, culled_faces,
        covered_pixels); lane + wide + culled = B*F."""
        if self._ws is None:
            raise RuntimeError("no call yet")
        torch.cuda.synchronize(self.device)
        out = (ctypes.c_int64 * 4)()
        _lib.check(_lib.load().gsr_mesh_raster_stats(_p(self._ws), out), "gsr_mesh_raster_stats")
        return dict(zip(("lane_faces", "wide_faces", "culled_faces", "covered_pixels"), (int(x) for x in out)))


class BaseMeshRenderer:
    """The visibility half of the reference's BaseMeshRenderer (utils/graphics_utils.py:420-492) with
    its names: render_fragments only; mesh shading (render_mesh's Phong / texture shaders) is not part
    of this library."""

    def __init__(self, faces, image_size=512, focal_length=24, max_batch=8, device="cuda"):
        if isinstance(image_size, (tuple, list)):
            H, W = int(image_size[0]), int(image_size[1])
        else:
            H = W = int(image_size)
        self.image_size = (H, W)
        self.focal_length = float(focal_length)
        side = min(H, W)
        # PyTorch3D's non-square rule: the shorter side spans NDC [-1, 1]
        self.tanfovx = (W / side) / self.focal_length
        self.tanfovy = (H / side) / self.focal_length
        self.rasterizer = MeshRasterizer(faces, W, H, max_batch, device)
        self.faces = self.rasterizer.faces
        self.device = self.rasterizer.device

    def render_fragments(self, vertices, cameras=None, transform_matrix=None, reverse_camera=True):
        """vertices [B,V,3], transform_matrix [B,4,4] or [B,3,4] world-to-camera -> (pix_to_face int64
        [B,H,W,1] packed as b*F + face (-1 empty), Fragments(pix_to_face, zbuf [B,H,W,1],
        bary_coords [B,H,W,1,3], dists=None))."""
        if cameras is not None:
            raise NotImplementedError("render_fragments: a PyTorch3D cameras object is not supported; pass "
                                      "transform_matrix (world-to-camera, [B,4,4])")
        if transform_matrix is None:
            raise RuntimeError("render_fragments needs transform_matrix")
        if not torch.is_tensor(vertices) or not vertices.is_cuda or not torch.is_tensor(transform_matrix) \
                or not transform_matrix.is_cuda:
            raise RuntimeError("render_fragments runs on the GPU only (got a CPU tensor)")
        B = vertices.shape[0]
        tm = transform_matrix.detach().to(torch.float32)
        if tm.dim() != 3 or tm.shape[0] != B or tm.shape[2] != 4 or tm.shape[1] not in (3, 4):
            raise RuntimeError(f"transform_matrix must have dimensions ({B}, 4, 4), got {tuple(tm.shape)}")
        if tm.shape[1] == 3:
            last = torch.tensor([0.0, 0.0, 0.0, 1.0], device=tm.device).expand(B, 1, 4)
            tm = torch.cat([tm, last], 1)
        if not reverse_camera:
            tm = tm.clone()
            tm[:, :2] = -tm[:, :2]
        if B > self.rasterizer.max_batch:  # the reference takes any batch: grow instead of refusing
            self.rasterizer = MeshRasterizer(self.faces, self.image_size[1], self.image_size[0], B, self.device)
        fr = self.rasterizer(vertices, tm, self.tanfovx, self.tanfovy, packed=True)
        pix_to_face = fr.pix_to_face.to(torch.int64).unsqueeze(-1)
        return pix_to_face, Fragments(pix_to_face, fr.zbuf.unsqueeze(-1), fr.bary_coords.unsqueeze(3), None)


def visible_uv_mask(pix_to_face, F, uvmap_f_idx, uvmap_mask):
    """The reference's UV visibility mask (ubody_gaussian.py:102-111) from packed pix_to_face
    [B,H,W,1]: texel (u, v) is visible in frame b iff the face it lies on (uvmap_f_idx [U,U]) wins a
    pixel there, and uvmap_mask [U,U] covers it.  Returns [B,U,U] in uvmap_mask's dtype."""
    B = pix_to_face.shape[0]
    p = pix_to_face.reshape(B, -1).to(torch.int64)
    offs = torch.arange(B, device=p.device, dtype=torch.int64)[:, None] * F
    local = p - offs
    hit = (p >= 0) & (local >= 0) & (local < F)
    vis = torch.zeros((B, F + 1), dtype=torch.bool, device=p.device)
    vis.scatter_(1, torch.where(hit, local, torch.full_like(local, F)), True)
    idx = uvmap_f_idx.to(device=p.device, dtype=torch.int64)
    return vis[:, :F][:, idx] * uvmap_mask.to(p.device)
