"""Float64 torch restatement of Ubody_Gaussian.forward's Gaussian assembly
(models/UbodyAvatar/ubody_gaussian.py:252-278), differentiable by autograd with respect to the
canonical attributes: the reference of every gradient test of the assembly's backward.

The face orientation and scale and the two rotmat_to_unitquat results come from oracle/lbs_oracle.py
as plain (non-differentiated) tensors -- exactly what the GPU backward treats as constant
(include/gsr_deform.h): nothing differentiates through the mesh."""
import numpy as np
import torch

import lbs_oracle as lo


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def quat_product(p, q):
    """roma.quat_product (xyzw)."""
    v = p[..., 3:] * q[..., :3] + q[..., 3:] * p[..., :3] + torch.linalg.cross(p[..., :3], q[..., :3])
    w = p[..., 3] * q[..., 3] - (p[..., :3] * q[..., :3]).sum(-1)
    return torch.cat([v, w[..., None]], -1)


def _xyzw(q):
    return torch.cat([q[..., 1:], q[..., :1]], -1)


def _wxyz(q):
    return torch.cat([q[..., 3:], q[..., :3]], -1)


class Constants:
    """What the assembly takes from the deformed mesh, float64, no graph."""

    def __init__(self, verts, vert_transforms, faces, binding_face, face_bary):
        verts = np.asarray(verts, np.float64)
        self.B, self.V = verts.shape[:2]
        bind = np.asarray(binding_face).astype(np.int64)
        faces = np.asarray(faces).astype(np.int64)
        qd, m_v = lo.rotmat_to_unitquat(np.asarray(vert_transforms, np.float64)[:, :, :3, :3])
        orient, fscale = lo.face_orientation(verts, faces)
        qf, m_f = lo.rotmat_to_unitquat(orient)
        self.verts = _t(verts)
        self.qd = _t(qd)                                   # [B,V,4] xyzw
        self.orient = _t(orient[:, bind])                  # [B,N,3,3]
        self.s = _t(fscale[:, bind])                       # [B,N,1]
        self.qf = _t(qf[:, bind])                          # [B,N,4] xyzw
        self.centre = _t(np.einsum("nk,bnkj->bnj", np.asarray(face_bary, np.float64), verts[:, faces][:, bind]))
        self.margin = np.concatenate([m_v, m_f[:, bind]], 1)  # [B,P] decision margins


def forward(c, vtx_rotations, vtx_scales, local_xyz, uv_rotations, uv_scales):
    """(xyz [B,P,3], rotation [B,P,4] wxyz, scaling [B,P,3]) of float64 attribute tensors, each [n,k]
    (shared) or [B,n,k]."""
    def pf(x):
        return x.expand((c.B,) + tuple(x.shape)) if x.dim() == 2 else x

    qv = _wxyz(quat_product(c.qd, _xyzw(pf(vtx_rotations))))
    qv = qv / qv.norm(dim=-1, keepdim=True).clamp_min(1e-12)  # F.normalize
    xyz = torch.einsum("bnij,bnj->bni", c.orient, pf(local_xyz)) * c.s + c.centre
    qu = _wxyz(quat_product(c.qf, _xyzw(pf(uv_rotations))))
    return (torch.cat([c.verts, xyz], 1), torch.cat([qv, qu], 1),
            torch.cat([pf(vtx_scales), pf(uv_scales) * c.s], 1))


ATTRS = ("vtx_rotations", "vtx_scales", "local_xyz", "uv_rotations", "uv_scales")


def gradients(c, attrs, g_xyz, g_rot, g_scl):
    """Float64 gradients (numpy, in ATTRS order) of sum(<g, output>) with respect to `attrs` (numpy,
    ATTRS order, [n,k] or [B,n,k])."""
    leaves = [_t(a).clone().requires_grad_(True) for a in attrs]
    xyz, rot, scl = forward(c, *leaves)
    loss = (xyz * _t(g_xyz)).sum() + (rot * _t(g_rot)).sum() + (scl * _t(g_scl)).sum()
    loss.backward()
    return [l.grad.numpy() for l in leaves]
