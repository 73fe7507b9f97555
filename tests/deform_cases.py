"""Inputs of the assembly-backward tests: a random-soup mesh posed in B frames, built as
test_gpu_deform.py::test_fused_deform_forward_equals_two_step_and_flags_bad_index builds its avatar
(verts ~ N(0, 0.25), T = I + N(0, 0.1) on its 3x3 block), with NON-unit vertex rotations (unit
quaternions times a factor in [0.5, 2]) so that the normalise backward's projection term is exercised."""
import numpy as np


def quats(rng, n):
    q = rng.normal(size=(n, 4)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def make_case(seed, V, F, N, B, sort_bindings=False, per_frame=()):
    """dict of float32 / int32 numpy inputs.  per_frame: names of the canonical attributes given per
    frame ([B,n,k]); the others are shared ([n,k]).  The scale ranges are the fused-forward test's, so
    the avatar renders."""
    rng = np.random.default_rng(seed)
    faces = np.stack([rng.choice(V, 3, replace=False) for _ in range(F)]).astype(np.int32)
    bind = rng.integers(0, F, N).astype(np.int32)
    if sort_bindings:
        bind = np.sort(bind)
    c = dict(V=V, F=F, N=N, B=B, faces=faces, binding_face=bind)
    c["vtx_rotations"] = (quats(rng, V) * rng.uniform(0.5, 2.0, (V, 1))).astype(np.float32)
    c["vtx_scales"] = rng.uniform(0.005, 0.03, (V, 3)).astype(np.float32)
    c["uv_rotations"] = quats(rng, N)
    c["uv_scales"] = rng.uniform(0.1, 1.5, (N, 3)).astype(np.float32)
    c["local_xyz"] = rng.normal(scale=0.01, size=(N, 3)).astype(np.float32)
    c["face_bary"] = rng.dirichlet(np.ones(3), N).astype(np.float32)
    c["opacities"] = rng.uniform(0.2, 0.95, (V + N, 1)).astype(np.float32)
    c["colors"] = rng.uniform(0, 1, (V + N, 32)).astype(np.float32)
    c["verts"] = rng.normal(scale=0.25, size=(B, V, 3)).astype(np.float32)
    T = np.broadcast_to(np.eye(4, dtype=np.float32), (B, V, 4, 4)).copy()
    T[..., :3, :3] += rng.normal(scale=0.1, size=(B, V, 3, 3)).astype(np.float32)
    c["vert_transforms"] = T
    for name in per_frame:  # every frame its own values, of the shared table's magnitude
        a = c[name]
        c[name] = (a[None] * rng.uniform(0.7, 1.3, (B,) + a.shape)).astype(np.float32)
    P = V + N
    c["g_xyz"] = rng.normal(size=(B, P, 3)).astype(np.float32)
    c["g_rot"] = rng.normal(size=(B, P, 4)).astype(np.float32)
    c["g_scl"] = rng.normal(size=(B, P, 3)).astype(np.float32)
    return c


ATTRS = ("vtx_rotations", "vtx_scales", "local_xyz", "uv_rotations", "uv_scales")
ROT_ATTRS = ("vtx_rotations", "uv_rotations")


def block_face_runs(c):
    """Face-run length (max - min + 1 of the bound faces) of every 256-Gaussian block that holds a UV
    Gaussian: <= 256 lets a kernel share face frames per block, > 256 forces the per-Gaussian path."""
    V, P = c["V"], c["V"] + c["N"]
    runs = []
    for b0 in range(0, P, 256):
        n0, n1 = max(b0 - V, 0), min(b0 + 256, P) - V
        if n1 > n0:
            f = c["binding_face"][n0:n1]
            runs.append(int(f.max() - f.min() + 1))
    return runs
