"""Seeded inputs shared by the feature lifting's CPU and GPU tests (test_feature_lift_ref.py,
test_gpu_feature_lift.py), built from what the tree has: the template mesh with per-frame posed
vertices and cameras (mesh_raster_cases), the template's texels-per-face counts, and the face
visibility of the mesh rasterizer's restatement (mesh_raster_ref).

UV layout of uv_layout(): face_of = repeat(arange(F), texel_count); a sorted random 75% of the U*U
texels are placed, each on a face drawn from face_of in order (so neighbouring texels lie on the same
or neighbouring faces, as in a UV atlas); the rest get -1 (uvmap_mask == 0).  Half of the placed texels
are then re-bound to faces that the rasterizer reports visible, drawn from the frames' visible lists
with the frames in turn.  At these small image sizes only a few per cent of the 20,908 faces win a
pixel, and without the re-binding nearly every texel would be masked by visibility.  The cameras look
from different sides and a face is rarely seen by two of them, so about half of the placed texels are
visible in some frame (shares()["visible"], what the GPU test's 20-80% condition is about) and a
sixth to a quarter in any one frame (shares()["visible_frames"]).  Barycentrics are Dirichlet(1,1,1).
"""
import functools

import numpy as np

import feature_lift_ref as ref
import mesh_raster_cases as mc
import mesh_raster_ref as mref

CAMS_A = ((0.0, 22.0), (0.7, 22.0), (2.5, 12.0))
CAMS_B = ((0.3, 8.0), (0.0, 22.0), (2.5, 12.0))
# (W, H, C, U, cameras) of the GPU test's seeded cases; B = 3 everywhere
CASES = ((64, 64, 5, 32, CAMS_A), (96, 64, 35, 48, CAMS_A), (24, 16, 1, 32, CAMS_B), (24, 16, 128, 32, CAMS_B))


def texel_counts():
    from guava_renderer_amd import avatar
    return avatar.template_mesh()[2]


def uv_layout(U, faces, face_visible, seed):
    """-> (texel_face int32 [U*U] with -1 = masked, texel_bary f32 [U*U,3], uvmap_mask f32 [U*U])."""
    rng = np.random.default_rng(seed)
    F = faces.shape[0]
    face_of = np.repeat(np.arange(F), texel_counts())
    n = U * U
    n_placed = (3 * n) // 4
    placed = np.sort(rng.choice(n, n_placed, replace=False))
    texel_face = np.full(n, -1, np.int64)
    texel_face[placed] = face_of[(np.arange(n_placed) * face_of.size) // n_placed]
    lists = [np.nonzero(v)[0] for v in face_visible]
    assert all(own.size for own in lists)
    rebound = rng.choice(placed, n_placed // 2, replace=False)
    for j, t in enumerate(rebound):  # the frames in turn, so that a frame with few visible faces gets its share
        own = lists[j % len(lists)]
        texel_face[t] = own[rng.integers(0, own.size)]
    bary = rng.dirichlet((1.0, 1.0, 1.0), n).astype(np.float32)
    return texel_face.astype(np.int32), bary, (texel_face >= 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def geometry(W, H, U, cams, seed=3):
    """The geometry of one case, made once and read-only: dict of verts [B,V,3], faces [F,3], w2c
    [B,4,4], tx / ty [B] (per frame), face_visible uint8 [B,F], texel_face [U*U], texel_bary [U*U,3],
    uvmap_mask [U*U]."""
    verts, w2c = mc.posed_batch(cams, seed=seed)
    _, faces = mc.template()
    tx, ty = mc.template_fov(W, H)
    tx = np.float32(tx) * np.array([1.0, 1.05, 1.0], np.float32)[:len(cams)]
    ty = np.float32(ty) * np.array([1.0, 1.0, 0.95], np.float32)[:len(cams)]
    vis = mref.rasterize_batch(verts, faces, w2c, tx, ty, W, H)["face_visible"]
    tf, tb, mask = uv_layout(U, faces, vis, seed + 100)
    g = dict(verts=verts, faces=np.array(faces), w2c=w2c, tx=tx, ty=ty, face_visible=vis, texel_face=tf, texel_bary=tb,
             uvmap_mask=mask)
    for a in g.values():
        a.setflags(write=False)
    return g


def features(B, C, H, W, seed):
    """A feature map [B,C,H,W] f32: smooth waves plus noise, of order 1."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a = rng.uniform(0.05, 0.4, (B, C, 2, 1, 1)).astype(np.float32)
    f = np.sin(a[:, :, 0] * x + rng.uniform(0, 6, (B, C, 1, 1)).astype(np.float32)) * np.cos(a[:, :, 1] * y)
    return (f + 0.3 * rng.standard_normal((B, C, H, W))).astype(np.float32)


def gradient(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def shares(g, W, H):
    """What a case asserts about itself on the restatement alone: dict of
    masked (share of texels with uvmap_mask == 0), visible (share of the placed texels on a face that
    some frame sees), visible_frames (that share per frame), uv_outside / vertex_outside (share of the samples fully outside the image: for the
    UV path among the placed texels with no visibility term, zeros mode; for the vertices, clamped by
    the border mode), partial (share of those UV samples with one to three taps outside), max_taps (the
    most taps on one feature-map pixel, UV path without visibility)."""
    B = g["verts"].shape[0]
    tf = g["texel_face"]
    placed = tf >= 0
    vis = np.stack([g["face_visible"][b][np.where(placed, tf, 0)] != 0 for b in range(B)]) & placed
    # every placed texel samples when no visibility term is given (face_visible = NULL)
    fr = ref.uv_taps(g["verts"], g["faces"], tf, g["texel_bary"], g["w2c"], g["tx"], g["ty"], W, H, None)
    n_in = np.stack([t["mask"].sum(1) for t in fr])
    cand = B * placed.sum()
    npix = np.zeros((B, H * W), np.int64)
    for b, t in enumerate(fr):
        for k in range(4):
            m = t["mask"][:, k]
            np.add.at(npix[b], (t["ty"][:, k] * W + t["tx"][:, k])[m], 1)
    vout = 0
    for b in range(B):
        _, _, ix, iy = ref.project(g["verts"][b], g["w2c"][b], g["tx"][b], g["ty"][b], W, H)
        vout += (~((ix > -1) & (ix < W) & (iy > -1) & (iy < H))).sum()
    return dict(masked=float((~placed).mean()), visible=float(vis.any(0).sum() / placed.sum()),
                visible_frames=[float(v.sum() / placed.sum()) for v in vis],
                uv_outside=float((placed & (n_in == 0)).sum() / cand),
                vertex_outside=float(vout / (B * g["verts"].shape[1])),
                partial=float((placed & (n_in > 0) & (n_in < 4)).sum() / cand), max_taps=int(npix.max()))
