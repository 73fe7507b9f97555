"""Inputs shared by the mesh rasterizer's CPU and GPU tests (test_mesh_raster_ref.py,
test_gpu_mesh_raster.py): hand-built scenes in pixel coordinates and the template-mesh cameras.

Exact pixel coordinates: with w2c = I, tanfov = 0.5 and z in {2, 4}, den = z + 1e-7f rounds to z in
float32 and den*tanfov is a power of two, so a vertex placed at x = ((2*px + 1)/W - 1) * (z/2) lands
on px exactly when px is a small integer (z = 1 with tanfov = 1 would not do: 1 + 1e-7f rounds to
1 + 2^-23 in float32, which moves every vertex by a few 1e-7 pixels)."""
import functools

import numpy as np

TANFOV_EXACT = 0.5
EYE = np.eye(4, dtype=np.float32)


def pixel_verts(pts, W, H):
    """[(px, py, z), ...] -> world vertices [n,3] f32 that project there under w2c = I, tanfov = 0.5."""
    p = np.asarray(pts, np.float64)
    s = p[:, 2] * TANFOV_EXACT
    x = ((2.0 * p[:, 0] + 1.0) / W - 1.0) * s
    y = ((2.0 * p[:, 1] + 1.0) / H - 1.0) * s
    return np.stack([x, y, p[:, 2]], 1).astype(np.float32)


# far corner of the edge case's square, by image height: (2*py + 1)/H must be a dyadic fraction for py
# to be exact, which at H = 24 holds for py = 1, 4, 7, 10, 13, ... only
EDGE_HI = {8: 5, 24: 13}


def edge_points(H):
    lo, hi = 1, EDGE_HI[H]
    return [(lo, lo, 2), (hi, lo, 2), (hi, hi, 2), (lo, hi, 2)]


def edge_scene(W=8, H=8):
    """Two triangles sharing the diagonal of the square (1,1)-(hi,hi), hi = EDGE_HI[H], z = 2: every
    pixel coordinate is an exact integer.  faces 0 = (A,B,C), 1 = (A,C,D)."""
    return pixel_verts(edge_points(H), W, H), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


# names of hand_scene's faces, by index
HAND_FACES = ("edge_a", "edge_b", "big_a", "big_b", "dup_0", "dup_1", "zero_area", "behind", "offscreen",
              "huge", "subpixel")


def hand_scene(W, H):
    """The GPU test's hand-built scene at W x H (multiples of 8): (verts [V,3], faces [F,3]), w2c = I,
    tanfov = 0.5.  Faces as HAND_FACES:
      edge_a/b   the integer-coordinate edge case (edge_scene), z = 2, in front
      big_a/b    two large interpenetrating triangles with opposite depth slopes (wide path)
      dup_0/1    one triangle twice (the lower index wins)
      zero_area, behind (z < 0), offscreen   never appear
      huge       larger than the image: the box clamps to the image, wide path
      subpixel   inside one pixel, holding no centre, nearest of all (would show if it were covered)."""
    sx, sy = W / 8.0, H / 8.0
    S = lambda pts: [(x * sx, y * sy, z) for x, y, z in pts]  # noqa: E731
    pts, faces = [], []

    def add(tri):
        faces.append([len(pts), len(pts) + 1, len(pts) + 2])
        pts.extend(tri)
    pts.extend(edge_points(H))
    faces.extend([[0, 1, 2], [0, 2, 3]])
    add(S([(-0.5, -0.3, 2.6), (7.7, 0.2, 4.4), (3.4, 7.8, 3.3)]))
    add(S([(7.9, 7.5, 2.7), (-0.4, 6.9, 4.1), (4.2, -0.6, 3.2)]))
    dup = S([(5.5, 5.5, 2.5), (7.5, 5.6, 2.5), (6.4, 7.6, 2.25)])
    add(dup)
    faces.append(list(faces[-1]))
    add(S([(2.0, 3.0, 2.2), (4.0, 5.0, 2.2), (3.0, 4.0, 2.2)]))
    add(S([(2.0, 2.0, -3.0), (6.0, 2.5, -3.0), (3.0, 6.0, -3.0)]))
    add(S([(50.0, 52.0, 3.0), (60.0, 53.0, 3.0), (55.0, 61.0, 3.0)]))
    add(S([(-20.0, -15.0, 6.0), (40.0, -10.0, 6.0), (5.0, 60.0, 6.0)]))
    add([(2.2, 6.2, 1.5), (2.7, 6.3, 1.5), (2.4, 6.8, 1.5)])
    assert len(faces) == len(HAND_FACES)
    return pixel_verts(pts, W, H), np.asarray(faces, np.int32)


@functools.lru_cache(maxsize=None)
def template():
    from guava_renderer_amd import avatar
    v, f, _ = avatar.template_mesh()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def template_fov(W, H, focal=24.0):
    """(tanfovx, tanfovy) = 1/focal scaled by side/min(W, H): the shorter side spans NDC [-1, 1]."""
    m = float(min(W, H))
    return (W / m) / focal, (H / m) / focal


def template_camera(yaw, dist):
    from guava_renderer_amd import camera
    return camera.look_at_w2c(yaw, 0.1, dist)


# (W, H, yaw, distance) of the float32-against-float64 comparison
F32_F64_INPUTS = ((64, 64, 0.0, 22.0), (96, 64, 0.7, 22.0), (128, 128, 2.5, 22.0), (64, 48, 0.3, 4.0),
                  (256, 256, 0.0, 22.0))


def posed_batch(cams, seed=0, scale=0.01):
    """Per-frame posed vertices (template + a small smooth per-frame offset) and cameras for
    cams = ((yaw, dist), ...): (verts [B,V,3] f32, w2c [B,4,4] f32)."""
    v, _ = template()
    rng = np.random.default_rng(seed)
    out = []
    for _ in cams:
        a, ph = rng.normal(0, scale, (3, 3)), rng.uniform(0, 6.28, 3)
        out.append((v + np.sin(v @ a.T * 40.0 + ph) * scale).astype(np.float32))
    w2c = np.stack([template_camera(y, d) for y, d in cams]).astype(np.float32)
    return np.stack(out), w2c
