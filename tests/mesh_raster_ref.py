"""Numpy restatement of the mesh visibility rasterizer's semantics (include/gsr_mesh.h):
PyTorch3D's fine rasterizer at blur_radius = 0, faces_per_pixel = 1, perspective_correct = True, in this
project's camera convention.

`dtype` selects the arithmetic: np.float32 evaluates the kernel's expressions op for op (every numpy
ufunc rounds once, numpy fuses nothing, `/` is correctly rounded), np.float64 is the ground truth the
float32 result is judged against.  Constants are the float32 constants of the contract in both.

The candidate (face, pixel) pairs of all faces are expanded into flat arrays (each face's clipped
bounding box, in chunks) and evaluated at once; the winner of a pixel is the first pair in
(pz, face index) order.
"""
import numpy as np

LANE_BOX = 16  # csrc/mesh_raster.hip kLaneBox: boxes up to this many pixel centres stay on the face's lane


def _project(verts, w2c, tanfovx, tanfovy, W, H, T):
    c = lambda v: T(np.float32(v))  # noqa: E731
    v = np.asarray(verts, np.float32).astype(T)
    M = np.asarray(w2c, np.float32).astype(T)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]

    def row(r):
        return (M[r, 0] * x + M[r, 1] * y) + (M[r, 2] * z + M[r, 3])
    xv, yv, zv = row(0), row(1), row(2)
    den = zv + c(1e-7)
    xn = xv / (den * c(tanfovx))
    yn = yv / (den * c(tanfovy))
    px = ((xn + T(1)) * T(W) - T(1)) * T(0.5)
    py = ((yn + T(1)) * T(H) - T(1)) * T(0.5)
    assert px.dtype == T and py.dtype == T and zv.dtype == T
    return px, py, zv


def rasterize(verts, faces, w2c, tanfovx, tanfovy, W, H, dtype=np.float32, chunk=1 << 21):
    """One frame.  verts [V,3], faces [F,3], w2c [4,4] -> dict of
      pix_to_face int32 [H,W] (-1 empty), zbuf [H,W] dtype (-1), bary [H,W,3] dtype (-1),
      face_visible uint8 [F],
      min_w [H,W]  the winner's smallest |w_i| before the perspective correction (inf where empty),
      z_gap [H,W]  runner-up pz minus winner pz (inf without a runner-up),
      cond  [H,W]  S / |area| of the winner, S = the sum of the absolute values of the six products of
                   its three edge functions (0 where empty),
      stats (faces on their own lane, faces on the wide path, faces culled, covered pixels)."""
    T = np.dtype(dtype).type
    c = lambda v: T(np.float32(v))  # noqa: E731
    faces = np.asarray(faces, np.int64)
    F, V = faces.shape[0], np.asarray(verts).shape[0]
    with np.errstate(all="ignore"):
        px, py, zv = _project(verts, w2c, tanfovx, tanfovy, W, H, T)
        idx_ok = ((faces >= 0) & (faces < V)).all(1)
        fi = np.where(idx_ok[:, None], faces, 0)
        x0, x1, x2 = px[fi[:, 0]], px[fi[:, 1]], px[fi[:, 2]]
        y0, y1, y2 = py[fi[:, 0]], py[fi[:, 1]], py[fi[:, 2]]
        z0, z1, z2 = zv[fi[:, 0]], zv[fi[:, 1]], zv[fi[:, 2]]
        finite = np.ones(F, bool)
        for a in (x0, x1, x2, y0, y1, y2, z0, z1, z2):
            finite &= np.isfinite(a)
        area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
        thr = c(1e-8) * ((T(W) * T(H)) * T(0.25))
        ok = idx_ok & finite & ~(np.maximum(np.maximum(z0, z1), z2) < 0) & ~(np.abs(area) <= thr)
        z = lambda a: np.where(ok, a, T(0))  # noqa: E731
        xmin, xmax = z(np.minimum(np.minimum(x0, x1), x2)), z(np.maximum(np.maximum(x0, x1), x2))
        ymin, ymax = z(np.minimum(np.minimum(y0, y1), y2)), z(np.maximum(np.maximum(y0, y1), y2))
        xlo = np.clip(np.ceil(xmin), 0, W).astype(np.int64)
        xhi = np.clip(np.floor(xmax), -1, W - 1).astype(np.int64)
        ylo = np.clip(np.ceil(ymin), 0, H).astype(np.int64)
        yhi = np.clip(np.floor(ymax), -1, H - 1).astype(np.int64)
    nx = np.where(ok, np.maximum(xhi - xlo + 1, 0), 0)
    ny = np.where(ok, np.maximum(yhi - ylo + 1, 0), 0)
    n = nx * ny
    n_lane, n_wide, n_cull = int((ok & (n <= LANE_BOX)).sum()), int((ok & (n > LANE_BOX)).sum()), int((~ok).sum())

    sel = np.nonzero(n > 0)[0]
    kept = []
    start = 0
    while start < sel.size:
        cum = np.cumsum(n[sel[start:]])
        stop = start + max(1, int(np.searchsorted(cum, chunk, side="right")))
        s = sel[start:stop]
        cnt = n[s]
        f = np.repeat(s, cnt)
        k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ry = k // nx[f]
        xi, yi = xlo[f] + (k - ry * nx[f]), ylo[f] + ry
        with np.errstate(all="ignore"):
            qx, qy = xi.astype(T), yi.astype(T)
            A = area[f]

            def edge(ax, ay, bx, by):
                p1, p2 = (qx - ax[f]) * (by[f] - ay[f]), (qy - ay[f]) * (bx[f] - ax[f])
                return p1 - p2, np.abs(p1.astype(np.float64)) + np.abs(p2.astype(np.float64))
            e0, s0 = edge(x1, y1, x2, y2)
            e1, s1 = edge(x2, y2, x0, y0)
            e2, s2 = edge(x0, y0, x1, y1)
            w0, w1, w2 = e0 / A, e1 / A, e2 / A
            t0 = (w0 * z1[f]) * z2[f]
            t1 = (z0[f] * w1) * z2[f]
            t2 = (z0[f] * z1[f]) * w2
            d = np.maximum((t0 + t1) + t2, c(1e-8))
            b0, b1, b2 = t0 / d, t1 / d, t2 / d
            pz = (b0 * z0[f] + b1 * z1[f]) + b2 * z2[f]
            keep = (w0 > 0) & (w1 > 0) & (w2 > 0) & (pz >= 0)
            minw = np.minimum(np.minimum(np.abs(w0), np.abs(w1)), np.abs(w2))
            cond = (s0 + s1 + s2) / np.abs(A.astype(np.float64))
        kept.append((f[keep], (yi * W + xi)[keep], np.abs(pz[keep]), b0[keep], b1[keep], b2[keep], minw[keep],
                     cond[keep]))
        start = stop

    out = dict(pix_to_face=np.full(H * W, -1, np.int32), zbuf=np.full(H * W, -1, T),
               bary=np.full((H * W, 3), -1, T), face_visible=np.zeros(F, np.uint8),
               min_w=np.full(H * W, np.inf), z_gap=np.full(H * W, np.inf), cond=np.zeros(H * W))
    covered = 0
    if kept and sum(k[0].size for k in kept):
        f, pix, pz, b0, b1, b2, minw, cond = (np.concatenate(a) for a in zip(*kept))
        order = np.lexsort((f, pz, pix))  # by pixel, then pz, then face index
        f, pix, pz, b0, b1, b2, minw, cond = (a[order] for a in (f, pix, pz, b0, b1, b2, minw, cond))
        first = np.ones(pix.size, bool)
        first[1:] = pix[1:] != pix[:-1]
        w = np.nonzero(first)[0]
        p = pix[w]
        out["pix_to_face"][p] = f[w]
        out["zbuf"][p] = pz[w]
        out["bary"][p] = np.stack([b0[w], b1[w], b2[w]], 1)
        out["face_visible"][f[w]] = 1
        out["min_w"][p] = minw[w]
        out["cond"][p] = cond[w]
        second = w + 1
        has2 = (second < pix.size)
        has2[has2] = pix[second[has2]] == p[has2]
        out["z_gap"][p[has2]] = pz[second[has2]].astype(np.float64) - pz[w[has2]].astype(np.float64)
        covered = int(w.size)
    for k in ("pix_to_face", "zbuf", "min_w", "z_gap", "cond"):
        out[k] = out[k].reshape(H, W)
    out["bary"] = out["bary"].reshape(H, W, 3)
    out["stats"] = (n_lane, n_wide, n_cull, covered)
    return out


def rasterize_batch(verts, faces, w2c, tanfovx, tanfovy, W, H, dtype=np.float32):
    """verts [B,V,3], w2c [B,4,4], tanfovx / tanfovy scalars or [B] -> stacked dict (stats summed)."""
    B = np.asarray(verts).shape[0]
    tx = np.broadcast_to(np.asarray(tanfovx, np.float32), (B,))
    ty = np.broadcast_to(np.asarray(tanfovy, np.float32), (B,))
    frames = [rasterize(verts[b], faces, w2c[b], tx[b], ty[b], W, H, dtype) for b in range(B)]
    out = {k: np.stack([fr[k] for fr in frames]) for k in frames[0] if k != "stats"}
    out["stats"] = tuple(int(sum(fr["stats"][i] for fr in frames)) for i in range(4))
    out["frame_stats"] = [fr["stats"] for fr in frames]
    return out
