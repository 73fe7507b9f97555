"""Numpy restatement of the feature lifting's semantics (include/gsr_lift.h), forward and
backward.

`dtype` selects the arithmetic: np.float32 evaluates the kernels' expressions op for op (every numpy
ufunc rounds once, numpy fuses nothing, `/` is correctly rounded), np.float64 is the same recipe in
double.  Constants are the float32 constants of the contract in both.

The backward multiplies weight and gradient in `dtype` (the kernel's product) and accumulates the
products in float64 with np.add.at; beside dfeat it returns, per feature-map pixel, the number of taps
`n` [B,H,W] and the float64 sum `S` [B,C,H,W] of |w*dout|, from which the GPU test derives its bound.
"""
import numpy as np

TAP_DX = np.array([0, 1, 0, 1])
TAP_DY = np.array([0, 0, 1, 1])


def project(points, w2c, tanfovx, tanfovy, W, H, T=np.float32):
    """points [N,3], w2c [4,4] -> (xn, yn, ix, iy), each [N] of dtype T."""
    c = lambda v: T(np.float32(v))  # noqa: E731
    v = np.asarray(points).astype(T)
    M = np.asarray(w2c, np.float32).astype(T)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        def row(r):
            return (M[r, 0] * x + M[r, 1] * y) + (M[r, 2] * z + M[r, 3])
        xv, yv, zv = row(0), row(1), row(2)
        den = zv + c(1e-7)
        xn = xv / (den * c(tanfovx))
        yn = yv / (den * c(tanfovy))
        ix = ((xn + T(1)) * T(W) - T(1)) * T(0.5)
        iy = ((yn + T(1)) * T(H) - T(1)) * T(0.5)
    assert ix.dtype == T and iy.dtype == T
    return xn, yn, ix, iy


def taps(ix, iy, W, H, border, live=None):
    """Steps 1-4 of the header at pixel coordinates (ix, iy) [N]: dict of w [N,4] (w00, w10, w01, w11),
    tx / ty int64 [N,4] (tap coordinates), mask bool [N,4] (tap inside the image of a live sample) and
    live bool [N] (the sample is not all zeros).  `live` [N] pre-masks samples (UV zero rules)."""
    T = ix.dtype.type
    with np.errstate(all="ignore"):
        ok = np.isfinite(ix) & np.isfinite(iy)
        if live is not None:
            ok &= live
        x = np.where(ok, ix, T(0))
        y = np.where(ok, iy, T(0))
        if border:
            x = np.minimum(np.maximum(x, T(0)), T(W - 1))
            y = np.minimum(np.maximum(y, T(0)), T(H - 1))
        else:
            ok &= (x > T(-1)) & (x < T(W)) & (y > T(-1)) & (y < T(H))
            x = np.where(ok, x, T(0))
            y = np.where(ok, y, T(0))
        x0, y0 = np.floor(x), np.floor(y)
        wx1, wx0 = x - x0, (x0 + T(1)) - x
        wy1, wy0 = y - y0, (y0 + T(1)) - y
        w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], 1)
    assert w.dtype == T
    tx = x0.astype(np.int64)[:, None] + TAP_DX
    ty = y0.astype(np.int64)[:, None] + TAP_DY
    mask = ok[:, None] & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    return dict(w=w, tx=tx, ty=ty, mask=mask, live=ok, ix=ix, iy=iy)


def gather(feat_b, tp):
    """Step 5: feat_b [C,H,W] (dtype T) sampled at taps tp -> [N,C] of dtype T."""
    C, H, W = feat_b.shape
    T = feat_b.dtype.type
    flat = feat_b.reshape(C, H * W)
    t = []
    for k in range(4):
        pix = np.where(tp["mask"][:, k], tp["ty"][:, k] * W + tp["tx"][:, k], 0)
        val = tp["w"][:, k][:, None] * flat[:, pix].T
        t.append(np.where(tp["mask"][:, k][:, None], val, T(0)))
    out = ((t[0] + t[1]) + t[2]) + t[3]
    assert out.dtype == T
    return out


def uv_points(verts_b, faces, texel_face, texel_bary, face_visible_b=None, T=np.float32):
    """The UV path's sample points of one frame: (p [T,3] dtype T, live bool [T]) by the zero rules."""
    faces = np.asarray(faces, np.int64)
    tf = np.asarray(texel_face, np.int64)
    F, V = faces.shape[0], verts_b.shape[0]
    live = (tf >= 0) & (tf < F)
    f = np.where(live, tf, 0)
    idx = faces[f]
    live &= ((idx >= 0) & (idx < V)).all(1)
    if face_visible_b is not None:
        live &= np.asarray(face_visible_b)[f] != 0
    idx = np.where(live[:, None], idx, 0)
    v = np.asarray(verts_b).astype(T)
    b = np.asarray(texel_bary, np.float32).astype(T)
    with np.errstate(all="ignore"):
        p = (b[:, 0:1] * v[idx[:, 0]] + b[:, 1:2] * v[idx[:, 1]]) + b[:, 2:3] * v[idx[:, 2]]
    assert p.dtype == T
    return p, live


def _fov(t, B):
    return np.broadcast_to(np.asarray(t, np.float32), (B,))


def vertex_taps(verts, w2c, tanfovx, tanfovy, W, H, dtype=np.float32):
    """Per frame: (taps dict, ndc [V,2])."""
    B = verts.shape[0]
    tx, ty = _fov(tanfovx, B), _fov(tanfovy, B)
    out = []
    for b in range(B):
        xn, yn, ix, iy = project(verts[b], w2c[b], tx[b], ty[b], W, H, dtype)
        out.append((taps(ix, iy, W, H, True), np.stack([xn, yn], 1)))
    return out


def uv_taps(verts, faces, texel_face, texel_bary, w2c, tanfovx, tanfovy, W, H, face_visible=None, dtype=np.float32):
    B = verts.shape[0]
    tx, ty = _fov(tanfovx, B), _fov(tanfovy, B)
    out = []
    for b in range(B):
        p, live = uv_points(verts[b], faces, texel_face, texel_bary,
                            None if face_visible is None else face_visible[b], dtype)
        _, _, ix, iy = project(p, w2c[b], tx[b], ty[b], W, H, dtype)
        out.append(taps(ix, iy, W, H, False, live))
    return out


def lift_vertices(verts, w2c, tanfovx, tanfovy, feat, dtype=np.float32):
    """-> dict(out [B,V,C], ndc [B,V,2], taps [per frame])."""
    B, C, H, W = feat.shape
    fr = vertex_taps(verts, w2c, tanfovx, tanfovy, W, H, dtype)
    out = np.stack([gather(np.asarray(feat[b]).astype(dtype), fr[b][0]) for b in range(B)])
    return dict(out=out, ndc=np.stack([f[1] for f in fr]), taps=[f[0] for f in fr])


def lift_uv(verts, faces, texel_face, texel_bary, w2c, tanfovx, tanfovy, feat, face_visible=None, dtype=np.float32):
    """-> dict(out [B,C,T], taps [per frame])."""
    B, C, H, W = feat.shape
    fr = uv_taps(verts, faces, texel_face, texel_bary, w2c, tanfovx, tanfovy, W, H, face_visible, dtype)
    out = np.stack([gather(np.asarray(feat[b]).astype(dtype), fr[b]).T for b in range(B)])
    return dict(out=np.ascontiguousarray(out), taps=fr)


def scatter(tps, douts, C, H, W):
    """Backward over frames: tps[b] a taps dict, douts[b] [N,C] (dtype of the weights) ->
    dict(dfeat float64 [B,C,H,W], n int64 [B,H,W], S float64 [B,C,H,W])."""
    B = len(tps)
    dfeat = np.zeros((B, H * W, C))
    S = np.zeros((B, H * W, C))
    n = np.zeros((B, H * W), np.int64)
    for b, (tp, d) in enumerate(zip(tps, douts)):
        T = tp["w"].dtype.type
        d = np.asarray(d).astype(T)
        for k in range(4):
            m = tp["mask"][:, k]
            pix = (tp["ty"][:, k] * W + tp["tx"][:, k])[m]
            prod = (tp["w"][:, k][m][:, None] * d[m]).astype(np.float64)  # rounded in T, summed in double
            np.add.at(dfeat[b], pix, prod)
            np.add.at(S[b], pix, np.abs(prod))
            np.add.at(n[b], pix, 1)
    tr = lambda a: np.ascontiguousarray(a.reshape(B, H, W, C).transpose(0, 3, 1, 2))  # noqa: E731
    return dict(dfeat=tr(dfeat), n=n.reshape(B, H, W), S=tr(S))


def lift_vertices_backward(verts, w2c, tanfovx, tanfovy, dout, C, W, H, dtype=np.float32):
    """dout [B,V,C] -> scatter() dict."""
    fr = vertex_taps(verts, w2c, tanfovx, tanfovy, W, H, dtype)
    return scatter([f[0] for f in fr], [dout[b] for b in range(len(fr))], C, H, W)


def lift_uv_backward(verts, faces, texel_face, texel_bary, w2c, tanfovx, tanfovy, dout, W, H, face_visible=None,
                     dtype=np.float32):
    """dout [B,C,T] -> scatter() dict."""
    fr = uv_taps(verts, faces, texel_face, texel_bary, w2c, tanfovx, tanfovy, W, H, face_visible, dtype)
    return scatter(fr, [dout[b].T for b in range(len(fr))], dout.shape[1], H, W)
