// lift_dev.h -- the per-sample arithmetic of the feature lifting (include/gsr_lift.h): projection,
// guards, tap offsets and weights, as host/device inline functions.  lift.hip's kernels call them on
// the device; tools/lift_check.cpp calls the very same functions on the host under the sanitizers, with
// the tap loads made from exactly sized heap arrays.  Every operation is float32, written with all of
// its parentheses; the build compiles with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_LIFT_HD __host__ __device__ __forceinline__
#else
#define GSR_LIFT_HD inline
#endif

namespace gsr {

// One bilinear sample: taps k = 0..3 at (x0 + (k & 1), y0 + (k >> 1)) with weights w[k]
// (w00, w10, w01, w11).  Bit k of `mask` is set iff tap k lies inside the image: only those taps may
// be loaded.  mask == 0: the sample is all zeros (x0, y0 and w are then meaningless).
struct LiftSample {
    float w[4];
    int x0, y0;
    unsigned mask;
};

// gsr_mesh.h's camera: view transform by M = w2c[b] (row-major 4x4), NDC (xn, yn), pixel (ix, iy)
GSR_LIFT_HD void lift_project(const float* M, float tanfovx, float tanfovy, int W, int H, float x, float y, float z,
                              float& xn, float& yn, float& ix, float& iy) {
    const float xv = (M[0] * x + M[1] * y) + (M[2] * z + M[3]);
    const float yv = (M[4] * x + M[5] * y) + (M[6] * z + M[7]);
    const float zv = (M[8] * x + M[9] * y) + (M[10] * z + M[11]);
    const float den = zv + 1e-7f;
    xn = xv / (den * tanfovx);
    yn = yv / (den * tanfovy);
    ix = ((xn + 1.0f) * (float)W - 1.0f) * 0.5f;
    iy = ((yn + 1.0f) * (float)H - 1.0f) * 0.5f;
}

// torch grid_sample's bilinear taps (align_corners = False) at pixel coordinates (ix, iy); border != 0:
// padding_mode 'border', else 'zeros'.  Every guard is made in float before any conversion to int:
// behind them ix lies in (-1, W) and iy in (-1, H), W, H <= 16384, so floorf() converts exactly.
GSR_LIFT_HD LiftSample lift_taps(float ix, float iy, int W, int H, int border) {
    LiftSample s;
    s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.0f;
    s.x0 = s.y0 = 0;
    s.mask = 0u;
    if (!(isfinite(ix) && isfinite(iy))) return s;
    if (border) {
        ix = fminf(fmaxf(ix, 0.0f), (float)(W - 1));
        iy = fminf(fmaxf(iy, 0.0f), (float)(H - 1));
    } else if (!(ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H)) {
        return s;
    }
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float wx1 = ix - x0, wx0 = (x0 + 1.0f) - ix;
    const float wy1 = iy - y0, wy0 = (y0 + 1.0f) - iy;
    s.w[0] = wx0 * wy0;
    s.w[1] = wx1 * wy0;
    s.w[2] = wx0 * wy1;
    s.w[3] = wx1 * wy1;
    s.x0 = (int)x0;
    s.y0 = (int)y0;
    const bool xa = s.x0 >= 0 && s.x0 < W, xb = s.x0 + 1 >= 0 && s.x0 + 1 < W;
    const bool ya = s.y0 >= 0 && s.y0 < H, yb = s.y0 + 1 >= 0 && s.y0 + 1 < H;
    s.mask = (xa && ya ? 1u : 0u) | (xb && ya ? 2u : 0u) | (xa && yb ? 4u : 0u) | (xb && yb ? 8u : 0u);
    return s;
}

// element offset of tap k inside one H x W plane (valid only when bit k of the mask is set)
GSR_LIFT_HD int lift_tap_offset(const LiftSample& s, int k, int W) { return (s.y0 + (k >> 1)) * W + (s.x0 + (k & 1)); }

// the sample of one tap plane: ((t00 + t10) + t01) + t11, t = w * plane[tap] inside the image, +0 outside
GSR_LIFT_HD float lift_sample_plane(const LiftSample& s, const float* plane, int W) {
    const float t00 = (s.mask & 1u) ? s.w[0] * plane[lift_tap_offset(s, 0, W)] : 0.0f;
    const float t10 = (s.mask & 2u) ? s.w[1] * plane[lift_tap_offset(s, 1, W)] : 0.0f;
    const float t01 = (s.mask & 4u) ? s.w[2] * plane[lift_tap_offset(s, 2, W)] : 0.0f;
    const float t11 = (s.mask & 8u) ? s.w[3] * plane[lift_tap_offset(s, 3, W)] : 0.0f;
    return ((t00 + t10) + t01) + t11;
}

// UV path: the point of texel t on its face, p_k = (bary0*v0_k + bary1*v1_k) + bary2*v2_k.  False (the
// texel is zeros) for a masked texel (face < 0), a face >= F, a vertex index outside [0, V) and a face
// that `face_visible_b` (this frame's [F] row, may be null) marks 0.  Nothing outside the arrays'
// bounds is read.
GSR_LIFT_HD bool lift_uv_point(const float* verts_b, const int32_t* faces, const int32_t* texel_face,
                               const float* texel_bary, const uint8_t* face_visible_b, int V, int F, int t,
                               float p[3]) {
    const int f = texel_face[t];
    if (f < 0 || f >= F) return false;
    const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
    if (face_visible_b && face_visible_b[f] == 0) return false;
    const float b0 = texel_bary[3 * (int64_t)t], b1 = texel_bary[3 * (int64_t)t + 1], b2 = texel_bary[3 * (int64_t)t + 2];
    const float* v0 = verts_b + 3 * (int64_t)i0;
    const float* v1 = verts_b + 3 * (int64_t)i1;
    const float* v2 = verts_b + 3 * (int64_t)i2;
    for (int k = 0; k < 3; ++k) p[k] = (b0 * v0[k] + b1 * v1[k]) + b2 * v2[k];
    return true;
}

// the whole geometry of a UV sample of frame b (zeros mode): mask == 0 when the texel is zeros
GSR_LIFT_HD LiftSample lift_uv_sample(const float* verts_b, const int32_t* faces, const int32_t* texel_face,
                                      const float* texel_bary, const uint8_t* face_visible_b, const float* M,
                                      float tanfovx, float tanfovy, int V, int F, int W, int H, int t) {
    float p[3];
    if (!lift_uv_point(verts_b, faces, texel_face, texel_bary, face_visible_b, V, F, t, p)) {
        LiftSample s;
        s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.0f;
        s.x0 = s.y0 = 0;
        s.mask = 0u;
        return s;
    }
    float xn, yn, ix, iy;
    lift_project(M, tanfovx, tanfovy, W, H, p[0], p[1], p[2], xn, yn, ix, iy);
    return lift_taps(ix, iy, W, H, 0);
}

// the whole geometry of a vertex sample (border mode); (xn, yn) is the reference's vertices_img[..., :2]
GSR_LIFT_HD LiftSample lift_vertex_sample(const float* vert, const float* M, float tanfovx, float tanfovy, int W, int H,
                                          float& xn, float& yn) {
    float ix, iy;
    lift_project(M, tanfovx, tanfovy, W, H, vert[0], vert[1], vert[2], xn, yn, ix, iy);
    return lift_taps(ix, iy, W, H, 1);
}

}  // namespace gsr
