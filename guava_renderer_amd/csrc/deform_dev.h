// deform_dev.h -- device functions of GUAVA's Gaussian assembly (ubody_gaussian.py:252-278) shared by
// its forward kernels (deform.hip), its backward kernel (k_deform_gaussians_bwd, deform.hip) and the
// fused rasterizer backward of a posed avatar (k_preprocess_bwd_deformed, preprocess_bwd.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/gsr_deform.h"

namespace gsr {

// roma.rotmat_to_unitquat (scipy's from_matrix decision scheme), row-major m -> (x, y, z, w).
// The branch on the largest of (m00, m11, m22, trace) picks one of four candidate quaternions;
// the candidates share their off-diagonal sums, so all four are formed with 7 adds and the choice
// is made with selects (no dynamically indexed arrays, which compile to compare/select ladders).
__device__ __forceinline__ float4 rotmat_to_unitquat(const float m[9]) {
    const float d0 = m[0], d1 = m[4], d2 = m[8];
    const float d3 = (d0 + d1) + d2;
    int ch = 0;
    float best = d0;
    if (d1 > best) { best = d1; ch = 1; }
    if (d2 > best) { best = d2; ch = 2; }
    if (d3 > best) { best = d3; ch = 3; }
    const float t = 1.0f - d3;
    const float s01 = m[1] + m[3], s02 = m[2] + m[6], s12 = m[5] + m[7];  // m[3j+i] + m[3i+j]
    const float r0 = m[7] - m[5], r1 = m[2] - m[6], r2 = m[3] - m[1];     // the w candidates
    float4 q;
    q.x = ch == 0 ? t + 2.0f * m[0] : ch == 1 ? s01 : ch == 2 ? s02 : r0;
    q.y = ch == 0 ? s01 : ch == 1 ? t + 2.0f * m[4] : ch == 2 ? s12 : r1;
    q.z = ch == 0 ? s02 : ch == 1 ? s12 : ch == 2 ? t + 2.0f * m[8] : r2;
    q.w = ch == 0 ? r0 : ch == 1 ? r1 : ch == 2 ? r2 : 1.0f + d3;
    const float n = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    return make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
}

// roma.quat_product, xyzw: (p_w q_v + q_w p_v + p_v x q_v, p_w q_w - p_v . q_v)
__device__ __forceinline__ float4 quat_product(float4 p, float4 q) {
    float4 o;
    o.x = (p.w * q.x + q.w * p.x) + (p.y * q.z - p.z * q.y);
    o.y = (p.w * q.y + q.w * p.y) + (p.z * q.x - p.x * q.z);
    o.z = (p.w * q.z + q.w * p.z) + (p.x * q.y - p.y * q.x);
    o.w = p.w * q.w - ((p.x * q.x + p.y * q.y) + p.z * q.z);
    return o;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// compute_face_orientation (graphics_utils.py:61-80, safe_normalize eps 1e-20) of one deformed face
// and the frame's rotmat_to_unitquat (ubody_gaussian.py:257-258): fr = {m[9] (row-major, columns
// a0 a1 a2), s, q.xyzw}.
__device__ __forceinline__ void face_frame(const float* __restrict__ vb, int i0, int i1, int i2, float fr[14]) {
    const float v0x = vb[3 * i0], v0y = vb[3 * i0 + 1], v0z = vb[3 * i0 + 2];
    const float e1x = vb[3 * i1] - v0x, e1y = vb[3 * i1 + 1] - v0y, e1z = vb[3 * i1 + 2] - v0z;
    const float e2x = vb[3 * i2] - v0x, e2y = vb[3 * i2 + 1] - v0y, e2z = vb[3 * i2 + 2] - v0z;
    const float l1 = sqrtf(fmaxf(dot3(e1x, e1y, e1z, e1x, e1y, e1z), 1e-20f));
    const float a0x = e1x / l1, a0y = e1y / l1, a0z = e1z / l1;
    const float c1x = a0y * e2z - a0z * e2y, c1y = a0z * e2x - a0x * e2z, c1z = a0x * e2y - a0y * e2x;
    const float lc1 = sqrtf(fmaxf(dot3(c1x, c1y, c1z, c1x, c1y, c1z), 1e-20f));
    const float a1x = c1x / lc1, a1y = c1y / lc1, a1z = c1z / lc1;
    const float c2x = a1y * a0z - a1z * a0y, c2y = a1z * a0x - a1x * a0z, c2z = a1x * a0y - a1y * a0x;
    const float lc2 = sqrtf(fmaxf(dot3(c2x, c2y, c2z, c2x, c2y, c2z), 1e-20f));
    const float a2x = -(c2x / lc2), a2y = -(c2y / lc2), a2z = -(c2z / lc2);
    const float m[9] = {a0x, a1x, a2x, a0y, a1y, a2y, a0z, a1z, a2z};
    const float4 q = rotmat_to_unitquat(m);
#pragma unroll
    for (int k = 0; k < 9; k++) fr[k] = m[k];
    fr[9] = (l1 + fabsf(dot3(a2x, a2y, a2z, e2x, e2y, e2z))) / 2.0f;
    fr[10] = q.x; fr[11] = q.y; fr[12] = q.z; fr[13] = q.w;
}

#ifndef GSR_DEFORM_BWD_NOFRAME
#define GSR_DEFORM_BWD_NOFRAME 0  // timing ablation only (wrong gradients): the backward kernels take a
#endif                            // constant face frame: no vertex loads, no frame arithmetic

// the backward kernels' face frame: recomputed per thread (an upper bound on what sharing the frames
// through LDS, as the forward does, could save is the ablation above: DESIGN.md section 7)
__device__ __forceinline__ void face_frame_bwd(const float* __restrict__ vb, int i0, int i1, int i2, float fr[14]) {
    if (GSR_DEFORM_BWD_NOFRAME) {
#pragma unroll
        for (int k = 0; k < 14; k++) fr[k] = 0.25f * (float)(k + 1);
        return;
    }
    face_frame(vb, i0, i1, i2, fr);
}

// ---- backward of the assembly with respect to the canonical attributes.  The face frame and the
// vertex transform's quaternion are constants of this path (nothing differentiates through
// rotmat_to_unitquat, compute_face_orientation or the LBS).

// A UV Gaussian's binding resolved once, with the forward's range checks: the face id and its
// three vertex ids, or f = -1 for an out-of-range binding face or face-vertex index.
struct DeformBinding {
    int f, j0, j1, j2;
};
__device__ __forceinline__ DeformBinding resolve_binding(const int32_t* __restrict__ bind,
                                                         const int32_t* __restrict__ faces, int n, int V, int F) {
    DeformBinding r{-1, 0, 0, 0};
    const int bf = bind[n];
    if (bf >= 0 && bf < F) {
        const int a = faces[3 * bf], c = faces[3 * bf + 1], d = faces[3 * bf + 2];
        if (a >= 0 && a < V && c >= 0 && c < V && d >= 0 && d < V) { r.f = bf; r.j0 = a; r.j1 = c; r.j2 = d; }
    }
    return r;
}

// dL/dq of r = p (x) q (xyzw) given dL/dr: r is linear in q, r = L(p) q with L(p)^T = L(conj p).
__device__ __forceinline__ float4 quat_product_bwd_rhs(float4 p, float4 g) {
    return quat_product(make_float4(-p.x, -p.y, -p.z, p.w), g);
}

// Vertex Gaussian: out = r / max(||r||, 1e-12) with r = q(T_v) (x) q_v.  tv: the row-major 4x4
// vertex transform; qv, g and dq are wxyz (the attribute's and the rasterizer's order).
__device__ __forceinline__ void deform_bwd_vertex_rot(const float* __restrict__ tv16, const float qv[4],
                                                      const float g[4], float dq[4]) {
    const float4* tv = reinterpret_cast<const float4*>(tv16);
    const float4 r0 = tv[0], r1 = tv[1], r2 = tv[2];
    const float m[9] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z};
    const float4 p = rotmat_to_unitquat(m);
    const float4 r = quat_product(p, make_float4(qv[1], qv[2], qv[3], qv[0]));
    const float nn = fmaxf(sqrtf(((r.w * r.w + r.x * r.x) + r.y * r.y) + r.z * r.z), 1e-12f);
    const float ow = r.w / nn, ox = r.x / nn, oy = r.y / nn, oz = r.z / nn;
    const float og = ((ow * g[0] + ox * g[1]) + oy * g[2]) + oz * g[3];
    const float4 gr = make_float4((g[1] - ox * og) / nn, (g[2] - oy * og) / nn, (g[3] - oz * og) / nn,
                                  (g[0] - ow * og) / nn);
    const float4 d = quat_product_bwd_rhs(p, gr);
    dq[0] = d.w; dq[1] = d.x; dq[2] = d.y; dq[3] = d.z;
}

// UV Gaussian on the face frame fr (face_frame): xyz = (M local) s + centre, rotation = q_f (x) q_uv
// (not normalised), scale = scale_uv s.  g_rot and d_rot are wxyz.
__device__ __forceinline__ void deform_bwd_uv(const float fr[14], const float g_xyz[3], const float g_rot[4],
                                              const float g_scale[3], float d_local[3], float d_rot[4],
                                              float d_scale[3]) {
    const float s = fr[9];
    d_local[0] = s * dot3(fr[0], fr[3], fr[6], g_xyz[0], g_xyz[1], g_xyz[2]);
    d_local[1] = s * dot3(fr[1], fr[4], fr[7], g_xyz[0], g_xyz[1], g_xyz[2]);
    d_local[2] = s * dot3(fr[2], fr[5], fr[8], g_xyz[0], g_xyz[1], g_xyz[2]);
    const float4 d = quat_product_bwd_rhs(make_float4(fr[10], fr[11], fr[12], fr[13]),
                                          make_float4(g_rot[1], g_rot[2], g_rot[3], g_rot[0]));
    d_rot[0] = d.w; d_rot[1] = d.x; d_rot[2] = d.y; d_rot[3] = d.z;
#pragma unroll
    for (int c = 0; c < 3; c++) d_scale[c] = s * g_scale[c];
}

}  // namespace gsr
