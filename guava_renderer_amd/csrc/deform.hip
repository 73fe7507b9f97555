// deform.hip -- per-frame avatar deformation on gfx950: linear-blend skinning (SMPL-X body /
// FLAME head) and GUAVA's Gaussian assembly, B frames per launch set (include/gsr_deform.h).
//
// Reference (restated, not translated):
//   lbs / lbs_wobeta                models/modules/flame/lbs.py:142-229 / :255-333
//   blend_shapes, vertices2joints   lbs.py:355-376, :335-352
//   batch_rodrigues                 lbs.py:379-410
//   batch_rigid_transform           lbs.py:426-482
//   Ubody_Gaussian.forward          models/UbodyAvatar/ubody_gaussian.py:252-278
//   compute_face_orientation        utils/graphics_utils.py:52-80
//   roma 1.5.3 rotmat_to_unitquat / quat_product (third-party, scipy-derived; call sites
//   ubody_gaussian.py:253-254,258,270)
//
// Kernels (all B frames per launch):
//   k_pack_rows      segs x B WGs     the coefficient rows of EHM.forward from their pieces
//   k_lbs_rodrigues  B*J threads      axis-angle -> R, pose feature R - I
//   k_lbs_blend      3V/64 x B/16 WGs (B = 1: one frame, 16 waves per WG) v_shaped = template + shapedirs.betas, v_posed = v_shaped +
//                                     posedirs.feature: the bases are streamed once per 16 frames
//                                     (HBM-bound: 4*(NB + 9(J-1)) bytes per vertex coordinate)
//   k_lbs_blend_mfma 3V/32 x B/32 WGs the same for B > 16 on the matrix cores (f32 MFMA), bases
//                                     streamed once per 32 frames
//   k_lbs_coef_tiles                  B > 16 on tiled bases: the blend's coefficient rows (pose features,
//                                     betas) as 32-frame x 8-k tiles, in place of k_lbs_rodrigues
//   k_lbs_blend_tiledc                the matrix-core blend on tiled bases and tiled coefficients; one
//                                     blend or two independent ones per launch
//   k_lbs_joints     J/4 x B WGs      J_regressor . v_shaped (+ joints_offset)
//   k_lbs_chain      B WGs            the kinematic chain in LDS, one tree level per step
//   k_lbs_skin       V x B            T_v = sum_j w_vj A_j, v = T_v [v_posed; 1]
//   k_deform_gaussians (V+N) x B/8    vertex + UV Gaussians straight into the rasterizer's inputs
//                                     (face frames once per face and frame, in LDS)
//   k_deform_gaussians_bwd (V+N) x 1  gradients of the canonical attributes (shared ones: frame sums in
//                                     frame order in one thread; per-frame only: (V+N) x B/8); no LDS
// Every sum runs in a fixed order (fmaf chains over k in index order, 3-term dots left to right),
// so results are deterministic run to run.
#include <climits>
#include <cstdlib>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_deform.h"
#include "deform_dev.h"
#include "deform_internal.h"
#include "gsr_internal.h"
#include "preprocess_dev.h"

namespace gsr {

#ifndef GSR_DEFORM_NOSTORE
#define GSR_DEFORM_NOSTORE 0  // timing ablation only: skip the UV rotation and the means/scales stores
#endif

constexpr int kLbsFrames = 16;  // frames per k_lbs_blend workgroup (accumulators per thread)
constexpr int kLbsSplit = 4;    // k_lbs_blend waves per workgroup, each an interleaved slice of k
// single-frame batches (the per-frame drop-in path): one accumulator per thread and 16 waves per
// workgroup, so the K-long stream of every coordinate has 16 slices of loads in flight
constexpr int kLbsSplit1 = 16;

struct Parents {
    int8_t p[GSR_LBS_MAX_JOINTS];
};

// batch_rodrigues (lbs.py:379-410): angle = |r + 1e-8|, dir = r / angle,
// R = I + sin K + (1 - cos) K.K with K the cross-product matrix of dir.
// batch_rodrigues (lbs.py:379-410) of pose entry t (axis-angle, or a rotation matrix when !pose2rot)
__device__ __forceinline__ void rodrigues_one(const float* __restrict__ pose, int t, int pose2rot, float (&R)[9]) {
    if (pose2rot) {
        const float rx = pose[3 * t], ry = pose[3 * t + 1], rz = pose[3 * t + 2];
        const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
        const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
        const float x = rx / angle, y = ry / angle, z = rz / angle;
        const float c = cosf(angle), s = sinf(angle);
        const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
        const float omc = 1.0f - c;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const float kk = K[3 * r] * K[q] + K[3 * r + 1] * K[3 + q] + K[3 * r + 2] * K[6 + q];
                R[3 * r + q] = ((r == q ? 1.0f : 0.0f) + s * K[3 * r + q]) + omc * kk;
            }
    } else {
#pragma unroll
        for (int e = 0; e < 9; e++) R[e] = pose[9 * t + e];
    }
}

__global__ void k_lbs_rodrigues(int B, int J, const float* __restrict__ pose, int pose2rot,
                                float* __restrict__ rot, float* __restrict__ feat) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * J) return;
    const int b = t / J, j = t - b * J;
    float R[9];
    rodrigues_one(pose, t, pose2rot, R);
#pragma unroll
    for (int e = 0; e < 9; e++) rot[9 * t + e] = R[e];
    if (j > 0) {  // pose_feature = (rot_mats[:, 1:] - I).view(B, -1)   (lbs.py:303)
        float* f = feat + (int64_t)b * (J - 1) * 9 + (j - 1) * 9;
#pragma unroll
        for (int e = 0; e < 9; e++) f[e] = R[e] - ((e % 4) == 0 ? 1.0f : 0.0f);
    }
}

// acc[f] += sum over this wave's k-slice (k = w mod kLbsSplit, ascending) of coef[k][f] * base[k][m],
// kLbsBatch loads of the k-major base issued before their FMAs (enough bytes in flight to stream
// from HBM with ~4 waves per SIMD).
constexpr int kLbsBatch = 16;
template <int NF, int SPLIT>
__device__ __forceinline__ void lbs_stream(const float* __restrict__ base, int M, int m, int K, int w,
                                           const float* coef, float (&acc)[NF]) {
    for (int k0 = w; k0 < K; k0 += SPLIT * kLbsBatch) {
        float v[kLbsBatch];
#pragma unroll
        for (int u = 0; u < kLbsBatch; u++) {
            const int k = k0 + u * SPLIT;
            v[u] = k < K ? base[(int64_t)k * M + m] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kLbsBatch; u++) {
            const int k = k0 + u * SPLIT;
            if (k >= K) break;
            if constexpr (NF % 4 == 0) {
                const float4* c = reinterpret_cast<const float4*>(&coef[k * NF]);
#pragma unroll
                for (int q = 0; q < NF / 4; q++) {
                    const float4 cq = c[q];
                    acc[4 * q] = fmaf(cq.x, v[u], acc[4 * q]); acc[4 * q + 1] = fmaf(cq.y, v[u], acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(cq.z, v[u], acc[4 * q + 2]); acc[4 * q + 3] = fmaf(cq.w, v[u], acc[4 * q + 3]);
                }
            } else {
#pragma unroll
                for (int f = 0; f < NF; f++) acc[f] = fmaf(coef[k * NF + f], v[u], acc[f]);
            }
        }
    }
}

// v_shaped = v_template + blend_shapes(betas, shapedirs); v_posed = pose_offsets + v_shaped
// (lbs.py:186,201,210 / :305,314): a [3V x K] x [K x B] product streamed from HBM.  A workgroup
// owns 64 vertex coordinates (lane = coordinate) of kLbsFrames frames; its kLbsSplit waves take
// interleaved slices of k (k = w mod kLbsSplit), so each coordinate's K-long stream has 4 waves of
// loads in flight instead of one serial chain, and the slice sums are added in slice order through
// LDS (deterministic).  The frame coefficients sit in LDS (broadcast reads); the k-major bases are
// read coalesced, once per frame group.
inline dim3 lbs_blend_grid(int M, int B, int nf) {
    const int nx8 = ((M + 63) / 64 + 7) / 8 * 8;
    return dim3(nx8 * ((B + nf - 1) / nf));
}

template <int NF, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void k_lbs_blend(int B, int M, int NB, int NP,
                                                              const float* __restrict__ vt, int64_t vt_stride,
                                                              const float* __restrict__ betas,
                                                              const float* __restrict__ sd_t,
                                                              const float* __restrict__ feat,
                                                              const float* __restrict__ pd,
                                                              float* __restrict__ v_shaped,
                                                              float* __restrict__ v_posed) {
    extern __shared__ float4 lds4[];  // coef [(NB + NP)][NF], then the slice reduction
    float* coef = reinterpret_cast<float*>(lds4);
    // XCD-aware order (1-D grid, lbs_blend_grid): the frame groups of one coordinate block are
    // dealt to the same XCD back to back, so all but the first read the basis slice from its L2
    const int ng = (B + NF - 1) / NF;
    const int jx = (int)(blockIdx.x >> 3);
    const int by = jx % ng;
    const int bx = (jx / ng) * 8 + (int)(blockIdx.x & 7);
    if (bx * 64 >= M) return;  // padding block (the whole workgroup, before any barrier)
    const int b0 = by * NF;
    const int nk = NB + NP;
    for (int idx = threadIdx.x; idx < nk * NF; idx += blockDim.x) {
        const int k = idx / NF, f = idx - k * NF;
        const int b = b0 + f;
        float v = 0.f;
        if (b < B) v = k < NB ? betas[(int64_t)b * NB + k] : feat[(int64_t)b * NP + (k - NB)];
        coef[idx] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = bx * 64 + lane;
    const bool ok = m < M;
    const int nf = min(NF, B - b0);
    float as[NF], ap[NF];
#pragma unroll
    for (int f = 0; f < NF; f++) { as[f] = 0.f; ap[f] = 0.f; }
    if (ok) {
        lbs_stream<NF, SPLIT>(sd_t, M, m, NB, w, coef, as);
        lbs_stream<NF, SPLIT>(pd, M, m, NP, w, coef + NB * NF, ap);
    }
    // slice reduction through LDS: red[w][f][lane]
    float* red = coef;
    __syncthreads();  // coefficients no longer needed
#pragma unroll
    for (int f = 0; f < NF; f++) red[(w * NF + f) * 64 + lane] = as[f];
    __syncthreads();
    float vs[NF];
#pragma unroll
    for (int f = 0; f < NF; f++) vs[f] = 0.f;
    if (w == 0) {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            float acc = red[f * 64 + lane];
            for (int u = 1; u < SPLIT; u++) acc += red[(u * NF + f) * 64 + lane];
            const int b = b0 + f;
            if (ok && f < nf) {
                const float tv = vt[(int64_t)b * vt_stride + m];
                vs[f] = NB > 0 ? tv + acc : tv;
                v_shaped[(int64_t)b * M + m] = vs[f];
            }
        }
    }
    if (!v_posed) return;  // blend_shapes + joints only (gsr_blend_joints); uniform
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; f++) red[(w * NF + f) * 64 + lane] = ap[f];
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int f = 0; f < NF; f++) {
            float acc = red[f * 64 + lane];
            for (int u = 1; u < SPLIT; u++) acc += red[(u * NF + f) * 64 + lane];
            if (ok && f < nf) v_posed[(int64_t)(b0 + f) * M + m] = acc + vs[f];
        }
    }
}

// The same products for batches of more than kLbsFrames frames, on the matrix cores, with the
// bases read ONCE per 32 frames: D[b][m] = sum_k coef[b][k] base[k][m] is a (32 frames x 32
// coordinates) tile per workgroup, v_mfma_f32_32x32x2_f32 (exact f32 products) with A = the
// frames' coefficients (row b, k) and B = the k-major bases (column m, coalesced 128-byte
// half-wave loads).  The 4 waves take interleaved k-steps and their partial tiles are added in
// wave order through LDS (deterministic); each wave then finishes 4 of the 16 output registers:
// v_shaped = template + shape sum, v_posed = v_shaped + pose sum (the VALU kernel's association).
// (Measured variants: 8 waves x 16 loads in flight, and the coefficient block staged transposed
// in LDS, were both slower at B = 32.)
typedef float floatx16 __attribute__((ext_vector_type(16)));
constexpr int kBlendUnroll = 8;  // k-steps whose loads are issued before their MFMAs

__device__ __forceinline__ void blend_mfma_part(floatx16& acc, const float* __restrict__ coef, int ncoef,
                                                const float* __restrict__ base, int M, int K, int bA, bool bok,
                                                int m, bool mok, int w, int hi) {
    const int nsteps = (K + 1) / 2;
    for (int s0 = w; s0 < nsteps; s0 += 4 * kBlendUnroll) {
        float a[kBlendUnroll], bb[kBlendUnroll];
#pragma unroll
        for (int u = 0; u < kBlendUnroll; u++) {
            const int k = 2 * (s0 + 4 * u) + hi;
            const bool kok = s0 + 4 * u < nsteps && k < K;
            a[u] = (bok && kok) ? coef[(int64_t)bA * ncoef + k] : 0.f;
            bb[u] = (mok && kok) ? base[(int64_t)k * M + m] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kBlendUnroll; u++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bb[u], acc, 0, 0, 0);
    }
}

__global__ __launch_bounds__(256) void k_lbs_blend_mfma(int B, int M, int NB, int NP,
                                                        const float* __restrict__ vt, int64_t vt_stride,
                                                        const float* __restrict__ betas,
                                                        const float* __restrict__ sd_t,
                                                        const float* __restrict__ feat,
                                                        const float* __restrict__ pd,
                                                        float* __restrict__ v_shaped,
                                                        float* __restrict__ v_posed) {
    __shared__ float red[4][2][16][64];  // per-wave partial tiles: [wave][shape/pose][register][lane]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5, l32 = lane & 31;
    const int m0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int m = m0 + l32, bA = b0 + l32;
    const bool mok = m < M, bok = bA < B;
    floatx16 as, ap;
#pragma unroll
    for (int r = 0; r < 16; r++) { as[r] = 0.f; ap[r] = 0.f; }
    if (NB > 0) blend_mfma_part(as, betas, NB, sd_t, M, NB, bA, bok, m, mok, w, hi);
    if (NP > 0 && v_posed) blend_mfma_part(ap, feat, NP, pd, M, NP, bA, bok, m, mok, w, hi);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        red[w][0][r][lane] = as[r];
        red[w][1][r][lane] = ap[r];
    }
    __syncthreads();
    // wave w finishes registers 4w..4w+3: row (frame) (r&3) + 8(r>>2) + 4(lane>>5), column m
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = 4 * w + i;
        const int b = b0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (!mok || b >= B) continue;
        float S = red[0][0][r][lane], Pz = red[0][1][r][lane];
#pragma unroll
        for (int u = 1; u < 4; u++) { S += red[u][0][r][lane]; Pz += red[u][1][r][lane]; }
        const float tv = vt[(int64_t)b * vt_stride + m];
        const float vs = NB > 0 ? tv + S : tv;
        v_shaped[(int64_t)b * M + m] = vs;
        if (v_posed) v_posed[(int64_t)b * M + m] = Pz + vs;
    }
}

// ---- tiled bases (GsrLbsSparse.shapedirs_tiled / posedirs_tiled, include/gsr_deform.h)
// A base [K][M] re-laid once per avatar as 1-KB tiles of 32 coordinates x 8 k: tile (t, g) holds, as
// float4 (t * nkg + g) * 64 + 32 h + c, component j, the value base[8g + 4h + j][32t + c] (K padded to
// a multiple of 8, M to 32, with zeros).  Every load is then one fully coalesced 16-byte-per-lane
// wave read (1 KB), where the k-major layout gives 4-byte lanes (256 B per load instruction): the
// blend's bases stream at HBM rate with a quarter of the load instructions in flight.
constexpr int kTiledUnroll = 4;  // tile groups whose loads are issued before their products
#ifndef GSR_BLEND_COEF_VEC
#define GSR_BLEND_COEF_VEC 1
#endif

// D[frame][m] over the k of one base: v_mfma_f32_32x32x2_f32 with lane (c, h) holding base[8g + 4h + j]
// [32t + c] (B operand) and coef[frame b0 + c][8g + 4h + j] (A operand) for the j-th MFMA of a group
// (the lane halves' k of one MFMA are 8g + j and 8g + 4 + j); wave w takes the groups g = w mod 4.
// The coefficient gathers (lane = frame row, 4 consecutive k) are 16- or 8-byte loads when the rows'
// stride and base allow (vw = 4 / 2, wave-uniform): 16 scattered dword loads per step were the
// texture path's load (TA 48% / TD 58% busy at 37% of HBM), four times the base tile's loads.
__device__ __forceinline__ int coef_vec_width(const float* coef, int ncoef) {
    if (((uintptr_t)coef & 15) == 0 && (ncoef & 3) == 0) return 4;
    if (((uintptr_t)coef & 7) == 0 && (ncoef & 1) == 0) return 2;
    return 1;
}

__device__ __forceinline__ void blend_tiled_mfma_part(floatx16& acc, const float* __restrict__ coef, int ncoef,
                                                      const float4* __restrict__ tb, int K, int t, int bA,
                                                      bool bok, int w, int hi, int lane, int nw = 4) {
    const int nkg = (K + 7) / 8;
    const int nfull = GSR_BLEND_COEF_VEC ? K / 8 : 0;  // groups whose 8 k are all < K
    const int vw = coef_vec_width(coef, ncoef);
    const float4* __restrict__ p = tb + (int64_t)t * nkg * 64 + lane;
    const float* __restrict__ cr = coef + (int64_t)bA * ncoef;
    for (int g0 = w; g0 < nkg; g0 += nw * kTiledUnroll) {
        float4 v[kTiledUnroll];
        float a[kTiledUnroll][4];
#pragma unroll
        for (int u = 0; u < kTiledUnroll; u++) {
            const int g = g0 + nw * u;
            v[u] = g < nkg ? p[(int64_t)g * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
            const int k0 = 8 * g + 4 * hi;
            if (g < nfull && vw == 4) {
                const float4 c = bok ? *reinterpret_cast<const float4*>(cr + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
                a[u][0] = c.x; a[u][1] = c.y; a[u][2] = c.z; a[u][3] = c.w;
            } else if (g < nfull && vw == 2) {
                const float2 c0 = bok ? *reinterpret_cast<const float2*>(cr + k0) : make_float2(0.f, 0.f);
                const float2 c1 = bok ? *reinterpret_cast<const float2*>(cr + k0 + 2) : make_float2(0.f, 0.f);
                a[u][0] = c0.x; a[u][1] = c0.y; a[u][2] = c1.x; a[u][3] = c1.y;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = k0 + j;
                    a[u][j] = (bok && k < K) ? cr[k] : 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kTiledUnroll; u++) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], v[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][1], v[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][2], v[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][3], v[u].w, acc, 0, 0, 0);
        }
    }
}

// k_lbs_blend_mfma over the tiled bases: one workgroup per 32 coordinates x 32 frames, the same
// wave-order reduction and epilogue.  NW waves split the k groups (g = w mod NW): 8 when the model
// has at most 512 coordinate tiles (blend_ksplit; the FLAME head, 471: 4 waves per workgroup left the SIMDs under two
// waves each, every wave a long serial load -> MFMA chain), else 4.
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_lbs_blend_tiled(int B, int M, int NB, int NP,
                                                         const float* __restrict__ vt, int64_t vt_stride,
                                                         const float* __restrict__ betas,
                                                         const float4* __restrict__ sd_tiled,
                                                         const float* __restrict__ feat,
                                                         const float4* __restrict__ pd_tiled,
                                                         float* __restrict__ v_shaped,
                                                         float* __restrict__ v_posed) {
    __shared__ float red[NW][2][16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5, l32 = lane & 31;
    const int t = blockIdx.x, m0 = t * 32, b0 = blockIdx.y * 32;
    const int m = m0 + l32, bA = b0 + l32;
    const bool mok = m < M, bok = bA < B;
    floatx16 as, ap;
#pragma unroll
    for (int r = 0; r < 16; r++) { as[r] = 0.f; ap[r] = 0.f; }
    if (NB > 0) blend_tiled_mfma_part(as, betas, NB, sd_tiled, NB, t, bA, bok, w, hi, lane, NW);
    if (NP > 0 && v_posed) blend_tiled_mfma_part(ap, feat, NP, pd_tiled, NP, t, bA, bok, w, hi, lane, NW);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        red[w][0][r][lane] = as[r];
        red[w][1][r][lane] = ap[r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16 / NW; i++) {
        const int r = (16 / NW) * w + i;
        const int b = b0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (!mok || b >= B) continue;
        float S = red[0][0][r][lane], Pz = red[0][1][r][lane];
#pragma unroll
        for (int u = 1; u < NW; u++) { S += red[u][0][r][lane]; Pz += red[u][1][r][lane]; }
        const float tv = vt[(int64_t)b * vt_stride + m];
        const float vs = NB > 0 ? tv + S : tv;
        v_shaped[(int64_t)b * M + m] = vs;
        if (v_posed) v_posed[(int64_t)b * M + m] = Pz + vs;
    }
}

// ---- tiled coefficients (the A operand in the base tiles' layout)
// The B coefficient rows [B][K] of a blend as 1-KB tiles of 32 frames x 8 k: as float4
// (bt * nkg + g) * 64 + 32 h + c, component j, the value coef[32 bt + c][8g + 4h + j], zero where the
// frame is >= B or k >= K.  A wave's coefficient load is then one contiguous 1-KB read, like its base
// tile: the row-major gather of blend_tiled_mfma_part touches 64 cache lines (rows >= 1,400 bytes
// apart) for the same 1 KB, once per k-group and workgroup.  k_lbs_coef_tiles writes every word of
// the tiles on every call (the workspace is reused; the blend reads the padding).
__device__ __forceinline__ int64_t coef_tile_index(int nkg, int b, int k) {
    return ((((int64_t)(b >> 5) * nkg + (k >> 3)) * 64 + 32 * ((k >> 2) & 1) + (b & 31)) << 2) + (k & 3);
}

// One model's coefficient tiles: threads [0, n_pose) take (frame of the padded 32-frame tiles, joint):
// k_lbs_rodrigues' rotation (the same expressions) and pose feature R - I into feat_tiles, zeros for
// the padding frames and the k tail; threads [n_pose, n_pose + n_beta) take one float4 of beta_tiles
// from the row-major betas.
struct CoefJob {
    int B, J, NB, pose2rot;
    int n_pose, n_beta;
    const float* pose;   // null: no pose part (n_pose = 0)
    const float* betas;  // null: no betas part (n_beta = 0)
    float* feat_tiles;
    float4* beta_tiles;
};

__device__ __forceinline__ void coef_tiles_one(const CoefJob& c, int idx) {
    if (idx < c.n_pose) {
        const int J = c.J, NP = 9 * (J - 1), nkg = (NP + 7) / 8;
        const int b = idx / J, j = idx - b * J;
        float R[9];
        if (b < c.B) {
            rodrigues_one(c.pose, idx, c.pose2rot, R);
#pragma unroll
            for (int e = 0; e < 9; e++) R[e] = R[e] - ((e % 4) == 0 ? 1.0f : 0.0f);
        } else {
#pragma unroll
            for (int e = 0; e < 9; e++) R[e] = 0.f;
        }
        if (j > 0) {
#pragma unroll
            for (int e = 0; e < 9; e++) c.feat_tiles[coef_tile_index(nkg, b, 9 * (j - 1) + e)] = R[e];
            if (j == J - 1)
                for (int k = NP; k < 8 * nkg; k++) c.feat_tiles[coef_tile_index(nkg, b, k)] = 0.f;
        }
        return;
    }
    idx -= c.n_pose;
    if (idx >= c.n_beta) return;
    const int NB = c.NB, nkg = (NB + 7) / 8;
    const int lane = idx & 63, tg = idx >> 6;
    const int g = tg % nkg, bt = tg / nkg;
    const int b = 32 * bt + (lane & 31), k0 = 8 * g + 4 * (lane >> 5);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = (b < c.B && k0 + j < NB) ? c.betas[(int64_t)b * NB + k0 + j] : 0.f;
    c.beta_tiles[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// the coefficient tiles of one model, or of two independent ones in one launch (EHM's FLAME head and
// body: both depend only on the packed rows)
__global__ __launch_bounds__(256) void k_lbs_coef_tiles(CoefJob a, CoefJob b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int na = a.n_pose + a.n_beta;
    if (i < na) coef_tiles_one(a, i);
    else if (i - na < b.n_pose + b.n_beta) coef_tiles_one(b, i - na);
}

// blend_tiled_mfma_part with the coefficients read from their tiles: the same a and v operands in
// the same order, so the same sums bit for bit; no per-lane frame / k selects in the loop.
// One k group per round on two register sets: a round's two loads are issued before the round
// before it multiplies.  More loads in flight per wave ran slower.
__device__ __forceinline__ void blend_tiledc_mfma_part(floatx16& acc, const float4* __restrict__ ct,
                                                       const float4* __restrict__ tb, int K, int t, int bt, int w,
                                                       int lane, int nw) {
    const int nkg = (K + 7) / 8;
    const float4* __restrict__ p = tb + (int64_t)t * nkg * 64 + lane;
    const float4* __restrict__ c = ct + (int64_t)bt * nkg * 64 + lane;
    auto mma = [&](const float4& v, const float4& a) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, v.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, v.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, v.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, v.w, acc, 0, 0, 0);
    };
    if (w >= nkg) return;
    float4 v0 = p[(int64_t)w * 64], a0 = c[(int64_t)w * 64], v1, a1;
    for (int g = w; g < nkg; g += 2 * nw) {
        const bool more = g + nw < nkg;
        if (more) { v1 = p[(int64_t)(g + nw) * 64]; a1 = c[(int64_t)(g + nw) * 64]; }
        mma(v0, a0);
        if (more) {
            if (g + 2 * nw < nkg) { v0 = p[(int64_t)(g + 2 * nw) * 64]; a0 = c[(int64_t)(g + 2 * nw) * 64]; }
            mma(v1, a1);
        }
    }
}

// One batched blend over tiled bases and tiled coefficients (k_lbs_blend_tiled's arguments)
struct BlendTJob {
    int M, NB, NP;
    const float* vt;
    int64_t vt_stride;
    const float4* beta_tiles;
    const float4* sd_tiled;
    const float4* feat_tiles;
    const float4* pd_tiled;
    float* v_shaped;
    float* v_posed;
};

// k_lbs_blend_tiled<KS>'s arithmetic on tiled coefficients, in a workgroup of WAVES >= KS waves: each
// group of KS waves owns one coordinate tile (tile = WAVES / KS * tw + group) of frame tile bt, splits
// the k groups KS ways and reduces in its own wave order -- the sums of k_lbs_blend_tiled<KS>, bit
// for bit, whatever the workgroup size.
template <int WAVES, int KS>
__device__ __forceinline__ void blend_tiledc_block(const BlendTJob& j, int B, int tw, int bt,
                                                   float (*red)[2][16][64]) {
    const int lane = threadIdx.x & 63, w8 = threadIdx.x >> 6, hi = lane >> 5, l32 = lane & 31;
    const int sg = w8 / KS, w = w8 % KS;
    const int M = j.M, NB = j.NB;
    const int t = tw * (WAVES / KS) + sg;
    const bool tok = t < (M + 31) / 32;  // (an odd tile count leaves the last workgroup's second group idle)
    const int m = t * 32 + l32, b0 = bt * 32;
    const bool mok = tok && m < M;
    floatx16 as, ap;
#pragma unroll
    for (int r = 0; r < 16; r++) { as[r] = 0.f; ap[r] = 0.f; }
    if (tok && NB > 0) blend_tiledc_mfma_part(as, j.beta_tiles, j.sd_tiled, NB, t, bt, w, lane, KS);
    if (tok && j.NP > 0 && j.v_posed)
        blend_tiledc_mfma_part(ap, j.feat_tiles, j.pd_tiled, j.NP, t, bt, w, lane, KS);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        red[w8][0][r][lane] = as[r];
        red[w8][1][r][lane] = ap[r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16 / KS; i++) {
        const int r = (16 / KS) * w + i;
        const int b = b0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (!mok || b >= B) continue;
        float S = red[sg * KS][0][r][lane], Pz = red[sg * KS][1][r][lane];
#pragma unroll
        for (int u = 1; u < KS; u++) { S += red[sg * KS + u][0][r][lane]; Pz += red[sg * KS + u][1][r][lane]; }
        const float tv = j.vt[(int64_t)b * j.vt_stride + m];
        const float vs = NB > 0 ? tv + S : tv;
        j.v_shaped[(int64_t)b * M + m] = vs;
        if (j.v_posed) j.v_posed[(int64_t)b * M + m] = Pz + vs;
    }
}

// One blend (na = grid.x), or two independent ones in one launch (EHM's FLAME head blend beside the
// body's shape blend, the batched k_lbs_blend_tiled1_pair): workgroups [0, na) take job a with a
// KSA-way k split, the rest job b with KSB; blockIdx.y is the 32-frame tile.  Neither job reads what
// the other writes.
template <int WAVES, int KSA, int KSB>
__global__ __launch_bounds__(64 * WAVES) void k_lbs_blend_tiledc(int B, BlendTJob a, int na, BlendTJob b) {
    __shared__ float red[WAVES][2][16][64];
    if ((int)blockIdx.x < na) blend_tiledc_block<WAVES, KSA>(a, B, blockIdx.x, blockIdx.y, red);
    else blend_tiledc_block<WAVES, KSB>(b, B, blockIdx.x - na, blockIdx.y, red);
}

// One frame over the tiled bases (the per-frame drop-in path): lane (c, h) of wave w sums
// coef[8g + 4h + j] base[8g + 4h + j][32t + c] over its groups g = w mod 4 (four fmaf per 16-byte
// load), then the two lane halves and the four waves are added in a fixed order through LDS.
__device__ __forceinline__ float blend_tiled_one(const float* __restrict__ coef, const float4* __restrict__ tb,
                                                 int K, int t, int w, int hi, int lane) {
    const int nkg = (K + 7) / 8;
    const float4* __restrict__ p = tb + (int64_t)t * nkg * 64 + lane;
    float acc = 0.f;
    for (int g0 = w; g0 < nkg; g0 += 4 * kTiledUnroll) {
        float4 v[kTiledUnroll];
        float a[kTiledUnroll][4];
#pragma unroll
        for (int u = 0; u < kTiledUnroll; u++) {
            const int g = g0 + 4 * u;
            v[u] = g < nkg ? p[(int64_t)g * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int k = 8 * g + 4 * hi + j;
                a[u][j] = k < K ? coef[k] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < kTiledUnroll; u++) {
            acc = fmaf(a[u][0], v[u].x, acc);
            acc = fmaf(a[u][1], v[u].y, acc);
            acc = fmaf(a[u][2], v[u].z, acc);
            acc = fmaf(a[u][3], v[u].w, acc);
        }
    }
    return acc;
}

// pose (single-frame LBS, gsr_lbs_sp): the pose features are formed here from the frame's pose
// (rodrigues_one, the same expressions as k_lbs_rodrigues) instead of read from a launch before
__device__ __forceinline__ void blend_tiled1_block(const Blend1Job& j, int t) {
    __shared__ float red[2][4][64];
    __shared__ float sfeat[9 * (GSR_LBS_MAX_JOINTS - 1)];
    const int M = j.M, NB = j.NB, NP = j.NP;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5, l32 = lane & 31;
    const int m = t * 32 + l32;
    const float* feat = j.feat;
    if (j.pose && NP > 0 && j.v_posed) {
        const int jn = NP / 9;  // J - 1 posed joints (pose_feature skips the root)
        if ((int)threadIdx.x < jn) {
            float R[9];
            rodrigues_one(j.pose, (int)threadIdx.x + 1, j.pose2rot, R);
#pragma unroll
            for (int e = 0; e < 9; e++) sfeat[9 * threadIdx.x + e] = R[e] - ((e % 4) == 0 ? 1.0f : 0.0f);
        }
        __syncthreads();
        feat = sfeat;
    }
    red[0][w][lane] = NB > 0 ? blend_tiled_one(j.betas, j.sd_tiled, NB, t, w, hi, lane) : 0.f;
    red[1][w][lane] = (NP > 0 && j.v_posed) ? blend_tiled_one(feat, j.pd_tiled, NP, t, w, hi, lane) : 0.f;
    __syncthreads();
    if (w == 0 && hi == 0 && m < M) {
        float S = 0.f, Pz = 0.f;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            S += red[0][u][l32] + red[0][u][l32 + 32];
            Pz += red[1][u][l32] + red[1][u][l32 + 32];
        }
        const float vs = NB > 0 ? j.vt[m] + S : j.vt[m];
        j.v_shaped[m] = vs;
        if (j.v_posed) j.v_posed[m] = Pz + vs;
    }
}

__global__ __launch_bounds__(256) void k_lbs_blend_tiled1(Blend1Job j) { blend_tiled1_block(j, blockIdx.x); }

// Two independent single-frame blends in one launch (EHM's FLAME head blend beside the body's shape
// blend, gsr_ehm_forward at B = 1): workgroups [0, na) take job a, the rest job b.  One launch fewer
// on the serial per-frame path, and the two partial grids share the chip instead of running in turn.
__global__ __launch_bounds__(256) void k_lbs_blend_tiled1_pair(Blend1Job a, int na, Blend1Job b) {
    if ((int)blockIdx.x < na) blend_tiled1_block(a, blockIdx.x);
    else blend_tiled1_block(b, blockIdx.x - na);
}

// blend launcher: the matrix-core kernel for more than kLbsFrames frames, the streaming one otherwise
// (tiled bases, when the caller prepared them: B > kLbsFrames and B = 1)
static void launch_blend(int B, int M, int NB, int NP, const float* vt, int64_t vt_stride, const float* betas,
                         const float* sd_t, const float* feat, const float* pd, float* vs, float* vp,
                         hipStream_t s, const GsrLbsSparse* sp = nullptr, const float* pose = nullptr,
                         int pose2rot = 1);

// the single-frame tiled blend forms the pose features itself (k_lbs_blend_tiled1's pose argument)
static bool blend_takes_pose(int B, int NB, int NP, const float* vp, const GsrLbsSparse* sp) {
    static const bool tiled_on = tune_env("GSR_BLEND_TILED", 1) != 0;
    return B == 1 && tiled_on && sp && (NB == 0 || sp->shapedirs_tiled) && (NP == 0 || !vp || sp->posedirs_tiled) &&
           (NB > 0 || (NP > 0 && vp)) && NP <= 9 * (GSR_LBS_MAX_JOINTS - 1);
}

static size_t lbs_blend_lds(int NB, int NP, int nf, int split) {
    const size_t coef = sizeof(float) * (size_t)(NB + NP) * nf;
    const size_t red = sizeof(float) * (size_t)split * nf * 64;
    return coef > red ? coef : red;
}

static void lbs_blend_attr(size_t lds) {
    static size_t attr = 0;
    if (lds > 65536 && attr < lds) {
        attr = lds;
        hipFuncSetAttribute((const void*)k_lbs_blend<kLbsFrames, kLbsSplit>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipFuncSetAttribute((const void*)k_lbs_blend<1, kLbsSplit1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    }
}

Blend1Job blend1_job(int M, int NB, int NP, const float* vt, const float* betas, const float* feat, float* vs,
                     float* vp, const GsrLbsSparse* sp, const float* pose, int pose2rot) {
    return Blend1Job{M, NB, vp ? NP : 0, pose2rot, vt, betas, reinterpret_cast<const float4*>(sp->shapedirs_tiled),
                     feat, reinterpret_cast<const float4*>(sp->posedirs_tiled), vs, vp, pose};
}

// whether launch_blend takes the single-frame tiled kernel (k_lbs_blend_tiled1) for these arguments
bool blend_tiled1_applies(int B, int NB, int NP, const float* vp, const GsrLbsSparse* sp) {
    static const bool tiled_on = tune_env("GSR_BLEND_TILED", 1) != 0;
    return B == 1 && tiled_on && sp && (NB == 0 || sp->shapedirs_tiled) && (NP == 0 || !vp || sp->posedirs_tiled) &&
           (NB > 0 || (NP > 0 && vp));
}

// the k split of a matrix-core blend over M coordinates on tiled bases: 8 waves per tile for at most
// 512 coordinate tiles (the FLAME head, 471), else 4 -- by the model alone, on every path, so a
// frame's sums depend neither on the batch it came in nor on the entry point (the choice was by the
// whole grid before: the same split up to 32 frames)
static int blend_ksplit(int M) {
    static const int nw_env = tune_env("GSR_BLEND_NW", 0);
    return nw_env == 4 || nw_env == 8 ? nw_env : ((M + 31) / 32 <= 512 ? 8 : 4);
}

static void launch_blend(int B, int M, int NB, int NP, const float* vt, int64_t vt_stride, const float* betas,
                         const float* sd_t, const float* feat, const float* pd, float* vs, float* vp,
                         hipStream_t s, const GsrLbsSparse* sp, const float* pose, int pose2rot) {
    static const bool valu_only = tune_env("GSR_BLEND_VALU", 0) == 1;  // timing A/B only
    // GSR_BLEND_TILED=0: the k-major kernels even with tiled bases (A/B)
    static const bool tiled_on = tune_env("GSR_BLEND_TILED", 1) != 0;
    const bool tiled = tiled_on && sp && (NB == 0 || sp->shapedirs_tiled) &&
                       (NP == 0 || !vp || sp->posedirs_tiled) && (NB > 0 || (NP > 0 && vp));
    if (tiled && B > kLbsFrames && !valu_only) {
        const dim3 grid((M + 31) / 32, (B + 31) / 32);
        const int nw = blend_ksplit(M);
        const float4* sdt = reinterpret_cast<const float4*>(sp->shapedirs_tiled);
        const float4* pdt = reinterpret_cast<const float4*>(sp->posedirs_tiled);
        if (nw == 8)
            hipLaunchKernelGGL(k_lbs_blend_tiled<8>, grid, dim3(512), 0, s, B, M, NB, vp ? NP : 0, vt, vt_stride,
                               betas, sdt, feat, pdt, vs, vp);
        else
            hipLaunchKernelGGL(k_lbs_blend_tiled<4>, grid, dim3(256), 0, s, B, M, NB, vp ? NP : 0, vt, vt_stride,
                               betas, sdt, feat, pdt, vs, vp);
        return;
    }
    if (tiled && B == 1) {
        const Blend1Job j = blend1_job(M, NB, NP, vt, betas, feat, vs, vp, sp, pose, pose2rot);
        hipLaunchKernelGGL(k_lbs_blend_tiled1, dim3((M + 31) / 32), dim3(256), 0, s, j);
        return;
    }
    if (B > kLbsFrames && !valu_only) {
        hipLaunchKernelGGL(k_lbs_blend_mfma, dim3((M + 31) / 32, (B + 31) / 32), dim3(256), 0, s, B, M, NB,
                           vp ? NP : 0, vt, vt_stride, betas, sd_t, feat, pd, vs, vp);
        return;
    }
    static const bool single = tune_env("GSR_BLEND_SINGLE", 1) != 0;  // 0: B = 1 on the 16-frame kernel (A/B)
    if (B == 1 && single) {
        const size_t lds = lbs_blend_lds(NB, vp ? NP : 0, 1, kLbsSplit1);
        lbs_blend_attr(lds);
        hipLaunchKernelGGL((k_lbs_blend<1, kLbsSplit1>), lbs_blend_grid(M, B, 1), dim3(64 * kLbsSplit1), lds, s, B, M,
                           NB, vp ? NP : 0, vt, vt_stride, betas, sd_t, feat, pd, vs, vp);
        return;
    }
    const size_t lds = lbs_blend_lds(NB, vp ? NP : 0, kLbsFrames, kLbsSplit);
    lbs_blend_attr(lds);
    hipLaunchKernelGGL((k_lbs_blend<kLbsFrames, kLbsSplit>), lbs_blend_grid(M, B, kLbsFrames), dim3(64 * kLbsSplit),
                       lds, s, B, M, NB, vp ? NP : 0, vt, vt_stride, betas, sd_t, feat, pd, vs, vp);
}

// vertices2joints (lbs.py:335-352): J[b,j,:] = sum_v J_regressor[j,v] v_shaped[b,v,:], plus
// joints_offset (lbs.py:191/:295).  One workgroup per (group of kJointsPerWG joints, frame), so a
// frame's vertices are read once per group rather than once per joint; fixed-shape tree reduction.
constexpr int kJointsPerWG = 4;

__global__ __launch_bounds__(256) void k_lbs_joints(int V, int J, const float* __restrict__ jreg,
                                                    const float* __restrict__ v_shaped,
                                                    const float* __restrict__ joff,
                                                    float* __restrict__ joints) {
    __shared__ float red[3 * kJointsPerWG][256];
    const int j0 = blockIdx.x * kJointsPerWG, b = blockIdx.y;
    const int nj = min(kJointsPerWG, J - j0);
    const float* vs = v_shaped + (int64_t)b * V * 3;
    float acc[kJointsPerWG][3];
#pragma unroll
    for (int q = 0; q < kJointsPerWG; q++) acc[q][0] = acc[q][1] = acc[q][2] = 0.f;
    // four vertices' loads in flight per round; each thread still sums its vertices in index order
    constexpr int kU = 4;
    int v0 = threadIdx.x;
    for (; v0 + 256 * (kU - 1) < V; v0 += 256 * kU) {
        float x[kU], y[kU], z[kU], wv[kU][kJointsPerWG];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int v = v0 + 256 * u;
            x[u] = vs[3 * v]; y[u] = vs[3 * v + 1]; z[u] = vs[3 * v + 2];
#pragma unroll
            for (int q = 0; q < kJointsPerWG; q++) wv[u][q] = q < nj ? jreg[(int64_t)(j0 + q) * V + v] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; u++)
#pragma unroll
            for (int q = 0; q < kJointsPerWG; q++) {
                acc[q][0] = fmaf(wv[u][q], x[u], acc[q][0]);
                acc[q][1] = fmaf(wv[u][q], y[u], acc[q][1]);
                acc[q][2] = fmaf(wv[u][q], z[u], acc[q][2]);
            }
    }
    for (int v = v0; v < V; v += 256) {
        const float x = vs[3 * v], y = vs[3 * v + 1], z = vs[3 * v + 2];
#pragma unroll
        for (int q = 0; q < kJointsPerWG; q++) {
            const float wv = q < nj ? jreg[(int64_t)(j0 + q) * V + v] : 0.f;
            acc[q][0] = fmaf(wv, x, acc[q][0]);
            acc[q][1] = fmaf(wv, y, acc[q][1]);
            acc[q][2] = fmaf(wv, z, acc[q][2]);
        }
    }
#pragma unroll
    for (int q = 0; q < kJointsPerWG; q++)
        for (int c = 0; c < 3; c++) red[3 * q + c][threadIdx.x] = acc[q][c];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int e = 0; e < 3 * kJointsPerWG; e++) red[e][threadIdx.x] += red[e][threadIdx.x + h];
        __syncthreads();
    }
    if ((int)threadIdx.x < 3 * nj) {
        const int q = threadIdx.x / 3, c = threadIdx.x - 3 * q;
        float v = red[threadIdx.x][0];
        if (joff) v = v + joff[((int64_t)b * J + j0 + q) * 3 + c];
        joints[((int64_t)b * J + j0 + q) * 3 + c] = v;
    }
}

// vertices2joints over the J_regressor's nonzeros (CSR rows, vertex order; gsr_lbs_sp): one wave
// per (joint, frame), lanes take the row's nonzeros 64 at a time (each lane its own fmaf chain in
// index order), then a fixed xor-tree across the lanes -- deterministic run to run.  SMPL-X / FLAME
// joint regressors are sparse (a joint averages a few dozen vertices), so a frame's joints cost one
// load round instead of the dense kernel's pass over J x V weights.
__global__ __launch_bounds__(256) void k_lbs_joints_csr(int B, int V, int J, const int32_t* __restrict__ row,
                                                        const int32_t* __restrict__ col,
                                                        const float* __restrict__ val,
                                                        const float* __restrict__ v_shaped,
                                                        const float* __restrict__ joff,
                                                        float* __restrict__ joints) {
    const int w = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (w >= B * J) return;
    const int b = w / J, j = w - b * J;
    const float* vs = v_shaped + (int64_t)b * V * 3;
    float x = 0.f, y = 0.f, z = 0.f;
    for (int k = row[j] + lane; k < row[j + 1]; k += 64) {
        const int v = col[k];
        const float wv = val[k];
        x = fmaf(wv, vs[3 * v], x);
        y = fmaf(wv, vs[3 * v + 1], y);
        z = fmaf(wv, vs[3 * v + 2], z);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        x += __shfl_xor(x, off);
        y += __shfl_xor(y, off);
        z += __shfl_xor(z, off);
    }
    if (lane < 3) {
        float v = lane == 0 ? x : lane == 1 ? y : z;
        if (joff) v = v + joff[((int64_t)b * J + j) * 3 + lane];
        joints[((int64_t)b * J + j) * 3 + lane] = v;
    }
}

// batch_rigid_transform (lbs.py:426-482), one frame per workgroup: local transforms
// [R | J_i - J_parent], the chain product chain_i = chain_parent . local_i, posed joints =
// chain[:, :3, 3], A = chain - pad(chain . [J; 0]).  The chain runs level by level of the kinematic
// tree (16 threads per joint, one matrix element each): every joint of a level in one step, so
// SMPL-X's 54 sequential products become its tree depth (~10) barrier steps -- each product is
// the same expression as the sequential chain's, so the results are identical.
// rot == null: each joint's rotation from the pose (rodrigues_one), as the single-frame path does.
// jrow != null (single frame, CSR regressor): the rest joints are regressed here first -- each of the
// 16 waves takes joints w, w + 16, ... with k_lbs_joints_csr's per-lane chains and xor tree (the same
// sums, bit for bit) -- and written to `joints`, one launch fewer per lbs call.
// At B > 1 the same per frame (workgroup b: frame b's v_shaped, offsets and joints).
// nchain < gridDim.x: the workgroups past the chains only regress joints -- frame (blockIdx.x - nchain)
// of another model, xj (EHM's unspliced body template beside the FLAME head's chain: its inputs are
// ready at the same point).  They read nothing a chain workgroup writes, and the reverse.
struct ChainJoints {
    const int32_t* row;
    const int32_t* col;
    const float* val;
    const float* vs;    // v_shaped [B][V][3]
    const float* joff;  // [B][J][3], or null
    float* joints;      // [B][J][3] out
    int V, J;
};
// the rest joints of frame b, k_lbs_joints_csr's sums: the workgroup's 16 waves take joints w, w + 16, ...
__device__ __forceinline__ void chain_regress_joints(const ChainJoints& cj, int b, int t, float* sjt) {
    const int w = t >> 6, lane = t & 63;
    const float* vs = cj.vs + (int64_t)b * cj.V * 3;
    for (int j = w; j < cj.J; j += 16) {
        float x = 0.f, y = 0.f, z = 0.f;
        for (int k = cj.row[j] + lane; k < cj.row[j + 1]; k += 64) {
            const int v = cj.col[k];
            const float wv = cj.val[k];
            x = fmaf(wv, vs[3 * v], x);
            y = fmaf(wv, vs[3 * v + 1], y);
            z = fmaf(wv, vs[3 * v + 2], z);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            x += __shfl_xor(x, off);
            y += __shfl_xor(y, off);
            z += __shfl_xor(z, off);
        }
        if (lane < 3) {
            float v = lane == 0 ? x : lane == 1 ? y : z;
            if (cj.joff) v = v + cj.joff[((int64_t)b * cj.J + j) * 3 + lane];
            if (sjt) sjt[3 * j + lane] = v;
            cj.joints[((int64_t)b * cj.J + j) * 3 + lane] = v;
        }
    }
}
__global__ __launch_bounds__(16 * GSR_LBS_MAX_JOINTS) void k_lbs_chain(int J, Parents par,
                                                                     const float* __restrict__ rot,
                                                                     const float* __restrict__ joints,
                                                                     float* __restrict__ jtrans,
                                                                     float* __restrict__ A,
                                                                     const float* __restrict__ pose, int pose2rot,
                                                                     ChainJoints cj, int nchain, ChainJoints xj) {
    __shared__ float tm[GSR_LBS_MAX_JOINTS][16];
    __shared__ float ch[GSR_LBS_MAX_JOINTS][16];
    __shared__ int depth[GSR_LBS_MAX_JOINTS];
    __shared__ float sjt[GSR_LBS_MAX_JOINTS * 3];
    __shared__ int maxd;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= nchain) {  // (the whole workgroup, before any barrier)
        chain_regress_joints(xj, b - nchain, t, nullptr);
        return;
    }
    const float* Jb = joints + (int64_t)b * J * 3;
    if (cj.row) {
        chain_regress_joints(cj, b, t, sjt);
        __syncthreads();
        Jb = sjt;
    }
    if (t == 0) maxd = 0;
    if (t < J) {
        float R[9];
        if (rot) {
#pragma unroll
            for (int e = 0; e < 9; e++) R[e] = rot[((int64_t)b * J + t) * 9 + e];
        } else {
            rodrigues_one(pose, b * J + t, pose2rot, R);
        }
        float rel[3];
        for (int c = 0; c < 3; c++) rel[c] = t == 0 ? Jb[c] : Jb[3 * t + c] - Jb[3 * par.p[t] + c];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) tm[t][4 * r + c] = R[3 * r + c];
            tm[t][4 * r + 3] = rel[r];
        }
        tm[t][12] = 0.f; tm[t][13] = 0.f; tm[t][14] = 0.f; tm[t][15] = 1.f;
        int dd = 0;
        for (int i = t; i > 0 && dd < GSR_LBS_MAX_JOINTS; i = par.p[i]) dd++;  // (parents precede children)
        depth[t] = dd;
    }
    __syncthreads();
    if (t < J) atomicMax(&maxd, depth[t]);
    if (t < 16) ch[0][t] = tm[0][t];
    __syncthreads();
    const int j = t >> 4, e = t & 15, r = e >> 2, c = e & 3;
    const int dj = j < J ? depth[j] : -1;
    for (int lvl = 1; lvl <= maxd; lvl++) {
        if (dj == lvl) {
            const float* P = ch[par.p[j]];
            const float* L = tm[j];
            ch[j][e] = P[4 * r] * L[c] + P[4 * r + 1] * L[4 + c] + P[4 * r + 2] * L[8 + c] + P[4 * r + 3] * L[12 + c];
        }
        __syncthreads();
    }
    if (t < J) {
        const float* T = ch[t];
        const float jx = Jb[3 * t], jy = Jb[3 * t + 1], jz = Jb[3 * t + 2];
        float* a = A + ((int64_t)b * J + t) * 16;
        for (int rr = 0; rr < 4; rr++) {
            const float tj = T[4 * rr] * jx + T[4 * rr + 1] * jy + T[4 * rr + 2] * jz + T[4 * rr + 3] * 0.0f;
            a[4 * rr] = T[4 * rr];
            a[4 * rr + 1] = T[4 * rr + 1];
            a[4 * rr + 2] = T[4 * rr + 2];
            a[4 * rr + 3] = T[4 * rr + 3] - tj;
        }
        if (jtrans)
            for (int rr = 0; rr < 3; rr++) jtrans[((int64_t)b * J + t) * 3 + rr] = T[4 * rr + 3];
    }
}

// Skinning over each vertex's nonzero weights (ELL: K (joint, weight) pairs per vertex, joints
// increasing, padding weight 0; gsr_lbs_sp): the same fmaf chains in joint order as k_lbs_skin,
// minus its terms with a zero weight (fma(0, a, t) == t), so the results are bit-identical to the
// dense kernel's with K loads per vertex instead of J.
template <int KMAX>
__global__ __launch_bounds__(256) void k_lbs_skin_ell(int V, int J, int K, const int32_t* __restrict__ sj,
                                                      const float* __restrict__ sw,
                                                      const float* __restrict__ A,
                                                      const float* __restrict__ v_posed,
                                                      float* __restrict__ verts,
                                                      float* __restrict__ vtrans) {
    __shared__ float As[GSR_LBS_MAX_JOINTS * 16];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < J * 16; i += blockDim.x) As[i] = A[(int64_t)b * J * 16 + i];
    __syncthreads();
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    int jj[KMAX];
    float ww[KMAX];
#pragma unroll
    for (int u = 0; u < KMAX; u++) {
        jj[u] = u < K ? min((int)sj[(int64_t)u * V + v], J - 1) : 0;  // (in range by contract; clamped)
        ww[u] = u < K ? sw[(int64_t)u * V + v] : 0.f;
    }
    float T[16];
#pragma unroll
    for (int e = 0; e < 16; e++) T[e] = 0.f;
#pragma unroll
    for (int u = 0; u < KMAX; u++) {
        if (u >= K) break;
        const float* Aj = As + 16 * jj[u];
#pragma unroll
        for (int e = 0; e < 16; e++) T[e] = fmaf(ww[u], Aj[e], T[e]);
    }
    const float* vp = v_posed + ((int64_t)b * V + v) * 3;
    const float px = vp[0], py = vp[1], pz = vp[2];
    float* out = verts + ((int64_t)b * V + v) * 3;
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = T[4 * r] * px + T[4 * r + 1] * py + T[4 * r + 2] * pz + T[4 * r + 3] * 1.0f;
    if (vtrans) {
        float* o = vtrans + ((int64_t)b * V + v) * 16;
#pragma unroll
        for (int e = 0; e < 16; e++) o[e] = T[e];
    }
}

// Skinning (lbs.py:218-227 / :320-331): T = W . A per vertex, v = T [v_posed; 1].
__global__ __launch_bounds__(256) void k_lbs_skin(int V, int J, const float* __restrict__ w_t,
                                                  const float* __restrict__ A,
                                                  const float* __restrict__ v_posed,
                                                  float* __restrict__ verts,
                                                  float* __restrict__ vtrans) {
    __shared__ float As[GSR_LBS_MAX_JOINTS * 16];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < J * 16; i += blockDim.x) As[i] = A[(int64_t)b * J * 16 + i];
    __syncthreads();
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    // T = sum_j w_j A_j as 8 packed pairs (v_pk_fma_f32: two independent fmaf chains per
    // instruction, each in j order); four weight loads in flight per round
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 T2[8];
#pragma unroll
    for (int e = 0; e < 8; e++) T2[e] = f2{0.f, 0.f};
    const f2* A2 = reinterpret_cast<const f2*>(As);
    // 16 weight loads in flight per round (the kernel is load-latency bound; J <= 64 is 4 rounds)
    for (int j0 = 0; j0 < J; j0 += 16) {
        float w16[16];
#pragma unroll
        for (int u = 0; u < 16; u++) w16[u] = j0 + u < J ? w_t[(int64_t)(j0 + u) * V + v] : 0.f;
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if (j0 + u >= J) break;
#pragma unroll
            for (int e = 0; e < 8; e++)
                T2[e] = __builtin_elementwise_fma(f2{w16[u], w16[u]}, A2[8 * (j0 + u) + e], T2[e]);
        }
    }
    float T[16];
#pragma unroll
    for (int e = 0; e < 8; e++) { T[2 * e] = T2[e].x; T[2 * e + 1] = T2[e].y; }
    const float* p = v_posed + ((int64_t)b * V + v) * 3;
    const float x = p[0], y = p[1], z = p[2];
    float* o = verts + ((int64_t)b * V + v) * 3;
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = T[4 * r] * x + T[4 * r + 1] * y + T[4 * r + 2] * z + T[4 * r + 3] * 1.0f;
    if (vtrans) {
        float4* tv = reinterpret_cast<float4*>(vtrans + ((int64_t)b * V + v) * 16);
        tv[0] = make_float4(T[0], T[1], T[2], T[3]);
        tv[1] = make_float4(T[4], T[5], T[6], T[7]);
        tv[2] = make_float4(T[8], T[9], T[10], T[11]);
        tv[3] = make_float4(T[12], T[13], T[14], T[15]);
    }
}

// EHM.forward's head splice (EHM.py:72-75, :121-124): the FLAME head vertices (+ eyelid blend
// shapes, times head_scale) replace the body template's FLAME-mapped vertices, re-anchored from the
// mean of head joints [hj0, hj1) to the mean of body joints [bj0, bj1).
__global__ __launch_bounds__(256) void k_splice_head(
    int Vb, int Nh, const int32_t* __restrict__ idx, const float* __restrict__ head,
    const float* __restrict__ r_eyelid, const float* __restrict__ l_eyelid,
    const float* __restrict__ eyelid, const float* __restrict__ head_scale,
    const float* __restrict__ hjoints, int Jh, int hj0, int hj1, const float* __restrict__ bjoints,
    int Jb, int bj0, int bj1, float* __restrict__ body, uint32_t* __restrict__ bad) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nh) return;
    const int d = idx[i];
    if (d < 0 || d >= Vb) {
        if (bad) atomicOr(bad, 2u);
        return;
    }
    const float* hj = hjoints + (int64_t)b * Jh * 3;
    const float* bjt = bjoints + (int64_t)b * Jb * 3;
    for (int c = 0; c < 3; c++) {
        float h = head[((int64_t)b * Nh + i) * 3 + c];
        if (eyelid) {
            h = h + r_eyelid[3 * i + c] * eyelid[2 * b + 1];
            h = h + l_eyelid[3 * i + c] * eyelid[2 * b];
        }
        if (head_scale) h = h * head_scale[3 * b + c];
        float hs = 0.f, bs = 0.f;
        for (int j = hj0; j < hj1; j++) hs += hj[3 * j + c];
        for (int j = bj0; j < bj1; j++) bs += bjt[3 * j + c];
        body[((int64_t)b * Vb + d) * 3 + c] = (h - hs / (float)(hj1 - hj0)) + bs / (float)(bj1 - bj0);
    }
}

// (rotmat_to_unitquat, quat_product, dot3 and face_frame: deform_dev.h)

constexpr int kDeformFrames = 8;  // frames per workgroup (GSR_DEFORM_FRAMES overrides, timing only)
constexpr int kFrStride = 15;  // LDS floats per face frame (odd: conflict-free per-thread rows)

// Vertex Gaussians (ubody_gaussian.py:252-254): xyz = LBS vertex, rotation =
// normalize(q(T_v[:3,:3]) (x) q_v) in wxyz, scale unchanged.  UV Gaussians (:257-271): frame
// [a0 a1 a2], scale s and q(frame) of the deformed binding face, centre = bary . face vertices,
// xyz = (frame . local) * s + centre, rotation = q(frame) (x) q_uv (not renormalised), scale =
// scale * s.
//
// One thread per Gaussian and fpw frames per workgroup: the frame-independent inputs (binding,
// face vertex indices, barycentrics and, when shared, local offsets / rotations / scales) are read
// once per workgroup instead of once per frame, which is most of the kernel's HBM traffic.  Face
// frames are computed once per (face, frame) as the reference does: GUAVA's UV Gaussians come in
// texel order, so a workgroup's 256 Gaussians bind a short run of faces, and the workgroup
// computes that run's frames into LDS (one thread per face) for its Gaussians to read; a
// workgroup whose faces span more than 256 ids computes per Gaussian (same function, same bits).
__global__ __launch_bounds__(256) void k_deform_gaussians(
    int B, int fpw, int V, int F, int N, const float* __restrict__ verts, const float* __restrict__ vtrans,
    const int32_t* __restrict__ faces, const float* __restrict__ vrot, int64_t s_vrot,
    const float* __restrict__ vscale, int64_t s_vscale, const int32_t* __restrict__ bind,
    const float* __restrict__ bary, const float* __restrict__ lxyz, int64_t s_lxyz,
    const float* __restrict__ urot, int64_t s_urot, const float* __restrict__ uscale,
    int64_t s_uscale, float* __restrict__ means, float* __restrict__ rots, float* __restrict__ scales,
    uint32_t* __restrict__ bad) {
    __shared__ float fr_lds[256 * kFrStride];
    __shared__ int range[2];
    const int P = V + N;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool uv = i >= V && i < P;
    const int n = i - V;
    // binding resolved once (reference: an IndexError; here a flag and NaN outputs)
    int f = -1, j0 = 0, j1 = 0, j2 = 0;
    if (uv) {
        const int bf = bind[n];
        if (bf >= 0 && bf < F) {
            const int a = faces[3 * bf], c = faces[3 * bf + 1], d = faces[3 * bf + 2];
            if (a >= 0 && a < V && c >= 0 && c < V && d >= 0 && d < V) { f = bf; j0 = a; j1 = c; j2 = d; }
        }
        if (f < 0 && bad) atomicOr(bad, 1u);
    }
    float w0 = 0.f, w1 = 0.f, w2 = 0.f;
    if (uv) { w0 = bary[3 * n]; w1 = bary[3 * n + 1]; w2 = bary[3 * n + 2]; }
    // the workgroup's face run
    if (threadIdx.x == 0) { range[0] = INT_MAX; range[1] = -1; }
    __syncthreads();
    if (f >= 0) { atomicMin(&range[0], f); atomicMax(&range[1], f); }
    __syncthreads();
    const int fmin = range[0], nf = range[1] - range[0] + 1;
    const bool shared_frames = range[1] >= 0 && nf <= 256;
    int t0 = -1, t1 = 0, t2 = 0;  // this thread's face in the run (shared mode)
    if (shared_frames && (int)threadIdx.x < nf) {
        const int ff = fmin + threadIdx.x;
        const int a = faces[3 * ff], c = faces[3 * ff + 1], d = faces[3 * ff + 2];
        if (a >= 0 && a < V && c >= 0 && c < V && d >= 0 && d < V) { t0 = a; t1 = c; t2 = d; }
    }
    const int b1 = min(B, (int)(blockIdx.y + 1) * fpw);
    for (int b = blockIdx.y * fpw; b < b1; b++) {
        const float* vb = verts + (int64_t)b * V * 3;
        if (shared_frames) {
            if (b > blockIdx.y * fpw) __syncthreads();  // the previous frame's readers are done
            if (t0 >= 0) face_frame(vb, t0, t1, t2, fr_lds + threadIdx.x * kFrStride);
            __syncthreads();
        }
        if (i >= P) continue;
        const int64_t o = (int64_t)b * P + i;
        if (i < V) {
            const float4* tv = reinterpret_cast<const float4*>(vtrans + ((int64_t)b * V + i) * 16);
            const float4 r0 = tv[0], r1 = tv[1], r2 = tv[2];
            const float m[9] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z};
            const float4 qd = rotmat_to_unitquat(m);
            const float* qv = vrot + b * s_vrot + 4 * (int64_t)i;  // wxyz
            const float4 q = quat_product(qd, make_float4(qv[1], qv[2], qv[3], qv[0]));
            // F.normalize over the wxyz vector: x / max(||x||, 1e-12)
            const float nn = fmaxf(sqrtf(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z), 1e-12f);
            reinterpret_cast<float4*>(rots)[o] = make_float4(q.w / nn, q.x / nn, q.y / nn, q.z / nn);
            for (int c = 0; c < 3; c++) {
                means[3 * o + c] = vb[3 * i + c];
                scales[3 * o + c] = vscale[b * s_vscale + 3 * (int64_t)i + c];
            }
            continue;
        }
        if (f < 0) {
            const float nan = __int_as_float(0x7fc00000);
            for (int c = 0; c < 3; c++) { means[3 * o + c] = nan; scales[3 * o + c] = nan; }
            reinterpret_cast<float4*>(rots)[o] = make_float4(nan, nan, nan, nan);
            continue;
        }
        float fr[14];
        if (shared_frames) {
            const float* src = fr_lds + (f - fmin) * kFrStride;
#pragma unroll
            for (int k = 0; k < 14; k++) fr[k] = src[k];
        } else {
            face_frame(vb, j0, j1, j2, fr);
        }
        const float s = fr[9];
        const float* qu = urot + b * s_urot + 4 * (int64_t)n;  // wxyz
        const float4 q = quat_product(make_float4(fr[10], fr[11], fr[12], fr[13]), make_float4(qu[1], qu[2], qu[3], qu[0]));
        if (!GSR_DEFORM_NOSTORE || q.w == 12345.f) reinterpret_cast<float4*>(rots)[o] = make_float4(q.w, q.x, q.y, q.z);
        const float* l = lxyz + b * s_lxyz + 3 * (int64_t)n;
        const float lx = l[0], ly = l[1], lz = l[2];
        const float cx = (w0 * vb[3 * j0] + w1 * vb[3 * j1]) + w2 * vb[3 * j2];
        const float cy = (w0 * vb[3 * j0 + 1] + w1 * vb[3 * j1 + 1]) + w2 * vb[3 * j2 + 1];
        const float cz = (w0 * vb[3 * j0 + 2] + w1 * vb[3 * j1 + 2]) + w2 * vb[3 * j2 + 2];
        const float mx = dot3(fr[0], fr[1], fr[2], lx, ly, lz) * s + cx;
        const float my = dot3(fr[3], fr[4], fr[5], lx, ly, lz) * s + cy;
        const float mz = dot3(fr[6], fr[7], fr[8], lx, ly, lz) * s + cz;
        const float* us = uscale + b * s_uscale + 3 * (int64_t)n;
        if (!GSR_DEFORM_NOSTORE || mx == 12345.f) {
            means[3 * o] = mx; means[3 * o + 1] = my; means[3 * o + 2] = mz;
            for (int c = 0; c < 3; c++) scales[3 * o + c] = us[c] * s;
        }
    }
}

// The avatar pipeline's fused forward (gsr_forward_batch_deformed): k_deform_gaussians' assembly of
// each (Gaussian, frame) -- the same face-frame sharing and the same expressions -- handed in
// registers to the projection of k_preprocess (preprocess_dev.h), which writes the geometry rows
// and the per-block summaries of the frame.  Gaussian blocks of kScanBlock = 256 (the workgroup) are
// preprocess's blocks, so the block summaries index as k_preprocess's.
__global__ __launch_bounds__(256) void k_deform_preprocess(int fpw, GsrDeformInputs dg, Dims d, Inputs in,
                                                           GeomArena g, Outputs o) {
    __shared__ float fr_lds[256 * kFrStride];
    __shared__ int range[2];
    const int V = dg.V, F = dg.F, N = dg.N, P = V + N;
    const int32_t* __restrict__ faces = dg.faces;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool uv = i >= V && i < P;
    const int n = i - V;
    int f = -1, j0 = 0, j1 = 0, j2 = 0;
    if (uv) {
        const int bf = dg.binding_face[n];
        if (bf >= 0 && bf < F) {
            const int a = faces[3 * bf], c = faces[3 * bf + 1], e = faces[3 * bf + 2];
            if (a >= 0 && a < V && c >= 0 && c < V && e >= 0 && e < V) { f = bf; j0 = a; j1 = c; j2 = e; }
        }
        if (f < 0 && dg.bad_index_flag) atomicOr(dg.bad_index_flag, 1u);
    }
    float w0 = 0.f, w1 = 0.f, w2 = 0.f;
    if (uv) { w0 = dg.face_bary[3 * n]; w1 = dg.face_bary[3 * n + 1]; w2 = dg.face_bary[3 * n + 2]; }
    if (threadIdx.x == 0) { range[0] = INT_MAX; range[1] = -1; }
    __syncthreads();
    if (f >= 0) { atomicMin(&range[0], f); atomicMax(&range[1], f); }
    __syncthreads();
    const int fmin = range[0], nf = range[1] - range[0] + 1;
    const bool shared_frames = range[1] >= 0 && nf <= 256;
    int t0 = -1, t1 = 0, t2 = 0;
    if (shared_frames && (int)threadIdx.x < nf) {
        const int ff = fmin + threadIdx.x;
        const int a = faces[3 * ff], c = faces[3 * ff + 1], e = faces[3 * ff + 2];
        if (a >= 0 && a < V && c >= 0 && c < V && e >= 0 && e < V) { t0 = a; t1 = c; t2 = e; }
    }
    const int b1 = min(d.B, (int)(blockIdx.y + 1) * fpw);
    for (int b = blockIdx.y * fpw; b < b1; b++) {
        const float* vb = dg.verts + (int64_t)b * V * 3;
        if (shared_frames) {
            if (b > (int)blockIdx.y * fpw) __syncthreads();
            if (t0 >= 0) face_frame(vb, t0, t1, t2, fr_lds + threadIdx.x * kFrStride);
            __syncthreads();
        }
        // the frame's depth-bucket counters (k_preprocess's duty)
        for (int k = i; k <= d.NB; k += d.nblk * kScanBlock) g.bcount[(int64_t)b * (d.NB + 1) + k] = 0u;
        const int64_t gid = (int64_t)b * P + i;
        uint32_t tiles = 0;
        if (i < P) {
            float mo[3], so[3], qq[4];
            if (i < V) {
                const float4* tv = reinterpret_cast<const float4*>(dg.vert_transforms + ((int64_t)b * V + i) * 16);
                const float4 r0 = tv[0], r1 = tv[1], r2 = tv[2];
                const float m[9] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z};
                const float4 qd = rotmat_to_unitquat(m);
                const float* qv = dg.vtx_rotations + b * dg.vtx_rot_stride + 4 * (int64_t)i;  // wxyz
                const float4 q = quat_product(qd, make_float4(qv[1], qv[2], qv[3], qv[0]));
                const float nn = fmaxf(sqrtf(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z), 1e-12f);
                qq[0] = q.w / nn; qq[1] = q.x / nn; qq[2] = q.y / nn; qq[3] = q.z / nn;
                for (int c = 0; c < 3; c++) {
                    mo[c] = vb[3 * i + c];
                    so[c] = dg.vtx_scales[b * dg.vtx_scale_stride + 3 * (int64_t)i + c];
                }
            } else if (f < 0) {
                const float nan = __int_as_float(0x7fc00000);
                for (int c = 0; c < 3; c++) { mo[c] = nan; so[c] = nan; }
                for (int c = 0; c < 4; c++) qq[c] = nan;
            } else {
                float fr[14];
                if (shared_frames) {
                    const float* src = fr_lds + (f - fmin) * kFrStride;
#pragma unroll
                    for (int k = 0; k < 14; k++) fr[k] = src[k];
                } else {
                    face_frame(vb, j0, j1, j2, fr);
                }
                const float s = fr[9];
                const float* qu = dg.uv_rotations + b * dg.uv_rot_stride + 4 * (int64_t)n;  // wxyz
                const float4 q = quat_product(make_float4(fr[10], fr[11], fr[12], fr[13]),
                                              make_float4(qu[1], qu[2], qu[3], qu[0]));
                qq[0] = q.w; qq[1] = q.x; qq[2] = q.y; qq[3] = q.z;
                const float* l = dg.local_xyz + b * dg.local_stride + 3 * (int64_t)n;
                const float lx = l[0], ly = l[1], lz = l[2];
                const float cx = (w0 * vb[3 * j0] + w1 * vb[3 * j1]) + w2 * vb[3 * j2];
                const float cy = (w0 * vb[3 * j0 + 1] + w1 * vb[3 * j1 + 1]) + w2 * vb[3 * j2 + 1];
                const float cz = (w0 * vb[3 * j0 + 2] + w1 * vb[3 * j1 + 2]) + w2 * vb[3 * j2 + 2];
                mo[0] = dot3(fr[0], fr[1], fr[2], lx, ly, lz) * s + cx;
                mo[1] = dot3(fr[3], fr[4], fr[5], lx, ly, lz) * s + cy;
                mo[2] = dot3(fr[6], fr[7], fr[8], lx, ly, lz) * s + cz;
                const float* us = dg.uv_scales + b * dg.uv_scale_stride + 3 * (int64_t)n;
                for (int c = 0; c < 3; c++) so[c] = us[c] * s;
            }
            tiles = preprocess_one(d, in, g, o, b, gid, mo, nullptr, so, qq, in.opac[in.s_opac * b + i]);
        }
        preprocess_block_sums(d, g, b, blockIdx.x, tiles, gid);
    }
    zero_ctrl_words(d, in, g);  // (in.fwd_only is set: no backward reads this workspace)
}

void launch_deform_preprocess(const Dims& d, const Inputs& in, const GeomArena& g, const Outputs& o,
                              const GsrDeformInputs& dg, hipStream_t s) {
    if (d.P == 0 || d.B == 0) return;
    // 4 frames per workgroup: 118.9 us per 32 frames vs 169.7 / 132.5 / 121.3 / 131.6 at 1 / 2 / 8 / 16
    // (GSR_FUSED_FRAMES; fewer re-reads of the binding set-up against fewer workgroups in flight)
    static const int fpw = [] {
        const int v = tune_env("GSR_FUSED_FRAMES", 4);
        return v >= 1 && v <= 64 ? v : 1;
    }();
    hipLaunchKernelGGL(k_deform_preprocess, dim3(d.nblk, (d.B + fpw - 1) / fpw), dim3(256), 0, s, fpw, dg, d, in,
                       g, o);
}

// Backward of k_deform_gaussians with respect to the canonical attributes (deform_dev.h): one thread
// per Gaussian walks frames [blockIdx.y * fpw, ...) in frame order.  An attribute shared by every
// frame (stride 0) gets its frame sum, accumulated in registers and written once (the launch then has
// grid.y = 1, as k_preprocess_bwd's reduce mode); a per-frame attribute gets one row per frame.  No
// atomics, no scatter, so the sums are deterministic.  Face frames are recomputed per thread (the
// forward's face_frame): the kernel has no LDS and no barrier.  A Gaussian with an out-of-range
// binding gets zero rows and sets the flag; nothing is read out of range.  verts and
// vert_transforms get no gradient (include/gsr_deform.h).
__global__ __launch_bounds__(256) void k_deform_gaussians_bwd(int B, int fpw, GsrDeformInputs dg,
                                                              const float* __restrict__ g_means,
                                                              const float* __restrict__ g_rots,
                                                              const float* __restrict__ g_scales, GsrDeformGrads o) {
    const int V = dg.V, N = dg.N, P = V + N;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int b0 = blockIdx.y * fpw, b1 = min(B, b0 + fpw);
    if (i < V) {
        float ar[4] = {0.f, 0.f, 0.f, 0.f}, as[3] = {0.f, 0.f, 0.f};
        for (int b = b0; b < b1; b++) {
            const int64_t gid = (int64_t)b * P + i;
            if (o.vtx_rotations) {
                const float* qv = dg.vtx_rotations + b * dg.vtx_rot_stride + 4 * (int64_t)i;
                const float q[4] = {qv[0], qv[1], qv[2], qv[3]};
                const float g[4] = {g_rots[4 * gid], g_rots[4 * gid + 1], g_rots[4 * gid + 2], g_rots[4 * gid + 3]};
                float dq[4];
                deform_bwd_vertex_rot(dg.vert_transforms + ((int64_t)b * V + i) * 16, q, g, dq);
                if (dg.vtx_rot_stride) {
#pragma unroll
                    for (int k = 0; k < 4; k++) o.vtx_rotations[b * dg.vtx_rot_stride + 4 * (int64_t)i + k] = dq[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) ar[k] += dq[k];
                }
            }
            if (o.vtx_scales) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float gs = g_scales[3 * gid + k];
                    if (dg.vtx_scale_stride) o.vtx_scales[b * dg.vtx_scale_stride + 3 * (int64_t)i + k] = gs;
                    else as[k] += gs;
                }
            }
        }
        if (o.vtx_rotations && !dg.vtx_rot_stride)
#pragma unroll
            for (int k = 0; k < 4; k++) o.vtx_rotations[4 * (int64_t)i + k] = ar[k];
        if (o.vtx_scales && !dg.vtx_scale_stride)
#pragma unroll
            for (int k = 0; k < 3; k++) o.vtx_scales[3 * (int64_t)i + k] = as[k];
        return;
    }
    const int n = i - V;
    const DeformBinding bd = resolve_binding(dg.binding_face, dg.faces, n, V, dg.F);
    if (bd.f < 0 && dg.bad_index_flag && blockIdx.y == 0) atomicOr(dg.bad_index_flag, 1u);
    float al[3] = {0.f, 0.f, 0.f}, ar[4] = {0.f, 0.f, 0.f, 0.f}, as[3] = {0.f, 0.f, 0.f};
    for (int b = b0; b < b1; b++) {
        const int64_t gid = (int64_t)b * P + i;
        float dl[3] = {0.f, 0.f, 0.f}, dr[4] = {0.f, 0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f};
        if (bd.f >= 0) {
            float fr[14];
            face_frame_bwd(dg.verts + (int64_t)b * V * 3, bd.j0, bd.j1, bd.j2, fr);
            float gm[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f};
            if (o.local_xyz)
#pragma unroll
                for (int k = 0; k < 3; k++) gm[k] = g_means[3 * gid + k];
            if (o.uv_rotations)
#pragma unroll
                for (int k = 0; k < 4; k++) gq[k] = g_rots[4 * gid + k];
            if (o.uv_scales)
#pragma unroll
                for (int k = 0; k < 3; k++) gs[k] = g_scales[3 * gid + k];
            deform_bwd_uv(fr, gm, gq, gs, dl, dr, ds);
        }
        if (o.local_xyz) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (dg.local_stride) o.local_xyz[b * dg.local_stride + 3 * (int64_t)n + k] = dl[k];
                else al[k] += dl[k];
            }
        }
        if (o.uv_rotations) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (dg.uv_rot_stride) o.uv_rotations[b * dg.uv_rot_stride + 4 * (int64_t)n + k] = dr[k];
                else ar[k] += dr[k];
            }
        }
        if (o.uv_scales) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (dg.uv_scale_stride) o.uv_scales[b * dg.uv_scale_stride + 3 * (int64_t)n + k] = ds[k];
                else as[k] += ds[k];
            }
        }
    }
    if (o.local_xyz && !dg.local_stride)
#pragma unroll
        for (int k = 0; k < 3; k++) o.local_xyz[3 * (int64_t)n + k] = al[k];
    if (o.uv_rotations && !dg.uv_rot_stride)
#pragma unroll
        for (int k = 0; k < 4; k++) o.uv_rotations[4 * (int64_t)n + k] = ar[k];
    if (o.uv_scales && !dg.uv_scale_stride)
#pragma unroll
        for (int k = 0; k < 3; k++) o.uv_scales[3 * (int64_t)n + k] = as[k];
}

struct PackTable {
    GsrRowSegment seg[GSR_PACK_MAX_SEGMENTS];
};

// gsr_pack_rows: one workgroup per (segment, frame); a row piece is at most a few hundred floats
__global__ __launch_bounds__(256) void k_pack_rows(PackTable t) {
    const GsrRowSegment sg = t.seg[blockIdx.x];
    const int b = blockIdx.y;
    for (int c = threadIdx.x; c < sg.width; c += 256)
        sg.dst[b * sg.dst_stride + c] = sg.src ? sg.src[b * sg.src_stride + c] : 0.f;
}

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct LbsArena {
    float *rot, *feat, *vs, *vp, *joints, *A;
    float *beta_tiles, *feat_tiles;  // the matrix-core blend's coefficient tiles (B > kLbsFrames)
};

size_t coef_tile_floats(int B, int K) { return (size_t)((B + 31) / 32) * (size_t)((K + 7) / 8) * 256; }

// (the tiles come last: lbs_skin_splice carves without NB for A and v_posed)
size_t carve_lbs(char* base, int B, int V, int J, int NB, LbsArena* a) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += align256(bytes);
        return reinterpret_cast<float*>(p);
    };
    const size_t f = sizeof(float);
    LbsArena t;
    t.rot = take(f * (size_t)B * J * 9);
    t.feat = take(f * (size_t)B * (J > 1 ? J - 1 : 1) * 9);
    t.vs = take(f * (size_t)B * V * 3);
    t.vp = take(f * (size_t)B * V * 3);
    t.joints = take(f * (size_t)B * J * 3);
    t.A = take(f * (size_t)B * J * 16);
    t.beta_tiles = take(f * coef_tile_floats(B, NB > 0 ? NB : 0));
    t.feat_tiles = take(f * coef_tile_floats(B, 9 * (J - 1)));
    if (a) *a = t;
    return off;
}

int hip_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(GSR_ERR_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
    return 0;
}

}  // namespace

// gsr_deform_gaussians' host-side checks on a GsrDeformInputs (also gsr_backward_batch_deformed's)
int check_deform_inputs(int B, const GsrDeformInputs* dg, const char* who) {
    auto bad = [&](const char* msg) { return api_fail(GSR_ERR_ARG, (std::string(who) + ": " + msg).c_str()); };
    if (!dg) return bad("null deform inputs");
    if (B <= 0 || dg->V < 0 || dg->N < 0 || dg->F < 0) return bad("bad sizes");
    if (dg->V + dg->N == 0) return 0;
    if (!dg->verts) return bad("null required pointer");
    if (dg->V > 0 && (!dg->vert_transforms || !dg->vtx_rotations || !dg->vtx_scales))
        return bad("vertex Gaussians need transforms, rotations, scales");
    if (dg->N > 0 && (!dg->faces || !dg->binding_face || !dg->face_bary || !dg->local_xyz || !dg->uv_rotations ||
                      !dg->uv_scales || dg->F == 0))
        return bad("UV Gaussians need faces and binding data");
    auto bad_stride = [](int64_t st, int64_t full) { return st != 0 && st != full; };
    if (bad_stride(dg->vtx_rot_stride, 4LL * dg->V) || bad_stride(dg->vtx_scale_stride, 3LL * dg->V) ||
        bad_stride(dg->local_stride, 3LL * dg->N) || bad_stride(dg->uv_rot_stride, 4LL * dg->N) ||
        bad_stride(dg->uv_scale_stride, 3LL * dg->N))
        return bad("strides must be 0 or a whole frame");
    return 0;
}

}  // namespace gsr

using namespace gsr;

// The tiled layout of a k-major base (GsrLbsSparse.*_tiled): one float4 per thread.
__global__ __launch_bounds__(256) void k_lbs_tile_base(int K, int M, int64_t n4, const float* __restrict__ base,
                                                       float4* __restrict__ tiled) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int nkg = (K + 7) / 8;
    const int lane = (int)(i & 63);
    const int64_t tg = i >> 6;
    const int g = (int)(tg % nkg), t = (int)(tg / nkg);
    const int m = 32 * t + (lane & 31), k0 = 8 * g + 4 * (lane >> 5);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = (m < M && k0 + j < K) ? base[(int64_t)(k0 + j) * M + m] : 0.f;
    tiled[i] = make_float4(v[0], v[1], v[2], v[3]);
}

extern "C" {

size_t gsr_lbs_workspace_bytes(int B, int V, int J, int NB) {
    if (B <= 0 || V <= 0 || J <= 0) return 0;
    return carve_lbs(nullptr, B, V, J, NB, nullptr);
}

}  // extern "C"

namespace {
// the joint regression of gsr_lbs / gsr_blend_joints: CSR rows when given, else the dense kernel
void launch_joints(int B, int V, int J, const float* J_regressor, const GsrLbsSparse* sp, const float* vs,
                   const float* joints_offset, float* joints, hipStream_t s) {
    if (sp && sp->jreg_row) {
        hipLaunchKernelGGL(k_lbs_joints_csr, dim3((B * J + 3) / 4), dim3(256), 0, s, B, V, J, sp->jreg_row,
                           sp->jreg_col, sp->jreg_val, vs, joints_offset, joints);
    } else {
        hipLaunchKernelGGL(k_lbs_joints, dim3((J + kJointsPerWG - 1) / kJointsPerWG, B), dim3(256), 0, s, V, J,
                           J_regressor, vs, joints_offset, joints);
    }
}
// NB: shape coefficients of the call, V: its vertices (the pose base is 9(J-1) x 3V)
int check_sparse(const GsrLbsSparse* sp, int J, int NB, int V, const char* who) {
    if (!sp) return 0;
    if (sp->jreg_row && (!sp->jreg_col || !sp->jreg_val))
        return api_fail(GSR_ERR_ARG, (std::string(who) + ": jreg_row without jreg_col / jreg_val").c_str());
    if (sp->skin_k && (sp->skin_k < 0 || sp->skin_k > GSR_LBS_SKIN_MAX_K || !sp->skin_joint || !sp->skin_weight))
        return api_fail(GSR_ERR_ARG, (std::string(who) + ": skin_k must be in [1, 16] with its arrays").c_str());
    if (((uintptr_t)sp->shapedirs_tiled | (uintptr_t)sp->posedirs_tiled) & 15)
        return api_fail(GSR_ERR_ARG, (std::string(who) + ": tiled bases must be 16-byte aligned").c_str());
    if (sp->shapedirs_tiled && NB > 0 && (sp->shapedirs_tiled_k != NB || sp->shapedirs_tiled_m != 3 * V))
        return api_fail(GSR_ERR_ARG, (std::string(who) + ": shapedirs_tiled was tiled for another NB x 3V").c_str());
    if (sp->posedirs_tiled && J > 1 && (sp->posedirs_tiled_k != 9 * (J - 1) || sp->posedirs_tiled_m != 3 * V))
        return api_fail(GSR_ERR_ARG, (std::string(who) + ": posedirs_tiled was tiled for another 9(J-1) x 3V").c_str());
    return 0;
}
}  // namespace

extern "C" {

int gsr_lbs(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride,
            const float* betas, const float* shapedirs_t, const float* pose, int pose2rot,
            const float* posedirs, const float* J_regressor, const int32_t* parents_host,
            const float* lbs_weights_t, const float* joints_offset, float* verts,
            float* joints_transformed, float* joints, float* vert_transforms,
            float* joint_transforms, float* v_shaped, char* workspace, void* stream) {
    return gsr_lbs_sp(B, V, J, NB, v_template, v_template_stride, betas, shapedirs_t, pose, pose2rot, posedirs,
                      J_regressor, parents_host, lbs_weights_t, joints_offset, verts, joints_transformed, joints,
                      vert_transforms, joint_transforms, v_shaped, workspace, nullptr, stream);
}

int gsr_lbs_sp(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride,
               const float* betas, const float* shapedirs_t, const float* pose, int pose2rot,
               const float* posedirs, const float* J_regressor, const int32_t* parents_host,
               const float* lbs_weights_t, const float* joints_offset, float* verts,
               float* joints_transformed, float* joints, float* vert_transforms,
               float* joint_transforms, float* v_shaped, char* workspace, const GsrLbsSparse* sp,
               void* stream) {
    return gsr::lbs_run(B, V, J, NB, v_template, v_template_stride, betas, shapedirs_t, pose, pose2rot, posedirs,
                        J_regressor, parents_host, lbs_weights_t, joints_offset, verts, joints_transformed, joints,
                        vert_transforms, joint_transforms, v_shaped, workspace, sp, stream, true);
}

}  // extern "C"

namespace gsr {
namespace {
// whether the matrix-core blend of these arguments runs on coefficient tiles (k_lbs_blend_tiledc);
// GSR_BLEND_COEF_TILES=0: the row-major gathers of k_lbs_blend_tiled (A/B)
bool blend_tiledc_applies(int B, int NB, int NP, const float* vp, const GsrLbsSparse* sp) {
    static const bool on = tune_env("GSR_BLEND_TILED", 1) != 0 && tune_env("GSR_BLEND_VALU", 0) != 1 &&
                           tune_env("GSR_BLEND_COEF_TILES", 1) != 0;
    return on && B > kLbsFrames && sp && (NB == 0 || sp->shapedirs_tiled) &&
           (NP == 0 || !vp || sp->posedirs_tiled) && (NB > 0 || (NP > 0 && vp));
}

CoefJob coef_job(int B, int J, int NB, const float* pose, int pose2rot, const float* betas, const LbsArena& a,
                 float* beta_tiles) {
    CoefJob c{};
    c.B = B; c.J = J; c.NB = betas ? NB : 0; c.pose2rot = pose2rot;
    c.n_pose = (pose && J > 1) ? (B + 31) / 32 * 32 * J : 0;
    c.n_beta = c.NB > 0 ? (int)(coef_tile_floats(B, c.NB) / 4) : 0;
    c.pose = pose; c.betas = betas;
    c.feat_tiles = a.feat_tiles;
    c.beta_tiles = reinterpret_cast<float4*>(beta_tiles);
    return c;
}

void launch_coef_tiles(const CoefJob& a, const CoefJob& b, hipStream_t s) {
    const int n = a.n_pose + a.n_beta + b.n_pose + b.n_beta;
    if (n == 0) return;
    hipLaunchKernelGGL(k_lbs_coef_tiles, dim3((n + 255) / 256), dim3(256), 0, s, a, b);
}

BlendTJob blendt_job(int M, int NB, int NP, const float* vt, int64_t vt_stride, const float* beta_tiles,
                     const float* feat_tiles, float* vs, float* vp, const GsrLbsSparse* sp) {
    return BlendTJob{M, NB, vp ? NP : 0, vt, vt_stride, reinterpret_cast<const float4*>(beta_tiles),
                     reinterpret_cast<const float4*>(sp->shapedirs_tiled), reinterpret_cast<const float4*>(feat_tiles),
                     reinterpret_cast<const float4*>(sp->posedirs_tiled), vs, vp};
}

// one blend, or (b != null) two independent ones in one launch
void launch_blend_tiledc(int B, const BlendTJob& a, const BlendTJob* b, hipStream_t s) {
    const int ka = blend_ksplit(a.M), kb = b ? blend_ksplit(b->M) : ka;
    const int waves = ka > kb ? ka : kb;
    const int na = ((a.M + 31) / 32 + waves / ka - 1) / (waves / ka);
    const int nb = b ? ((b->M + 31) / 32 + waves / kb - 1) / (waves / kb) : 0;
    const dim3 grid(na + nb, (B + 31) / 32);
    const BlendTJob jb = b ? *b : a;
#define GSR_BTC(W, KA, KB) \
    hipLaunchKernelGGL((k_lbs_blend_tiledc<W, KA, KB>), grid, dim3(64 * W), 0, s, B, a, na, jb)
    if (ka == 4 && kb == 4) GSR_BTC(4, 4, 4);
    else if (ka == 8 && kb == 8) GSR_BTC(8, 8, 8);
    else if (ka == 8) GSR_BTC(8, 8, 4);
    else GSR_BTC(8, 4, 8);
#undef GSR_BTC
}

int make_parents(int J, const int32_t* parents_host, Parents* par) {
    for (int i = 0; i < GSR_LBS_MAX_JOINTS; i++) par->p[i] = -1;
    if (parents_host[0] != -1) return api_fail(GSR_ERR_ARG, "gsr_lbs: parents[0] must be -1");
    for (int i = 1; i < J; i++) {
        if (parents_host[i] < 0 || parents_host[i] >= i)
            return api_fail(GSR_ERR_ARG, "gsr_lbs: parents must satisfy 0 <= parents[i] < i");
        par->p[i] = (int8_t)parents_host[i];
    }
    return 0;
}

void launch_skin(int B, int V, int J, const float* lbs_weights_t, const GsrLbsSparse* sp, const float* A,
                 const float* vp, float* verts, float* vert_transforms, hipStream_t s) {
    if (sp && sp->skin_k > 0) {
        const dim3 g((V + 255) / 256, B);
        if (sp->skin_k <= 4)
            hipLaunchKernelGGL(k_lbs_skin_ell<4>, g, dim3(256), 0, s, V, J, sp->skin_k, sp->skin_joint,
                               sp->skin_weight, A, vp, verts, vert_transforms);
        else if (sp->skin_k <= 8)
            hipLaunchKernelGGL(k_lbs_skin_ell<8>, g, dim3(256), 0, s, V, J, sp->skin_k, sp->skin_joint,
                               sp->skin_weight, A, vp, verts, vert_transforms);
        else
            hipLaunchKernelGGL(k_lbs_skin_ell<16>, g, dim3(256), 0, s, V, J, sp->skin_k, sp->skin_joint,
                               sp->skin_weight, A, vp, verts, vert_transforms);
    } else {
        hipLaunchKernelGGL(k_lbs_skin, dim3((V + 255) / 256, B), dim3(256), 0, s, V, J, lbs_weights_t, A, vp, verts,
                           vert_transforms);
    }
}
}  // namespace
}  // namespace gsr

// gsr_lbs_sp, or (skin = false) everything up to the skinning: the joint transforms A and v_posed stay
// in the workspace (lbs_skin_splice reads them)
int gsr::lbs_run(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride,
                 const float* betas, const float* shapedirs_t, const float* pose, int pose2rot,
                 const float* posedirs, const float* J_regressor, const int32_t* parents_host,
                 const float* lbs_weights_t, const float* joints_offset, float* verts,
                 float* joints_transformed, float* joints, float* vert_transforms,
                 float* joint_transforms, float* v_shaped, char* workspace, const GsrLbsSparse* sp,
                 void* stream, bool skin, const Blend1Job* companion, bool* companion_done) {
    if (companion_done) *companion_done = false;
    if (B <= 0 || V <= 0) return api_fail(GSR_ERR_ARG, "gsr_lbs: B and V must be positive");
    if (int rc = check_sparse(sp, J, betas ? NB : 0, V, "gsr_lbs")) return rc;
    if (J < 1 || J > GSR_LBS_MAX_JOINTS) return api_fail(GSR_ERR_ARG, "gsr_lbs: J must be in [1, 64]");
    if (!v_template || !pose || !J_regressor || !parents_host || !lbs_weights_t || (skin && !verts) || !workspace)
        return api_fail(GSR_ERR_ARG, "gsr_lbs: null required pointer");
    if (J > 1 && !posedirs) return api_fail(GSR_ERR_ARG, "gsr_lbs: posedirs is null");
    if (v_template_stride != 0 && v_template_stride != (int64_t)V * 3)
        return api_fail(GSR_ERR_ARG, "gsr_lbs: v_template stride must be 0 or V*3");
    if (betas) {
        if (NB <= 0 || !shapedirs_t) return api_fail(GSR_ERR_ARG, "gsr_lbs: betas need NB > 0 and shapedirs");
    } else {
        NB = 0;
    }
    Parents par;
    if (int rc = make_parents(J, parents_host, &par)) return rc;
    hipStream_t s = (hipStream_t)stream;
    LbsArena a;
    carve_lbs(workspace, B, V, J, NB, &a);
    float* vs = v_shaped ? v_shaped : a.vs;
    float* jr = joints ? joints : a.joints;
    float* A = joint_transforms ? joint_transforms : a.A;
    const int NP = (J - 1) * 9;
    const int M = V * 3;

    if (lbs_blend_lds(NB, NP, kLbsFrames, kLbsSplit) > 160 * 1024) return api_fail(GSR_ERR_ARG, "gsr_lbs: NB + 9(J-1) too large for LDS");
    // single frame on tiled bases: Rodrigues runs inside the blend (pose features) and the chain
    // (rotations), one launch fewer on the per-frame path; otherwise its own launch feeds both
    const bool fused = blend_takes_pose(B, NB, NP, a.vp, sp);
    // more than kLbsFrames frames on tiled bases: the launch before the blend writes the coefficient
    // tiles (pose features, and the caller's row-major betas re-laid) and the chain forms its rotations
    const bool tilec = blend_tiledc_applies(B, NB, NP, a.vp, sp);
    if (tilec) {
        launch_coef_tiles(coef_job(B, J, NB, pose, pose2rot, betas, a, a.beta_tiles), CoefJob{}, s);
        if (int rc = hip_check("lbs_coef_tiles")) return rc;
    } else if (!fused) {
        hipLaunchKernelGGL(k_lbs_rodrigues, dim3((B * J + 255) / 256), dim3(256), 0, s, B, J, pose,
                           pose2rot, a.rot, a.feat);
        if (int rc = hip_check("lbs_rodrigues")) return rc;
    }
    if (tilec) {
        const BlendTJob j = blendt_job(M, NB, NP, v_template, v_template_stride, a.beta_tiles, a.feat_tiles, vs, a.vp, sp);
        launch_blend_tiledc(B, j, nullptr, s);
    } else if (companion && companion_done && blend_tiled1_applies(B, NB, NP, a.vp, sp)) {
        // this blend and the caller's independent one in one launch (k_lbs_blend_tiled1_pair)
        const Blend1Job ja = blend1_job(M, NB, NP, v_template, betas, a.feat, vs, a.vp, sp, fused ? pose : nullptr,
                                        pose2rot);
        const int na = (M + 31) / 32, nb = (companion->M + 31) / 32;
        hipLaunchKernelGGL(k_lbs_blend_tiled1_pair, dim3(na + nb), dim3(256), 0, s, ja, na, *companion);
        *companion_done = true;
    } else {
        launch_blend(B, M, NB, NP, v_template, v_template_stride, betas, shapedirs_t, a.feat, posedirs, vs, a.vp, s,
                     sp, fused ? pose : nullptr, pose2rot);
    }
    if (int rc = hip_check("lbs_blend")) return rc;
    // single frame with the CSR regressor: the joints are regressed inside the chain's workgroup
    // (GSR_CHAIN_JOINTS=0: their own launch, A/B)
    // and on the coefficient-tile path (more than kLbsFrames frames); 1 < B <= kLbsFrames keeps its
    // launches (GSR_CHAIN_BATCH=0: only for single frames, as before, A/B)
    static const bool chain_joints_on = tune_env("GSR_CHAIN_JOINTS", 1) != 0;
    static const bool chain_batch_on = tune_env("GSR_CHAIN_BATCH", 1) != 0;
    ChainJoints cj{};
    if ((B == 1 || (tilec && chain_batch_on)) && sp && sp->jreg_row && chain_joints_on) {
        cj = ChainJoints{sp->jreg_row, sp->jreg_col, sp->jreg_val, vs, joints_offset, jr, V, J};
    } else {
        launch_joints(B, V, J, J_regressor, sp, vs, joints_offset, jr, s);
        if (int rc = hip_check("lbs_joints")) return rc;
    }
    hipLaunchKernelGGL(k_lbs_chain, dim3(B), dim3(16 * GSR_LBS_MAX_JOINTS), 0, s, J, par,
                       (fused || tilec) ? nullptr : a.rot, jr, joints_transformed, A, pose, pose2rot, cj, B,
                       ChainJoints{});
    if (int rc = hip_check("lbs_chain")) return rc;
    if (!skin) return 0;
    launch_skin(B, V, J, lbs_weights_t, sp, A, a.vp, verts, vert_transforms, s);
    return hip_check("lbs_skin");
}

bool gsr::ehm_batch_applies(int B, const GsrLbsSparse* sp_h, const GsrLbsSparse* sp_b, int NBh, int NBb) {
    // GSR_EHM_BATCH=0: the per-call path (lbs_run, blend_joints_run, lbs_skin_splice, gsr_lbs_sp), A/B
    static const bool on = tune_env("GSR_EHM_BATCH", 1) != 0 && tune_env("GSR_CHAIN_JOINTS", 1) != 0 &&
                           tune_env("GSR_CHAIN_BATCH", 1) != 0 && tune_env("GSR_EHM_SKIN_SPLICE", 1) != 0;
    if (!on || !sp_h || !sp_b || NBh <= 0 || NBb <= 0) return false;
    auto ok = [&](const GsrLbsSparse* sp, int NB) {
        return sp->jreg_row && sp->skin_k > 0 && sp->shapedirs_tiled && sp->posedirs_tiled &&
               blend_tiledc_applies(B, NB, 0, nullptr, sp);
    };
    return ok(sp_h, NBh) && ok(sp_b, NBb);
}

size_t gsr::lbs_coef_tile_bytes(int B, int K) { return sizeof(float) * coef_tile_floats(B, K); }

int gsr::ehm_batch_run(int B, const EhmBatchModel& head, const EhmBatchModel& body, float* body_betas_tiles,
                       float* head_joints_t, float* body_vt, float* body_tj, const float* joints_offset,
                       const int32_t* head_index, const float* r_eyelid, const float* l_eyelid,
                       const float* eyelid, const float* head_scale, int hj0, int hj1, int bj0, int bj1,
                       uint32_t* bad_index_flag, float* verts, float* joints_transformed, float* joints,
                       float* vert_transforms, float* joint_transforms, void* stream) {
    const int Vh = head.V, Jh = head.J, Vb = body.V, Jb = body.J;
    if (int rc = check_sparse(head.sp, Jh, head.NB, Vh, "gsr_ehm_forward")) return rc;
    if (int rc = check_sparse(body.sp, Jb, body.NB, Vb, "gsr_ehm_forward")) return rc;
    if (hj0 < 0 || hj1 <= hj0 || hj1 > Jh || bj0 < 0 || bj1 <= bj0 || bj1 > Jb)
        return api_fail(GSR_ERR_ARG, "gsr_ehm_forward: bad reference joint ranges");
    if (eyelid && (!r_eyelid || !l_eyelid)) return api_fail(GSR_ERR_ARG, "gsr_ehm_forward: eyelid bases missing");
    Parents par_h, par_b;
    if (int rc = make_parents(Jh, head.parents_host, &par_h)) return rc;
    if (int rc = make_parents(Jb, body.parents_host, &par_b)) return rc;
    hipStream_t s = (hipStream_t)stream;
    LbsArena ah, ab;
    carve_lbs(head.ws, B, Vh, Jh, head.NB, &ah);
    carve_lbs(body.ws, B, Vb, Jb, 0, &ab);
    const int NPh = 9 * (Jh - 1), NPb = 9 * (Jb - 1);
    float* jb = joints ? joints : ab.joints;
    float* Ab = joint_transforms ? joint_transforms : ab.A;
    // 2. the coefficient tiles of both models: FLAME betas + pose features, body betas + pose features
    launch_coef_tiles(coef_job(B, Jh, head.NB, head.pose, 1, head.betas, ah, ah.beta_tiles),
                      coef_job(B, Jb, body.NB, body.pose, 1, body.betas, ab, body_betas_tiles), s);
    if (int rc = hip_check("ehm_coef_tiles")) return rc;
    // 3. FLAME shape + pose blend beside the body template's shape blend
    const BlendTJob jh = blendt_job(Vh * 3, head.NB, NPh, head.v_template, head.vt_stride, ah.beta_tiles,
                                    ah.feat_tiles, ah.vs, ah.vp, head.sp);
    const BlendTJob jt = blendt_job(Vb * 3, body.NB, 0, body.v_template, body.vt_stride, body_betas_tiles, nullptr,
                                    body_vt, nullptr, body.sp);
    static const bool pair_on = tune_env("GSR_EHM_BATCH_PAIR", 1) != 0;  // 0: two launches (A/B)
    if (pair_on) {
        launch_blend_tiledc(B, jh, &jt, s);
    } else {
        launch_blend_tiledc(B, jh, nullptr, s);
        launch_blend_tiledc(B, jt, nullptr, s);
    }
    if (int rc = hip_check("ehm_blend_pair")) return rc;
    // 4. FLAME chain with its joints; further workgroups regress the unspliced body template's joints
    const ChainJoints cjh{head.sp->jreg_row, head.sp->jreg_col, head.sp->jreg_val, ah.vs, nullptr, ah.joints, Vh, Jh};
    const ChainJoints cjt{body.sp->jreg_row, body.sp->jreg_col, body.sp->jreg_val, body_vt, joints_offset, body_tj,
                          Vb, Jb};
    hipLaunchKernelGGL(k_lbs_chain, dim3(2 * B), dim3(16 * GSR_LBS_MAX_JOINTS), 0, s, Jh, par_h, nullptr, ah.joints,
                       head_joints_t, ah.A, head.pose, 1, cjh, B, cjt);
    if (int rc = hip_check("ehm_head_chain")) return rc;
    // 5. head skinning + splice into the body template
    if (int rc = lbs_skin_splice(B, Vh, Jh, head.sp, head.ws, Vb, head_index, r_eyelid, l_eyelid, eyelid, head_scale,
                                 head_joints_t, hj0, hj1, body_tj, Jb, bj0, bj1, body_vt, bad_index_flag, stream))
        return rc;
    // 6. body pose blend (lbs_wobeta: v_shaped is the spliced template)
    const BlendTJob jp = blendt_job(Vb * 3, 0, NPb, body_vt, (int64_t)Vb * 3, nullptr, ab.feat_tiles, ab.vs, ab.vp,
                                    body.sp);
    launch_blend_tiledc(B, jp, nullptr, s);
    if (int rc = hip_check("ehm_body_blend")) return rc;
    // 7. body chain with its joints
    const ChainJoints cjb{body.sp->jreg_row, body.sp->jreg_col, body.sp->jreg_val, ab.vs, joints_offset, jb, Vb, Jb};
    hipLaunchKernelGGL(k_lbs_chain, dim3(B), dim3(16 * GSR_LBS_MAX_JOINTS), 0, s, Jb, par_b, nullptr, jb,
                       joints_transformed, Ab, body.pose, 1, cjb, B, ChainJoints{});
    if (int rc = hip_check("ehm_body_chain")) return rc;
    // 8. skin
    launch_skin(B, Vb, Jb, nullptr, body.sp, Ab, ab.vp, verts, vert_transforms, s);
    return hip_check("lbs_skin");
}

// The FLAME head's skinning fused into the splice (EHM.py:67-75, :121-124): per head vertex, the ELL
// skinning of k_lbs_skin_ell (the same fmaf chains and vertex expression, so the same head vertex),
// then k_splice_head's eyelids, head scale and re-anchoring, written straight into the body template:
// the head vertices never reach memory and one launch goes.
template <int KMAX>
__global__ __launch_bounds__(256) void k_skin_splice(int Vh, int Jh, int K, const int32_t* __restrict__ sj,
                                                     const float* __restrict__ sw, const float* __restrict__ A,
                                                     const float* __restrict__ v_posed, int Vb,
                                                     const int32_t* __restrict__ idx,
                                                     const float* __restrict__ r_eyelid,
                                                     const float* __restrict__ l_eyelid,
                                                     const float* __restrict__ eyelid,
                                                     const float* __restrict__ head_scale,
                                                     const float* __restrict__ hjoints, int hj0, int hj1,
                                                     const float* __restrict__ bjoints, int Jb, int bj0, int bj1,
                                                     float* __restrict__ body, uint32_t* __restrict__ bad) {
    __shared__ float As[GSR_LBS_MAX_JOINTS * 16];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < Jh * 16; i += blockDim.x) As[i] = A[(int64_t)b * Jh * 16 + i];
    __syncthreads();
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Vh) return;
    const int d = idx[v];
    if (d < 0 || d >= Vb) {
        if (bad) atomicOr(bad, 2u);
        return;
    }
    int jj[KMAX];
    float ww[KMAX];
#pragma unroll
    for (int u = 0; u < KMAX; u++) {
        jj[u] = u < K ? min((int)sj[(int64_t)u * Vh + v], Jh - 1) : 0;
        ww[u] = u < K ? sw[(int64_t)u * Vh + v] : 0.f;
    }
    float T[16];
#pragma unroll
    for (int e = 0; e < 16; e++) T[e] = 0.f;
#pragma unroll
    for (int u = 0; u < KMAX; u++) {
        if (u >= K) break;
        const float* Aj = As + 16 * jj[u];
#pragma unroll
        for (int e = 0; e < 16; e++) T[e] = fmaf(ww[u], Aj[e], T[e]);
    }
    const float* vp = v_posed + ((int64_t)b * Vh + v) * 3;
    const float px = vp[0], py = vp[1], pz = vp[2];
    const float* hjb = hjoints + (int64_t)b * Jh * 3;
    const float* bjt = bjoints + (int64_t)b * Jb * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float h = T[4 * c] * px + T[4 * c + 1] * py + T[4 * c + 2] * pz + T[4 * c + 3] * 1.0f;
        if (eyelid) {
            h = h + r_eyelid[3 * v + c] * eyelid[2 * b + 1];
            h = h + l_eyelid[3 * v + c] * eyelid[2 * b];
        }
        if (head_scale) h = h * head_scale[3 * b + c];
        float hs = 0.f, bs = 0.f;
        for (int j = hj0; j < hj1; j++) hs += hjb[3 * j + c];
        for (int j = bj0; j < bj1; j++) bs += bjt[3 * j + c];
        body[((int64_t)b * Vb + d) * 3 + c] = (h - hs / (float)(hj1 - hj0)) + bs / (float)(bj1 - bj0);
    }
}

// the launch for gsr_ehm_forward: A and v_posed from the head's lbs workspace (lbs_run(skin = false));
// returns 1 (nothing launched) when the head has no ELL skinning weights
int gsr::lbs_skin_splice(int B, int Vh, int Jh, const GsrLbsSparse* sp_h, const char* ws_h, int Vb,
                         const int32_t* head_index, const float* r_eyelid, const float* l_eyelid,
                         const float* eyelid, const float* head_scale, const float* head_joints, int hj0, int hj1,
                         const float* body_joints, int Jb, int bj0, int bj1, float* body_v_shaped,
                         uint32_t* bad_index_flag, void* stream) {
    if (!sp_h || sp_h->skin_k <= 0) return 1;
    if (hj0 < 0 || hj1 <= hj0 || hj1 > Jh || bj0 < 0 || bj1 <= bj0 || bj1 > Jb)
        return api_fail(GSR_ERR_ARG, "gsr_ehm_forward: bad reference joint ranges");
    if (eyelid && (!r_eyelid || !l_eyelid)) return api_fail(GSR_ERR_ARG, "gsr_ehm_forward: eyelid bases missing");
    LbsArena a;
    carve_lbs(const_cast<char*>(ws_h), B, Vh, Jh, 0, &a);
    const dim3 g((Vh + 255) / 256, B);
    hipStream_t s = (hipStream_t)stream;
#define GSR_SKS(KM)                                                                                              \
    hipLaunchKernelGGL(k_skin_splice<KM>, g, dim3(256), 0, s, Vh, Jh, sp_h->skin_k, sp_h->skin_joint,            \
                       sp_h->skin_weight, a.A, a.vp, Vb, head_index, r_eyelid, l_eyelid, eyelid, head_scale,     \
                       head_joints, hj0, hj1, body_joints, Jb, bj0, bj1, body_v_shaped, bad_index_flag)
    if (sp_h->skin_k <= 4) GSR_SKS(4);
    else if (sp_h->skin_k <= 8) GSR_SKS(8);
    else GSR_SKS(16);
#undef GSR_SKS
    return hip_check("skin_splice");
}

extern "C" {

int gsr_blend_joints(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride,
                     const float* betas, const float* shapedirs_t, const float* J_regressor,
                     const float* joints_offset, float* v_shaped, float* joints, void* stream) {
    return gsr_blend_joints_sp(B, V, J, NB, v_template, v_template_stride, betas, shapedirs_t, J_regressor,
                               joints_offset, v_shaped, joints, nullptr, stream);
}

int gsr_blend_joints_sp(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride,
                        const float* betas, const float* shapedirs_t, const float* J_regressor,
                        const float* joints_offset, float* v_shaped, float* joints, const GsrLbsSparse* sp,
                        void* stream) {
    return gsr::blend_joints_run(B, V, J, NB, v_template, v_template_stride, betas, shapedirs_t, J_regressor,
                                 joints_offset, v_shaped, joints, sp, stream, false);
}

}  // extern "C"

// gsr_blend_joints_sp; blend_done: the blend shapes were launched already (k_lbs_blend_tiled1_pair)
int gsr::blend_joints_run(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride,
                          const float* betas, const float* shapedirs_t, const float* J_regressor,
                          const float* joints_offset, float* v_shaped, float* joints, const GsrLbsSparse* sp,
                          void* stream, bool blend_done) {
    if (B <= 0 || V <= 0 || J < 1) return api_fail(GSR_ERR_ARG, "gsr_blend_joints: bad sizes");
    if (int rc = check_sparse(sp, 1, betas ? NB : 0, V, "gsr_blend_joints")) return rc;
    if (!v_template || !J_regressor || !v_shaped || !joints)
        return api_fail(GSR_ERR_ARG, "gsr_blend_joints: null required pointer");
    if (v_template_stride != 0 && v_template_stride != (int64_t)V * 3)
        return api_fail(GSR_ERR_ARG, "gsr_blend_joints: v_template stride must be 0 or V*3");
    if (betas && (NB <= 0 || !shapedirs_t))
        return api_fail(GSR_ERR_ARG, "gsr_blend_joints: betas need NB > 0 and shapedirs");
    if (!betas) NB = 0;
    if (lbs_blend_lds(NB, 0, kLbsFrames, kLbsSplit) > 160 * 1024) return api_fail(GSR_ERR_ARG, "gsr_blend_joints: NB too large for LDS");
    hipStream_t s = (hipStream_t)stream;
    const int M = V * 3;
    if (!blend_done) {
        launch_blend(B, M, NB, 0, v_template, v_template_stride, betas, shapedirs_t, nullptr, nullptr, v_shaped, nullptr,
                     s, sp);
        if (int rc = hip_check("blend_shapes")) return rc;
    }
    launch_joints(B, V, J, J_regressor, sp, v_shaped, joints_offset, joints, s);
    return hip_check("vertices2joints");
}

extern "C" {

size_t gsr_lbs_tiled_floats(int K, int M) {
    if (K <= 0 || M <= 0) return 0;
    return (size_t)((M + 31) / 32) * (size_t)((K + 7) / 8) * 256;
}

int gsr_lbs_tile_bases(int K, int M, const float* base, float* tiled, void* stream) {
    if (K <= 0 || M <= 0 || !base || !tiled) return api_fail(GSR_ERR_ARG, "gsr_lbs_tile_bases: bad arguments");
    if (((uintptr_t)tiled & 15) != 0) return api_fail(GSR_ERR_ARG, "gsr_lbs_tile_bases: tiled must be 16-byte aligned");
    const int64_t n4 = (int64_t)gsr_lbs_tiled_floats(K, M) / 4;
    hipLaunchKernelGGL(k_lbs_tile_base, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, K, M,
                       n4, base, reinterpret_cast<float4*>(tiled));
    return hip_check("lbs_tile_base");
}

int gsr_splice_head(int B, int V_body, int N_head, const int32_t* head_index, const float* head_verts,
                    const float* r_eyelid, const float* l_eyelid, const float* eyelid_params,
                    const float* head_scale, const float* head_joints, int J_head, int hj0, int hj1,
                    const float* body_joints, int J_body, int bj0, int bj1, float* body_v_shaped,
                    uint32_t* bad_index_flag, void* stream) {
    if (B <= 0 || V_body <= 0 || N_head < 0) return api_fail(GSR_ERR_ARG, "gsr_splice_head: bad sizes");
    if (N_head == 0) return 0;
    if (!head_index || !head_verts || !head_joints || !body_joints || !body_v_shaped)
        return api_fail(GSR_ERR_ARG, "gsr_splice_head: null required pointer");
    if (eyelid_params && (!r_eyelid || !l_eyelid))
        return api_fail(GSR_ERR_ARG, "gsr_splice_head: eyelid_params need both eyelid bases");
    if (hj0 < 0 || hj1 <= hj0 || hj1 > J_head || bj0 < 0 || bj1 <= bj0 || bj1 > J_body)
        return api_fail(GSR_ERR_ARG, "gsr_splice_head: bad reference joint ranges");
    hipLaunchKernelGGL(k_splice_head, dim3((N_head + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,
                       V_body, N_head, head_index, head_verts, r_eyelid, l_eyelid, eyelid_params,
                       head_scale, head_joints, J_head, hj0, hj1, body_joints, J_body, bj0, bj1,
                       body_v_shaped, bad_index_flag);
    return hip_check("splice_head");
}

int gsr_pack_rows(int B, int nseg, const GsrRowSegment* segs, void* stream) {
    if (B <= 0 || nseg < 0 || nseg > GSR_PACK_MAX_SEGMENTS) return api_fail(GSR_ERR_ARG, "gsr_pack_rows: bad sizes");
    if (nseg == 0) return 0;
    if (!segs) return api_fail(GSR_ERR_ARG, "gsr_pack_rows: null segment table");
    PackTable t;
    for (int i = 0; i < nseg; i++) {
        t.seg[i] = segs[i];
        if (!segs[i].dst || segs[i].width < 0 || segs[i].width > 4096 || segs[i].dst_stride < segs[i].width ||
            segs[i].src_stride < 0)
            return api_fail(GSR_ERR_ARG, "gsr_pack_rows: bad segment");
    }
    hipLaunchKernelGGL(k_pack_rows, dim3(nseg, B), dim3(256), 0, (hipStream_t)stream, t);
    return hip_check("pack_rows");
}

int gsr_deform_gaussians(int B, int V, int F, int N, const float* verts,
                         const float* vert_transforms, const int32_t* faces,
                         const float* vtx_rotations, int64_t vtx_rot_stride,
                         const float* vtx_scales, int64_t vtx_scale_stride,
                         const int32_t* binding_face, const float* face_bary,
                         const float* local_xyz, int64_t local_stride,
                         const float* uv_rotations, int64_t uv_rot_stride,
                         const float* uv_scales, int64_t uv_scale_stride, float* means3D,
                         float* rotations, float* scales, uint32_t* bad_index_flag, void* stream) {
    if (B <= 0 || V < 0 || N < 0 || F < 0) return api_fail(GSR_ERR_ARG, "gsr_deform_gaussians: bad sizes");
    if (V + N == 0) return 0;
    if (!verts || !means3D || !rotations || !scales)
        return api_fail(GSR_ERR_ARG, "gsr_deform_gaussians: null required pointer");
    if (V > 0 && (!vert_transforms || !vtx_rotations || !vtx_scales))
        return api_fail(GSR_ERR_ARG, "gsr_deform_gaussians: vertex Gaussians need transforms, rotations, scales");
    if (N > 0 && (!faces || !binding_face || !face_bary || !local_xyz || !uv_rotations || !uv_scales || F == 0))
        return api_fail(GSR_ERR_ARG, "gsr_deform_gaussians: UV Gaussians need faces and binding data");
    auto bad_stride = [](int64_t st, int64_t full) { return st != 0 && st != full; };
    if (bad_stride(vtx_rot_stride, 4LL * V) || bad_stride(vtx_scale_stride, 3LL * V) ||
        bad_stride(local_stride, 3LL * N) || bad_stride(uv_rot_stride, 4LL * N) ||
        bad_stride(uv_scale_stride, 3LL * N))
        return api_fail(GSR_ERR_ARG, "gsr_deform_gaussians: strides must be 0 or a whole frame");
    hipStream_t s = (hipStream_t)stream;
    static const int fpw = [] {
        const int v = tune_env("GSR_DEFORM_FRAMES", kDeformFrames);
        return v >= 1 && v <= 64 ? v : 1;
    }();
    const int P = V + N;
    hipLaunchKernelGGL(k_deform_gaussians, dim3((P + 255) / 256, (B + fpw - 1) / fpw), dim3(256), 0, s, B, fpw,
                       V, F, N, verts, vert_transforms, faces, vtx_rotations, vtx_rot_stride, vtx_scales,
                       vtx_scale_stride, binding_face, face_bary, local_xyz, local_stride, uv_rotations,
                       uv_rot_stride, uv_scales, uv_scale_stride, means3D, rotations, scales,
                       bad_index_flag);
    return hip_check("deform_gaussians");
}

int gsr_deform_gaussians_backward(int B, const GsrDeformInputs* dg, const float* dL_dmeans3D,
                                  const float* dL_drotations, const float* dL_dscales,
                                  const GsrDeformGrads* grads, void* stream) {
    const char* who = "gsr_deform_gaussians_backward";
    if (const int rc = check_deform_inputs(B, dg, who)) return rc;
    if (!grads) return api_fail(GSR_ERR_ARG, "gsr_deform_gaussians_backward: null gradient struct");
    const int P = dg->V + dg->N;
    if (P == 0) return 0;
    GsrDeformGrads o = *grads;
    if (dg->V == 0) o.vtx_rotations = o.vtx_scales = nullptr;
    if (dg->N == 0) o.local_xyz = o.uv_rotations = o.uv_scales = nullptr;
    if (!o.vtx_rotations && !o.vtx_scales && !o.local_xyz && !o.uv_rotations && !o.uv_scales) return 0;
    if (((o.vtx_rotations || o.uv_rotations) && !dL_drotations) || ((o.vtx_scales || o.uv_scales) && !dL_dscales) ||
        (o.local_xyz && !dL_dmeans3D))
        return api_fail(GSR_ERR_ARG, "gsr_deform_gaussians_backward: a wanted gradient needs its upstream gradient");
    // a wanted output shared by every frame is a sum over all B frames in one thread (grid.y = 1);
    // with per-frame outputs only, the frames are grouped per workgroup as in the forward
    const bool any_shared = (o.vtx_rotations && !dg->vtx_rot_stride) || (o.vtx_scales && !dg->vtx_scale_stride) ||
                            (o.local_xyz && !dg->local_stride) || (o.uv_rotations && !dg->uv_rot_stride) ||
                            (o.uv_scales && !dg->uv_scale_stride);
    const int fpw = any_shared || B < kDeformFrames ? B : kDeformFrames;
    hipLaunchKernelGGL(k_deform_gaussians_bwd, dim3((P + 255) / 256, (B + fpw - 1) / fpw), dim3(256), 0,
                       (hipStream_t)stream, B, fpw, *dg, dL_dmeans3D, dL_drotations, dL_dscales, o);
    return hip_check("deform_gaussians_backward");
}

}  // extern "C"
