// lift.hip -- image-to-avatar feature lifting (include/gsr_lift.h) for gfx950: the projection gathers of
// the reference's Ubody_Gaussian_inferer (sample_prj_feature, convert_pixel_feature_to_uv,
// models/UbodyAvatar/ubody_gaussian.py:75-114) and their gradients with respect to the feature map.
// The per-sample arithmetic (projection, guards, taps) is lift_dev.h's, shared with the host check.
//
//   k_lift_uv        one lane per (frame, texel) and chunk of kUvChunk channels: the geometry once, then
//                    the channel loop; neighbouring texels hit neighbouring pixels and the stores are
//                    coalesced per channel plane.  Every out element is written exactly once.
//   k_lift_vertices  a workgroup per 64 vertices and chunk of 32 channels.  The input is planar and the
//                    output channel-contiguous: lanes over vertices gather (wave w the channels
//                    w, w + 4, ...) into an LDS tile, then lanes over channels store 128-byte runs.
//   k_lift_bwd       the scatter-add.  A lane-per-sample atomic into the planar [B,C,H,W] layout puts 64
//                    lanes in 64 rows, the slow shape of this chip's float atomics
//                    (MI355X_MICROARCH.md "Global float atomics").  Instead the sums go to a zeroed
//                    channels-last scratch [B,H,W,C]: each wave computes the geometry of 64 samples (one
//                    per lane), then walks its live samples with the lanes over the 2C contiguous floats of
//                    a tap row (taps x0 and x0 + 1 are neighbours in that layout).
//   k_lift_transpose scratch [B,H*W,C] -> dfeat [B,C,H*W] through an LDS tile; dfeat is overwritten in full.
#include <hip/hip_runtime.h>

#include "../../include/gsr.h"
#include "../../include/gsr_lift.h"
#include "gsr_internal.h"
#include "lift_dev.h"

namespace gsr {

constexpr int kUvChunk = 8;    // channels per k_lift_uv lane
constexpr int kVtxChunk = 32;  // channels per k_lift_vertices workgroup
constexpr int kVtxTile = 64;   // vertices per k_lift_vertices workgroup

struct LiftArgs {
    int B, V, F, T, C, W, H;
    const float* verts;
    const int32_t* faces;
    const int32_t* texel_face;
    const float* texel_bary;
    const float* w2c;
    const float* tanfovx;
    const float* tanfovy;
    const uint8_t* face_visible;
};

template <bool UV>
__device__ __forceinline__ LiftSample sample_of(const LiftArgs& a, int b, int n, float& xn, float& yn) {
    const float* M = a.w2c + 16 * (int64_t)b;
    const float* vb = a.verts + 3 * (int64_t)b * a.V;
    if (UV) {
        xn = yn = 0.f;
        return lift_uv_sample(vb, a.faces, a.texel_face, a.texel_bary,
                              a.face_visible ? a.face_visible + (int64_t)b * a.F : nullptr, M, a.tanfovx[b],
                              a.tanfovy[b], a.V, a.F, a.W, a.H, n);
    }
    return lift_vertex_sample(vb + 3 * (int64_t)n, M, a.tanfovx[b], a.tanfovy[b], a.W, a.H, xn, yn);
}

__global__ void __launch_bounds__(256) k_lift_uv(LiftArgs a, unsigned nblk, const float* __restrict__ feat,
                                                 float* __restrict__ out) {
    const unsigned chunk = blockIdx.x / nblk;
    const int64_t i = (int64_t)(blockIdx.x - chunk * nblk) * 256 + threadIdx.x;
    if (i >= (int64_t)a.B * a.T) return;
    const int b = (int)(i / a.T), t = (int)(i - (int64_t)b * a.T);
    float xn, yn;
    const LiftSample s = sample_of<true>(a, b, t, xn, yn);
    const int c0 = (int)chunk * kUvChunk;
    const int64_t HW = (int64_t)a.H * a.W;
#pragma unroll
    for (int k = 0; k < kUvChunk; ++k) {
        const int c = c0 + k;
        if (c >= a.C) break;
        const int64_t plane = (int64_t)b * a.C + c;
        out[plane * a.T + t] = s.mask ? lift_sample_plane(s, feat + plane * HW, a.W) : 0.0f;
    }
}

__global__ void __launch_bounds__(256) k_lift_vertices(LiftArgs a, unsigned ntile, unsigned nchunk,
                                                       const float* __restrict__ feat, float* __restrict__ out,
                                                       float* __restrict__ ndc) {
    __shared__ float tile[kVtxTile][kVtxChunk + 1];
    unsigned blk = blockIdx.x;
    const unsigned chunk = blk % nchunk;
    blk /= nchunk;
    const unsigned vt = blk % ntile;
    const int b = (int)(blk / ntile);
    const int v0 = (int)vt * kVtxTile, c0 = (int)chunk * kVtxChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int v = v0 + lane;
    if (v < a.V) {
        float xn, yn;
        const LiftSample s = sample_of<false>(a, b, v, xn, yn);
        if (ndc && chunk == 0 && wave == 0) {
            ndc[2 * ((int64_t)b * a.V + v)] = xn;
            ndc[2 * ((int64_t)b * a.V + v) + 1] = yn;
        }
        const int64_t HW = (int64_t)a.H * a.W;
#pragma unroll
        for (int k = 0; k < kVtxChunk / 4; ++k) {
            const int cl = wave + 4 * k, c = c0 + cl;
            if (c < a.C) tile[lane][cl] = s.mask ? lift_sample_plane(s, feat + ((int64_t)b * a.C + c) * HW, a.W) : 0.0f;
        }
    }
    __syncthreads();
    const int cl = threadIdx.x & (kVtxChunk - 1);
    for (int r = threadIdx.x / kVtxChunk; r < kVtxTile; r += 256 / kVtxChunk)
        if (v0 + r < a.V && c0 + cl < a.C) out[((int64_t)b * a.V + v0 + r) * a.C + c0 + cl] = tile[r][cl];
}

// dout element (sample n of frame b, channel c): UV [B,C,T], vertices [B,V,C]
template <bool UV>
__global__ void __launch_bounds__(256) k_lift_bwd(LiftArgs a, const float* __restrict__ dout, float* __restrict__ acc) {
    const int N = UV ? a.T : a.V;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < (int64_t)a.B * N;
    const int b = live ? (int)(i / N) : 0;
    const int n = live ? (int)(i - (int64_t)b * N) : 0;
    LiftSample s;
    s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
    s.x0 = s.y0 = 0;
    s.mask = 0u;
    if (live) {
        float xn, yn;
        s = sample_of<UV>(a, b, n, xn, yn);
    }
    const int lane = threadIdx.x & 63;
    const int64_t C = a.C;
    unsigned long long m = __ballot(s.mask != 0u);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const int sb = __shfl(b, src), sn = __shfl(n, src);
        const int x0 = __shfl(s.x0, src), y0 = __shfl(s.y0, src);
        const unsigned mask = (unsigned)__shfl((int)s.mask, src);
        const float w0 = __shfl(s.w[0], src), w1 = __shfl(s.w[1], src);
        const float w2 = __shfl(s.w[2], src), w3 = __shfl(s.w[3], src);
        const float* d = UV ? dout + (int64_t)sb * C * a.T + sn : dout + ((int64_t)sb * a.V + sn) * C;
        const int64_t dstride = UV ? a.T : 1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned rm = (mask >> (2 * r)) & 3u;  // this row's two taps
            if (!rm) continue;
            // element offset of (b, y0 + r, x0, channel 0): x0 may be -1, the masked tap is never touched
            const int64_t row = (((int64_t)sb * a.H + (y0 + r)) * a.W + x0) * C;
            const float wa = r ? w2 : w0, wb = r ? w3 : w1;
            for (int64_t j = lane; j < 2 * C; j += 64) {
                const bool second = j >= C;
                const int64_t c = second ? j - C : j;
                if ((rm >> (second ? 1 : 0)) & 1u) unsafeAtomicAdd(acc + row + j, (second ? wb : wa) * d[c * dstride]);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_lift_transpose(int C, int64_t HW, unsigned npt, unsigned nct,
                                                        const float* __restrict__ acc, float* __restrict__ dfeat) {
    __shared__ float tile[64][33];
    unsigned blk = blockIdx.x;
    const unsigned ct = blk % nct;
    blk /= nct;
    const unsigned pt = blk % npt;
    const int64_t b = blk / npt;
    const int c0 = (int)ct * 32;
    const int64_t p0 = (int64_t)pt * 64;
    {
        const int c = threadIdx.x & 31;
        for (int p = threadIdx.x >> 5; p < 64; p += 8)
            if (p0 + p < HW && c0 + c < C) tile[p][c] = acc[(b * HW + p0 + p) * C + c0 + c];
    }
    __syncthreads();
    const int px = threadIdx.x & 63;
    for (int c = threadIdx.x >> 6; c < 32; c += 4)
        if (p0 + px < HW && c0 + c < C) dfeat[(b * C + c0 + c) * HW + p0 + px] = tile[px][c];
}

static bool lift_sizes_ok(int B, int N, int C, int W, int H) {
    if (B <= 0 || N <= 0 || C <= 0 || W <= 0 || H <= 0 || W > 16384 || H > 16384) return false;
    const int64_t lim = (int64_t)1 << 31;
    return (int64_t)B * C * H * W < lim && (int64_t)B * N * C < lim && (int64_t)B * N < lim;
}

static inline size_t lift_up256(size_t n) { return (n + 255) & ~(size_t)255; }

static unsigned lift_blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

static int lift_done() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

// zeroes the scratch, scatters, transposes into dfeat
template <bool UV>
static int lift_backward(const LiftArgs& a, const float* dout, float* dfeat, void* workspace, hipStream_t s) {
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t N = UV ? a.T : a.V;
    float* acc = (float*)workspace;
    hipError_t e = hipMemsetAsync(acc, 0, (size_t)a.B * a.C * HW * sizeof(float), s);
    if (e != hipSuccess) return api_fail(GSR_ERR_HIP, hipGetErrorString(e));
    hipLaunchKernelGGL(k_lift_bwd<UV>, dim3(lift_blocks256((int64_t)a.B * N)), dim3(256), 0, s, a, dout, acc);
    const unsigned npt = (unsigned)((HW + 63) / 64), nct = (unsigned)((a.C + 31) / 32);
    hipLaunchKernelGGL(k_lift_transpose, dim3((unsigned)((int64_t)a.B * npt * nct)), dim3(256), 0, s, a.C, HW, npt, nct,
                       acc, dfeat);
    return lift_done();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_lift_vertices(int B, int V, int C, int W, int H, const float* verts, const float* w2c, const float* tanfovx,
                      const float* tanfovy, const float* feat, float* out, float* ndc, void* stream) {
    if (!lift_sizes_ok(B, V, C, W, H)) return api_fail(GSR_ERR_ARG, "gsr_lift_vertices: bad sizes");
    if (!verts || !w2c || !tanfovx || !tanfovy || !feat || !out)
        return api_fail(GSR_ERR_ARG, "gsr_lift_vertices: null required pointer");
    const LiftArgs a{B, V, 0, 0, C, W, H, verts, nullptr, nullptr, nullptr, w2c, tanfovx, tanfovy, nullptr};
    const unsigned ntile = (unsigned)((V + kVtxTile - 1) / kVtxTile), nchunk = (unsigned)((C + kVtxChunk - 1) / kVtxChunk);
    hipLaunchKernelGGL(k_lift_vertices, dim3((unsigned)((int64_t)B * ntile * nchunk)), dim3(256), 0, (hipStream_t)stream,
                       a, ntile, nchunk, feat, out, ndc);
    return lift_done();
}

int gsr_lift_uv(int B, int V, int F, int T, int C, int W, int H, const float* verts, const int32_t* faces,
                const int32_t* texel_face, const float* texel_bary, const float* w2c, const float* tanfovx,
                const float* tanfovy, const float* feat, const uint8_t* face_visible, float* out, void* stream) {
    if (!lift_sizes_ok(B, T, C, W, H) || V <= 0 || F <= 0 || (int64_t)B * V >= ((int64_t)1 << 31) ||
        (int64_t)B * F >= ((int64_t)1 << 31))
        return api_fail(GSR_ERR_ARG, "gsr_lift_uv: bad sizes");
    if (!verts || !faces || !texel_face || !texel_bary || !w2c || !tanfovx || !tanfovy || !feat || !out)
        return api_fail(GSR_ERR_ARG, "gsr_lift_uv: null required pointer");
    const LiftArgs a{B, V, F, T, C, W, H, verts, faces, texel_face, texel_bary, w2c, tanfovx, tanfovy, face_visible};
    const unsigned nblk = lift_blocks256((int64_t)B * T), nchunk = (unsigned)((C + kUvChunk - 1) / kUvChunk);
    hipLaunchKernelGGL(k_lift_uv, dim3((unsigned)((int64_t)nblk * nchunk)), dim3(256), 0, (hipStream_t)stream, a, nblk,
                       feat, out);
    return lift_done();
}

size_t gsr_lift_backward_workspace_bytes(int B, int C, int W, int H) {
    if (!lift_sizes_ok(B, 1, C, W, H)) return 0;
    return lift_up256((size_t)B * C * H * W * sizeof(float));
}

int gsr_lift_vertices_backward(int B, int V, int C, int W, int H, const float* verts, const float* w2c,
                               const float* tanfovx, const float* tanfovy, const float* dout, float* dfeat,
                               void* workspace, void* stream) {
    if (!lift_sizes_ok(B, V, C, W, H)) return api_fail(GSR_ERR_ARG, "gsr_lift_vertices_backward: bad sizes");
    if (!verts || !w2c || !tanfovx || !tanfovy || !dout || !dfeat || !workspace)
        return api_fail(GSR_ERR_ARG, "gsr_lift_vertices_backward: null required pointer");
    const LiftArgs a{B, V, 0, 0, C, W, H, verts, nullptr, nullptr, nullptr, w2c, tanfovx, tanfovy, nullptr};
    return lift_backward<false>(a, dout, dfeat, workspace, (hipStream_t)stream);
}

int gsr_lift_uv_backward(int B, int V, int F, int T, int C, int W, int H, const float* verts, const int32_t* faces,
                         const int32_t* texel_face, const float* texel_bary, const float* w2c, const float* tanfovx,
                         const float* tanfovy, const uint8_t* face_visible, const float* dout, float* dfeat,
                         void* workspace, void* stream) {
    if (!lift_sizes_ok(B, T, C, W, H) || V <= 0 || F <= 0 || (int64_t)B * V >= ((int64_t)1 << 31) ||
        (int64_t)B * F >= ((int64_t)1 << 31))
        return api_fail(GSR_ERR_ARG, "gsr_lift_uv_backward: bad sizes");
    if (!verts || !faces || !texel_face || !texel_bary || !w2c || !tanfovx || !tanfovy || !dout || !dfeat || !workspace)
        return api_fail(GSR_ERR_ARG, "gsr_lift_uv_backward: null required pointer");
    const LiftArgs a{B, V, F, T, C, W, H, verts, faces, texel_face, texel_bary, w2c, tanfovx, tanfovy, face_visible};
    return lift_backward<true>(a, dout, dfeat, workspace, (hipStream_t)stream);
}

}  // extern "C"
