// refiner_bwd.hip -- the backward of the refiner decoder's glue (include/gsr_refiner.h) for gfx950: one
// fused pass in front of each conv's backward and one behind it, with the per-plane reductions that give
// the gradients of s, d, the biases, the noise weight and the ToRGB weight folded into them.  The
// arithmetic is refiner_dev.h's, shared with the host check (tools/refiner_bwd_check.cpp).
//
// No atomics.  Every reduction over pixels has one fixed shape: a plane is cut into chunks of
// kRfChunkQuads = 256 lane-quads (a function of H and W alone), a workgroup of 4 waves owns one chunk,
//   lane   (t0 + t1) + (t2 + t3) over its four pixels (a lane past the plane's end adds +0)
//   wave   v = v + shfl_xor(v, m), m = 32, 16, 8, 4, 2, 1
//   chunk  ((w0 + w1) + w2) + w3 over the four waves, through LDS
// and the chunk sums go to a workspace.  A finishing kernel sums a plane's chunks: lane k of a wave adds
// chunks k, k + 64, ... in ascending order from +0, then the same butterfly.  So two runs give the same
// bits whatever grid the hardware schedules.
//
//   k_style_epilogue_bwd    a lane per 4 pixels: g_x, g_scale, g_shift, 4 chunk sums per workgroup (the noise
//                           weight's in float64, the same tree)
//   k_style_epilogue_finish one workgroup: plane sums -> g_d, g_post; then g_bias (b ascending), g_noise_weight
//   k_style_upmod_bwd       a lane per 4 output pixels (the g_s term) and per input pixel (g_x = s * up2T(g_y))
//   k_style_sum_finish      a wave per plane: g_s
//   k_style_torgb_bwd<O>    a lane per 4 pixels: g_acc, g_x for every channel, g_skip, O*C + O chunk sums
//   k_style_torgb_finish    a wave per channel: m[b,o,c] -> g_weight, g_s; one more wave: g_bias
//   k_style_coeffs_bwd      a workgroup per (layer, frame): g_s += ...; 8 more per layer: g_w2
#include <hip/hip_runtime.h>

#include "../../include/gsr.h"
#include "../../include/gsr_refiner.h"
#include "gsr_internal.h"
#include "refiner_dev.h"

#pragma clang fp contract(off)

namespace gsr {

constexpr int kRbBlock = kRfChunkQuads;  // a quad per lane
constexpr int kRbWaves = kRbBlock / 64;
constexpr int kRbFinishBlock = 1024;
constexpr int kRbCoeffBlock = kRfMaxChannels;

struct RbLayers {
    GsrStyleLayer l[kRfMaxLayers];
};

__device__ __forceinline__ float rb_wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

// the sum of n values p[k * stride], k ascending per lane, by one wave; every lane returns it
__device__ __forceinline__ float rb_strided_sum(const float* p, int64_t n, int64_t stride, int lane) {
    float acc = 0.0f;
    for (int64_t k = lane; k < n; k += 64) acc = acc + p[k * stride];
    return rb_wave_sum(acc);
}

__device__ __forceinline__ double rb_wave_sum(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double rb_strided_sum(const double* p, int64_t n, int64_t stride, int lane) {
    double acc = 0.0;
    for (int64_t k = lane; k < n; k += 64) acc = acc + p[k * stride];
    return rb_wave_sum(acc);
}

__device__ __forceinline__ RfQuad rb_zero() { return RfQuad{{0.0f, 0.0f, 0.0f, 0.0f}}; }

// the sums of one chunk, and of one plane: 24 bytes, the float64 noise sum on an 8-byte boundary
struct RbEpiSums {
    float sx, sv, sp, pad;
    double sn;
};
static_assert(sizeof(RbEpiSums) == 6 * sizeof(float), "the header states 6 floats per slot");

// ------------------------------------------------------------------ epilogue

__global__ void __launch_bounds__(kRbBlock)
    k_style_epilogue_bwd(int C, int64_t Q, int64_t chunks, const float* __restrict__ g_y, const float* __restrict__ x,
                         const float* __restrict__ d, int64_t d_stride, const float* __restrict__ noise, int noise_batch,
                         const float* __restrict__ noise_weight, const float* __restrict__ bias,
                         const float* __restrict__ scale, const float* __restrict__ shift,
                         const float* __restrict__ post, int64_t post_stride, float* __restrict__ g_x,
                         float* __restrict__ g_scale, float* __restrict__ g_shift, RbEpiSums* __restrict__ partial) {
    __shared__ float ws[kRbWaves][3];
    __shared__ double wn[kRbWaves];
    const int64_t plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const int64_t b = plane / C;
    const int c = (int)(plane - b * C);
    const int64_t q = chunk * kRbBlock + threadIdx.x;
    float t[3] = {0.0f, 0.0f, 0.0f};
    double tn = 0.0;
    if (q < Q) {
        const int64_t e = (plane * Q + q) * 4;
        const float a = d ? kRfSqrt2 * d[b * d_stride + c] : kRfSqrt2;
        const float bc = bias[c];
        const float nw = noise_batch ? noise_weight[0] : 0.0f;
        const float ps = post ? post[b * post_stride + c] : 0.0f;
        const RfQuad gq = rf_load(g_y + e), xq = rf_load(x + e);
        const RfQuad nq = noise_batch ? rf_load(noise + ((noise_batch == 1 ? 0 : b) * Q + q) * 4) : rb_zero();
        const RfQuad sc = scale ? rf_load(scale + e) : rb_zero(), sh = scale ? rf_load(shift + e) : rb_zero();
        RfQuad gx, gsc, gsh, tx, tv, tp;
        double n4[4];
        for (int k = 0; k < 4; ++k) {
            const RfEpiGrad r = rf_epilogue_bwd(gq.v[k], xq.v[k], a, nw, nq.v[k], bc, scale != nullptr, sc.v[k],
                                                sh.v[k], post != nullptr, ps);
            gx.v[k] = r.g_x, gsc.v[k] = r.g_scale, gsh.v[k] = r.g_shift;
            tx.v[k] = r.t_x, tv.v[k] = r.g_v, tp.v[k] = r.t_post;
            n4[k] = rf_noise_term(r.g_v, nq.v[k]);
        }
        rf_store(g_x + e, gx);
        if (scale) {
            rf_store(g_scale + e, gsc);
            rf_store(g_shift + e, gsh);
        }
        t[0] = rf_quad_sum(tx), t[1] = rf_quad_sum(tv), t[2] = rf_quad_sum(tp);
        tn = (n4[0] + n4[1]) + (n4[2] + n4[3]);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < 3; ++k) {
        const float v = rb_wave_sum(t[k]);
        if (lane == 0) ws[wave][k] = v;
    }
    tn = rb_wave_sum(tn);
    if (lane == 0) wn[wave] = tn;
    __syncthreads();
    if (threadIdx.x == 0) {
        RbEpiSums r;
        r.sx = ((ws[0][0] + ws[1][0]) + ws[2][0]) + ws[3][0];
        r.sv = ((ws[0][1] + ws[1][1]) + ws[2][1]) + ws[3][1];
        r.sp = ((ws[0][2] + ws[1][2]) + ws[2][2]) + ws[3][2];
        r.pad = 0.0f;
        r.sn = ((wn[0] + wn[1]) + wn[2]) + wn[3];
        partial[blockIdx.x] = r;
    }
}

// one workgroup.  sums: [planes], written here and read back after the barrier
__global__ void __launch_bounds__(kRbFinishBlock)
    k_style_epilogue_finish(int B, int C, int64_t chunks, const RbEpiSums* __restrict__ partial, RbEpiSums* sums,
                            float* __restrict__ g_d, float* __restrict__ g_post, float* __restrict__ g_bias,
                            float* __restrict__ g_noise_weight) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int waves = kRbFinishBlock / 64;
    const int64_t planes = (int64_t)B * C;
    for (int64_t p = wave; p < planes; p += waves) {
        const RbEpiSums* pp = partial + p * chunks;
        RbEpiSums r;
        r.sx = rb_strided_sum(&pp->sx, chunks, 6, lane);
        r.sv = rb_strided_sum(&pp->sv, chunks, 6, lane);
        r.sp = rb_strided_sum(&pp->sp, chunks, 6, lane);
        r.pad = 0.0f;
        r.sn = rb_strided_sum(&pp->sn, chunks, 3, lane);
        if (lane == 0) {
            sums[p] = r;
            if (g_d) g_d[p] = kRfSqrt2 * r.sx;
            if (g_post) g_post[p] = r.sp;
        }
    }
    __threadfence_block();
    __syncthreads();  // the plane sums, stored by this workgroup's waves, are read back below
    for (int c = threadIdx.x; c < C; c += kRbFinishBlock) {
        float acc = sums[c].sv;
        for (int b = 1; b < B; ++b) acc = acc + sums[(int64_t)b * C + c].sv;
        g_bias[c] = acc;
    }
    if (g_noise_weight && wave == 0) {
        const double v = rb_strided_sum(&sums->sn, planes, 3, lane);
        if (lane == 0) g_noise_weight[0] = (float)v;  // rounded once
    }
}

// ------------------------------------------------------------------ upmod

__global__ void __launch_bounds__(kRbBlock)
    k_style_upmod_bwd(int B, int C, int H, int W, int up, int x_batch, int64_t Q, int64_t chunks,
                      const float* __restrict__ g_y, const float* __restrict__ x, const float* __restrict__ s,
                      int64_t s_stride, float* __restrict__ g_x, float* __restrict__ partial) {
    __shared__ float ws[kRbWaves];
    const int64_t plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const int64_t b = plane / C;
    const int c = (int)(plane - b * C);
    const int64_t q = chunk * kRbBlock + threadIdx.x;
    float t = 0.0f;
    if (q < Q) {
        const float* gp = g_y + plane * Q * 4;
        const RfQuad gq = rf_load(gp + q * 4);
        const float sc = s[b * s_stride + c];
        if (up) {
            // Q output quads of the plane are as many as its input pixels: the lane owns one of each
            const int Hi = H >> 1, Wi = W >> 1;
            const float* xp = x + plane * Q;
            const int r = (int)((q * 4) / W), j0 = (int)(q * 4 - (int64_t)r * W);
            RfQuad u;
            rf_up2_quad(xp, Hi, Wi, r, j0, u.v);
            t = rf_quad_dot(gq, u);
            const int i = (int)(q / Wi), ci = (int)(q - (int64_t)i * Wi);
            g_x[plane * Q + q] = sc * rf_up2t(RfAtPlain{gp, W}, H, W, i, ci);
        } else {
            const int64_t xplane = x_batch == 1 ? c : plane;
            t = rf_quad_dot(gq, rf_load(x + (xplane * Q + q) * 4));
            if (x_batch != 1) {
                RfQuad o;
                for (int k = 0; k < 4; ++k) o.v[k] = sc * gq.v[k];
                rf_store(g_x + (plane * Q + q) * 4, o);
            } else if (b == 0) {  // the broadcast input: its gradient sums the frames, b ascending
                RfQuad o;
                for (int k = 0; k < 4; ++k) o.v[k] = sc * gq.v[k];
                for (int bb = 1; bb < B; ++bb) {
                    const RfQuad gb = rf_load(g_y + (((int64_t)bb * C + c) * Q + q) * 4);
                    const float sb = s[bb * s_stride + c];
                    for (int k = 0; k < 4; ++k) o.v[k] = o.v[k] + sb * gb.v[k];
                }
                rf_store(g_x + ((int64_t)c * Q + q) * 4, o);
            }
        }
    }
    const float v = rb_wave_sum(t);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__global__ void __launch_bounds__(kRbBlock)
    k_style_sum_finish(int64_t planes, int64_t chunks, const float* __restrict__ partial, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kRbWaves + (threadIdx.x >> 6);
    if (p >= planes) return;  // whole waves
    const float v = rb_strided_sum(partial + p * chunks, chunks, 1, lane);
    if (lane == 0) out[p] = v;
}

// ------------------------------------------------------------------ torgb

template <int O>
__global__ void __launch_bounds__(kRbBlock)
    k_style_torgb_bwd(int C, int H, int W, int64_t Q, const float* __restrict__ g_out, const float* __restrict__ y,
                      const float* __restrict__ x, const float* __restrict__ weight, const float* __restrict__ s,
                      int64_t s_stride, int skip_up, float* __restrict__ g_x, float* __restrict__ g_skip,
                      float* __restrict__ partial) {
    __shared__ float wm[O * kRfMaxChannels];
    __shared__ float ws[kRbWaves][O * kRfMaxChannels + O];
    const int64_t b = blockIdx.y, chunks = gridDim.x;
    for (int i = threadIdx.x; i < O * C; i += kRbBlock) wm[i] = weight[i] * s[b * s_stride + (i % C)];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    const bool live = q < Q;
    RfQuad g[O];
    for (int o = 0; o < O; ++o) {
        g[o] = rb_zero();
        if (live) {
            const int64_t e = ((b * O + o) * Q + q) * 4;
            g[o] = rf_load(g_out + e);
            if (y) {
                const RfQuad yq = rf_load(y + e);
                for (int k = 0; k < 4; ++k) g[o].v[k] = rf_sigmoid_bwd(g[o].v[k], yq.v[k]);
            }
            if (g_skip && !skip_up) rf_store(g_skip + e, g[o]);
            if (g_skip && skip_up) {  // Q output quads are as many as the half-size plane's pixels
                const int Wi = W >> 1;
                const int i = (int)(q / Wi), ci = (int)(q - (int64_t)i * Wi);
                const int64_t pl = (b * O + o) * Q * 4;
                g_skip[(b * O + o) * Q + q] = rf_up2t(RfAtAcc{g_out + pl, y ? y + pl : nullptr, W}, H, W, i, ci);
            }
        }
        const float v = rb_wave_sum(rf_quad_sum(g[o]));
        if (lane == 0) ws[wave][O * C + o] = v;
    }
    for (int c = 0; c < C; ++c) {
        RfQuad xq = rb_zero();
        if (live) {
            const int64_t e = ((b * C + c) * Q + q) * 4;
            xq = rf_load(x + e);
            rf_store(g_x + e, rf_torgb_bwd_x<O>(wm, C, c, g));
        }
        for (int o = 0; o < O; ++o) {
            const float v = rb_wave_sum(rf_quad_dot(g[o], xq));
            if (lane == 0) ws[wave][o * C + c] = v;
        }
    }
    __syncthreads();
    const int K = O * C + O;
    float* out = partial + (b * chunks + blockIdx.x) * K;
    for (int i = threadIdx.x; i < K; i += kRbBlock) out[i] = ((ws[0][i] + ws[1][i]) + ws[2][i]) + ws[3][i];
}

// wave w < C: channel w; wave C: the biases
__global__ void __launch_bounds__(kRbBlock)
    k_style_torgb_finish(int B, int C, int O, int64_t chunks, const float* __restrict__ partial,
                         const float* __restrict__ weight, const float* __restrict__ s, int64_t s_stride,
                         float* __restrict__ g_weight, float* __restrict__ g_s, float* __restrict__ g_bias) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * kRbWaves + (threadIdx.x >> 6);
    if (w > C) return;  // whole waves
    const int64_t K = (int64_t)O * C + O;
    if (w == C) {
        for (int o = 0; o < O; ++o) {
            float acc = 0.0f;
            for (int b = 0; b < B; ++b) {
                const float v = rb_strided_sum(partial + b * chunks * K + (int64_t)O * C + o, chunks, K, lane);
                acc = b == 0 ? v : acc + v;
            }
            if (lane == 0) g_bias[o] = acc;
        }
        return;
    }
    const int c = w;
    float gw[kRfMaxOut] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = 0; b < B; ++b) {
        const float sb = s[b * s_stride + c];
        float gs = 0.0f;
#pragma unroll
        for (int o = 0; o < kRfMaxOut; ++o) {
            if (o < O) {
                const float m = rb_strided_sum(partial + b * chunks * K + (int64_t)o * C + c, chunks, K, lane);
                gw[o] = b == 0 ? m * sb : gw[o] + m * sb;
                gs = o == 0 ? m * weight[c] : gs + m * weight[o * C + c];
            }
        }
        if (lane == 0) g_s[(int64_t)b * C + c] = gs;
    }
    if (lane == 0) {
#pragma unroll
        for (int o = 0; o < kRfMaxOut; ++o)
            if (o < O) g_weight[o * C + c] = gw[o];
    }
}

// ------------------------------------------------------------------ coeffs

__global__ void __launch_bounds__(kRbCoeffBlock)
    k_style_coeffs_bwd(RbLayers T, int B, int sum_in, int sum_out, const float* __restrict__ s,
                       const float* __restrict__ d, const float* __restrict__ w2, const float* __restrict__ g_d,
                       float* __restrict__ g_s, float* __restrict__ g_w2) {
    __shared__ float t[kRfMaxChannels];
    const GsrStyleLayer ly = T.l[blockIdx.x];
    if (ly.d_off < 0) return;  // the whole workgroup alike: a plain layer's g_s stays as given
    const float* tab = w2 + ly.w2_off;
    if ((int)blockIdx.y < B) {
        const int64_t b = blockIdx.y;
        for (int o = threadIdx.x; o < ly.c_out; o += kRbCoeffBlock)
            t[o] = rf_demod_bwd(d[b * sum_out + ly.d_off + o], g_d[b * sum_out + ly.d_off + o]);
        __syncthreads();
        const int i = threadIdx.x;
        if (i < ly.c_in) {
            float acc = t[0] * tab[i];
            for (int o = 1; o < ly.c_out; ++o) acc = acc + t[o] * tab[(int64_t)o * ly.c_in + i];
            const int64_t e = b * sum_in + ly.s_off + i;
            g_s[e] = g_s[e] + (2.0f * s[e]) * acc;
        }
        return;
    }
    const int slab = (int)blockIdx.y - B;
    const int64_t n = (int64_t)ly.c_out * ly.c_in;
    for (int64_t idx = (int64_t)slab * kRbCoeffBlock + threadIdx.x; idx < n; idx += (int64_t)kRfW2Slabs * kRbCoeffBlock) {
        const int o = (int)(idx / ly.c_in), i = (int)(idx - (int64_t)o * ly.c_in);
        float acc = 0.0f;
        for (int b = 0; b < B; ++b) {
            const float sv = s[(int64_t)b * sum_in + ly.s_off + i];
            const float tb = rf_demod_bwd(d[(int64_t)b * sum_out + ly.d_off + o], g_d[(int64_t)b * sum_out + ly.d_off + o]);
            const float term = tb * (sv * sv);
            acc = b == 0 ? term : acc + term;
        }
        g_w2[ly.w2_off + idx] = acc;
    }
}

static int rb_done() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

static bool rb_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// planes of H x W, W a multiple of 4: quads and chunks of one plane, and a grid of planes * chunks workgroups
// that fits (for the ToRGB, whose grid is chunks x B, planes = B)
static bool rb_image_ok(int64_t planes, int H, int W, int64_t& Q, int64_t& chunks) {
    if (planes <= 0 || H <= 0 || W <= 0 || (W & 3)) return false;
    Q = (int64_t)H * (W >> 2);
    chunks = rf_chunks(Q);
    return planes * chunks * kRbBlock < ((int64_t)1 << 32);  // HIP refuses a launch of 2^32 threads or more
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int64_t gsr_style_backward_chunks(int H, int W) {
    if (H <= 0 || W <= 0 || (W & 3)) return 0;
    return rf_chunks((int64_t)H * (W >> 2));
}

int gsr_style_epilogue_backward(int B, int C, int H, int W, const float* g_y, const float* x, const float* d,
                                int64_t d_stride, const float* noise, int noise_batch, const float* noise_weight,
                                const float* bias, const float* scale, const float* shift, const float* post,
                                int64_t post_stride, float* g_x, float* g_scale, float* g_shift, float* g_d,
                                float* g_post, float* g_bias, float* g_noise_weight, float* workspace, void* stream) {
    int64_t Q, chunks;
    if (B <= 0 || C <= 0 || !rb_image_ok((int64_t)B * C, H, W, Q, chunks) ||
        (noise_batch != 0 && noise_batch != 1 && noise_batch != B) || (d && d_stride < C) || (post && post_stride < C))
        return api_fail(GSR_ERR_ARG, "gsr_style_epilogue_backward: bad sizes (the width must be a multiple of 4)");
    if (!g_y || !x || !bias || !g_x || !g_bias || !workspace || (noise_batch && !(noise && noise_weight && g_noise_weight)) ||
        (!scale != !shift) || (scale && !(g_scale && g_shift)) || (d && !g_d) || (post && !g_post))
        return api_fail(GSR_ERR_ARG, "gsr_style_epilogue_backward: null required pointer");
    if (!rb_aligned(g_y) || !rb_aligned(x) || !rb_aligned(g_x) || (noise_batch && !rb_aligned(noise)) ||
        !rb_aligned(scale) || !rb_aligned(shift) || (scale && (!rb_aligned(g_scale) || !rb_aligned(g_shift))) ||
        !rb_aligned(workspace))
        return api_fail(GSR_ERR_ARG, "gsr_style_epilogue_backward: misaligned pointer");
    const int64_t planes = (int64_t)B * C;
    RbEpiSums* slots = reinterpret_cast<RbEpiSums*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_style_epilogue_bwd, dim3((unsigned)(planes * chunks)), dim3(kRbBlock), 0, st, C, Q, chunks, g_y,
                       x, d, d_stride, noise_batch ? noise : nullptr, noise_batch, noise_weight, bias, scale, shift, post,
                       post_stride, g_x, scale ? g_scale : nullptr, scale ? g_shift : nullptr, slots);
    hipLaunchKernelGGL(k_style_epilogue_finish, dim3(1), dim3(kRbFinishBlock), 0, st, B, C, chunks, slots,
                       slots + planes * chunks, d ? g_d : nullptr, post ? g_post : nullptr, g_bias,
                       noise_batch ? g_noise_weight : nullptr);
    return rb_done();
}

int gsr_style_upmod_backward(int B, int C, int H, int W, int up, int x_batch, const float* g_y, const float* x,
                             const float* s, int64_t s_stride, float* g_x, float* g_s, float* workspace, void* stream) {
    int64_t Q, chunks;
    if (B <= 0 || C <= 0 || !rb_image_ok((int64_t)B * C, H, W, Q, chunks) || (x_batch != 1 && x_batch != B) ||
        (up && x_batch != B) || s_stride < C || (up && (H & 1)))
        return api_fail(GSR_ERR_ARG, "gsr_style_upmod_backward: bad sizes (the output width must be a multiple of 4; "
                                     "a broadcast x only without the upsampling)");
    if (!g_y || !x || !s || !g_x || !g_s || !workspace)
        return api_fail(GSR_ERR_ARG, "gsr_style_upmod_backward: null required pointer");
    if (!rb_aligned(g_y) || (!up && (!rb_aligned(x) || !rb_aligned(g_x))))
        return api_fail(GSR_ERR_ARG, "gsr_style_upmod_backward: misaligned pointer");
    const int64_t planes = (int64_t)B * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_style_upmod_bwd, dim3((unsigned)(planes * chunks)), dim3(kRbBlock), 0, st, B, C, H, W, up ? 1 : 0,
                       x_batch, Q, chunks, g_y, x, s, s_stride, g_x, workspace);
    hipLaunchKernelGGL(k_style_sum_finish, dim3((unsigned)((planes + kRbWaves - 1) / kRbWaves)), dim3(kRbBlock), 0, st,
                       planes, chunks, workspace, g_s);
    return rb_done();
}

int gsr_style_torgb_backward(int B, int C, int O, int H, int W, const float* g_out, const float* y, const float* x,
                             const float* weight, const float* s, int64_t s_stride, int skip_up, float* g_x,
                             float* g_skip, float* g_weight, float* g_s, float* g_bias, float* workspace, void* stream) {
    int64_t Q, chunks;
    if (B <= 0 || B > 65535 || C <= 0 || C > kRfMaxChannels || O <= 0 || O > kRfMaxOut || !rb_image_ok(B, H, W, Q, chunks) ||
       
        s_stride < C || (g_skip && skip_up && (H & 1)))
        return api_fail(GSR_ERR_ARG, "gsr_style_torgb_backward: bad sizes (width a multiple of 4, C <= 512, out_dim <= 4)");
    if (!g_out || !x || !weight || !s || !g_x || !g_weight || !g_s || !g_bias || !workspace)
        return api_fail(GSR_ERR_ARG, "gsr_style_torgb_backward: null required pointer");
    if (!rb_aligned(g_out) || !rb_aligned(y) || !rb_aligned(x) || !rb_aligned(g_x) || (g_skip && !skip_up && !rb_aligned(g_skip)))
        return api_fail(GSR_ERR_ARG, "gsr_style_torgb_backward: misaligned pointer");
    const dim3 g((unsigned)chunks, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const int up = skip_up ? 1 : 0;
#define GSR_RB_TORGB(N)                                                                                              \
    hipLaunchKernelGGL(k_style_torgb_bwd<N>, g, dim3(kRbBlock), 0, st, C, H, W, Q, g_out, y, x, weight, s, s_stride, up, \
                       g_x, g_skip, workspace)
    switch (O) {
        case 1: GSR_RB_TORGB(1); break;
        case 2: GSR_RB_TORGB(2); break;
        case 3: GSR_RB_TORGB(3); break;
        default: GSR_RB_TORGB(4); break;
    }
#undef GSR_RB_TORGB
    hipLaunchKernelGGL(k_style_torgb_finish, dim3((unsigned)((C + 1 + kRbWaves - 1) / kRbWaves)), dim3(kRbBlock), 0, st, B,
                       C, O, chunks, workspace, weight, s, s_stride, g_weight, g_s, g_bias);
    return rb_done();
}

int gsr_style_coeffs_backward(int B, int L, const GsrStyleLayer* layers, int sum_in, int sum_out, int64_t w2_floats,
                              const float* s, const float* d, const float* w2, const float* g_d, float* g_s, float* g_w2,
                              void* stream) {
    if (B <= 0 || B > 65535 - kRfW2Slabs || L <= 0 || L > kRfMaxLayers || sum_in <= 0 || sum_out < 0 || w2_floats < 0)
        return api_fail(GSR_ERR_ARG, "gsr_style_coeffs_backward: bad sizes (at most 32 layers)");
    if (!layers || !s || !g_s) return api_fail(GSR_ERR_ARG, "gsr_style_coeffs_backward: null required pointer");
    RbLayers T{};
    bool any = false;
    for (int i = 0; i < L; ++i) {
        const GsrStyleLayer& y = layers[i];
        bool ok = y.c_in > 0 && y.c_in <= kRfMaxChannels && y.s_off >= 0 && (int64_t)y.s_off + y.c_in <= sum_in;
        if (ok && y.d_off >= 0) {
            ok = d && w2 && g_d && g_w2 && y.c_out > 0 && y.c_out <= kRfMaxChannels &&
                 (int64_t)y.d_off + y.c_out <= sum_out && y.w2_off >= 0 &&
                 (int64_t)y.w2_off + (int64_t)y.c_out * y.c_in <= w2_floats;
            any = true;
        }
        if (!ok) return api_fail(GSR_ERR_ARG, "gsr_style_coeffs_backward: a layer does not fit the totals (c_out <= 512)");
        T.l[i] = y;
    }
    if (!any) return 0;  // no demodulated layer: g_s is the answer as given
    hipLaunchKernelGGL(k_style_coeffs_bwd, dim3((unsigned)L, (unsigned)(B + kRfW2Slabs)), dim3(kRbCoeffBlock), 0,
                       (hipStream_t)stream, T, B, sum_in, sum_out, s, d, w2, g_d, g_s, g_w2);
    return rb_done();
}

}  // extern "C"
