// refiner.hip -- the refiner decoder's glue (include/gsr_refiner.h) for gfx950: the modulation and
// demodulation coefficients of a whole StyleGAN2 decoder in one launch, and the three elementwise passes
// that remain around each convolution once the modulated conv is written as a plain conv.  The
// arithmetic is refiner_dev.h's, shared with the host check.
//
//   k_style_coeffs    a workgroup per (layer, frame).  A wave per modulation row: 64 strided partial
//                     sums of latent . weight, a butterfly, + bias -> s.  Then, for a demodulated layer,
//                     a wave per output channel over the s just stored -> d.
//   k_style_upmod     a lane per 4 consecutive output pixels of a row: s[b,c] * (up2(x) or x).
//   k_style_epilogue  a lane per 4 pixels: sqrt(2)*d, noise, bias, LeakyReLU, SFT, the next conv's
//                     input modulation.  In place allowed: a lane reads its pixels before it writes.
//   k_style_torgb     a lane per 4 pixels, every output channel in registers; the O x C products
//                     W[o,c]*s[b,c] go to LDS once per workgroup.
// No atomics; no LDS but the ToRGB products; 16-byte stores everywhere and 16-byte loads wherever the
// source is not the half-resolution plane of an upsampling.
#include <hip/hip_runtime.h>

#include "../../include/gsr.h"
#include "../../include/gsr_refiner.h"
#include "gsr_internal.h"
#include "refiner_dev.h"

#pragma clang fp contract(off)

namespace gsr {

constexpr int kRfBlock = 256;
constexpr int kRfCoeffBlock = 1024;

struct RfLayers {
    GsrStyleLayer l[kRfMaxLayers];
};

__device__ __forceinline__ float rf_wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

__global__ void __launch_bounds__(kRfCoeffBlock) k_style_coeffs(RfLayers T, int S, int sum_in, int sum_out,
                                                                const float* __restrict__ latent,
                                                                const float* __restrict__ mw,
                                                                const float* __restrict__ mb,
                                                                const float* __restrict__ w2, float* s, float* d) {
    const GsrStyleLayer ly = T.l[blockIdx.x];
    const int b = (int)blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int waves = kRfCoeffBlock / 64;
    const float* lat = latent + (int64_t)b * S;
    float* sb = s + (int64_t)b * sum_in + ly.s_off;
    for (int row = wave; row < ly.c_in; row += waves) {
        const float* w = mw + (int64_t)(ly.s_off + row) * S;
        float acc = 0.0f;
        for (int k = lane; k < S; k += 64) acc = acc + lat[k] * w[k];
        acc = rf_wave_sum(acc);
        if (lane == 0) sb[row] = acc + mb[ly.s_off + row];
    }
    if (ly.d_off < 0) return;  // the whole workgroup alike
    __threadfence_block();
    __syncthreads();  // the layer's s, stored by this workgroup's waves, is read back below
    float* db = d + (int64_t)b * sum_out + ly.d_off;
    for (int o = wave; o < ly.c_out; o += waves) {
        const float* t = w2 + ly.w2_off + (int64_t)o * ly.c_in;
        float acc = 0.0f;
        for (int i = lane; i < ly.c_in; i += 64) acc = acc + rf_demod_term(sb[i], t[i]);
        acc = rf_wave_sum(acc);
        if (lane == 0) db[o] = rf_demod(acc, ly.eps);
    }
}

// quad index -> plane (b*C + c), row, first column
struct RfPos {
    int64_t plane;
    int r, j0;
};

__device__ __forceinline__ bool rf_pos(int64_t quads, int H, int Wq, RfPos& p) {
    const int64_t i = (int64_t)blockIdx.x * kRfBlock + threadIdx.x;
    if (i >= quads) return false;
    const int64_t row = i / Wq;
    p.j0 = (int)(i - row * Wq) * 4;
    p.plane = row / H;
    p.r = (int)(row - p.plane * H);
    return true;
}

__global__ void __launch_bounds__(kRfBlock) k_style_upmod(int64_t quads, int C, int H, int W, int up, int x_batch,
                                                          const float* __restrict__ x, const float* __restrict__ s,
                                                          int64_t s_stride, float* __restrict__ y) {
    RfPos p;
    if (!rf_pos(quads, H, W >> 2, p)) return;
    const int64_t b = p.plane / C;
    const int c = (int)(p.plane - b * C);
    const float sc = s[b * s_stride + c];
    const int64_t xplane = x_batch == 1 ? c : p.plane;
    RfQuad q;
    if (up) {
        const int Hi = H >> 1, Wi = W >> 1;
        rf_up2_quad(x + xplane * Hi * Wi, Hi, Wi, p.r, p.j0, q.v);
    } else {
        q = rf_load(x + (xplane * H + p.r) * W + p.j0);
    }
    for (int k = 0; k < 4; ++k) q.v[k] = sc * q.v[k];
    rf_store(y + (p.plane * H + p.r) * W + p.j0, q);
}

__global__ void __launch_bounds__(kRfBlock) k_style_epilogue(int64_t quads, int C, int H, int W, const float* x,
                                                             const float* __restrict__ d, int64_t d_stride,
                                                             const float* __restrict__ noise, int noise_batch,
                                                             const float* __restrict__ noise_weight,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ post, int64_t post_stride,
                                                             float* y) {
    RfPos p;
    if (!rf_pos(quads, H, W >> 2, p)) return;
    const int64_t b = p.plane / C;
    const int c = (int)(p.plane - b * C);
    const int64_t e = (p.plane * H + p.r) * W + p.j0;
    const float a = d ? kRfSqrt2 * d[b * d_stride + c] : kRfSqrt2;
    const float bc = bias[c];
    RfQuad q = rf_load(x + e);
    RfQuad n = {{0.0f, 0.0f, 0.0f, 0.0f}};
    if (noise_batch) {
        const float nw = noise_weight[0];
        n = rf_load(noise + ((noise_batch == 1 ? 0 : b) * H + p.r) * W + p.j0);
        for (int k = 0; k < 4; ++k) n.v[k] = nw * n.v[k];
    }
    for (int k = 0; k < 4; ++k) q.v[k] = rf_epilogue(q.v[k], a, n.v[k], bc);
    if (scale) {
        const RfQuad sc = rf_load(scale + e), sh = rf_load(shift + e);
        for (int k = 0; k < 4; ++k) q.v[k] = rf_sft(q.v[k], sc.v[k], sh.v[k]);
    }
    if (post) {
        const float ps = post[b * post_stride + c];
        for (int k = 0; k < 4; ++k) q.v[k] = q.v[k] * ps;
    }
    rf_store(y + e, q);
}

template <int O>
__global__ void __launch_bounds__(kRfBlock) k_style_torgb(int64_t quads, int C, int H, int W,
                                                          const float* __restrict__ x,
                                                          const float* __restrict__ weight,
                                                          const float* __restrict__ s, int64_t s_stride,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ skip, int skip_up, int sigmoid,
                                                          float* __restrict__ out) {
    __shared__ float wm[kRfMaxOut * kRfMaxChannels];
    __shared__ float bs[kRfMaxOut];
    const int64_t b = blockIdx.y;
    for (int i = threadIdx.x; i < O * C; i += kRfBlock) wm[i] = weight[i] * s[b * s_stride + (i % C)];
    if (threadIdx.x < O) bs[threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    RfPos p;  // plane = 0: the quads of one frame
    if (!rf_pos(quads, H, W >> 2, p)) return;
    const int64_t HW = (int64_t)H * W, e = (int64_t)p.r * W + p.j0;
    RfQuad acc[O];
    rf_torgb<O>(wm, bs, x + b * C * HW + e, HW, C, acc);
    for (int o = 0; o < O; ++o) {
        if (skip) {
            RfQuad k4;
            if (skip_up) {
                const int Hi = H >> 1, Wi = W >> 1;
                rf_up2_quad(skip + (b * O + o) * Hi * Wi, Hi, Wi, p.r, p.j0, k4.v);
            } else {
                k4 = rf_load(skip + (b * O + o) * HW + e);
            }
            for (int k = 0; k < 4; ++k) acc[o].v[k] = acc[o].v[k] + k4.v[k];
        }
        if (sigmoid)
            for (int k = 0; k < 4; ++k) acc[o].v[k] = ex_sigmoid(acc[o].v[k]);
        rf_store(out + (b * O + o) * HW + e, acc[o]);
    }
}

static int rf_done() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

static bool rf_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// B*C planes of H x W, W a multiple of 4, a grid that fits
static bool rf_image_ok(int B, int C, int H, int W, int64_t& quads, unsigned& grid) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (W & 3)) return false;
    quads = (int64_t)B * C * H * (W >> 2);
    const int64_t blocks = (quads + kRfBlock - 1) / kRfBlock;
    if (blocks > INT32_MAX) return false;
    grid = (unsigned)blocks;
    return true;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_style_coeffs(int B, int S, int L, const GsrStyleLayer* layers, int sum_in, int sum_out, int64_t w2_floats,
                     const float* latent, const float* mod_weight, const float* mod_bias, const float* w2, float* s,
                     float* d, void* stream) {
    if (B <= 0 || B > 65535 || S <= 0 || L <= 0 || L > kRfMaxLayers || sum_in <= 0 || sum_out < 0 || w2_floats < 0)
        return api_fail(GSR_ERR_ARG, "gsr_style_coeffs: bad sizes (at most 32 layers)");
    if (!layers || !latent || !mod_weight || !mod_bias || !s)
        return api_fail(GSR_ERR_ARG, "gsr_style_coeffs: null required pointer");
    RfLayers T{};
    for (int i = 0; i < L; ++i) {
        const GsrStyleLayer& y = layers[i];
        bool ok = y.c_in > 0 && y.c_in <= kRfMaxChannels && y.s_off >= 0 && (int64_t)y.s_off + y.c_in <= sum_in;
        if (ok && y.d_off >= 0)
            ok = d && w2 && y.c_out > 0 && (int64_t)y.d_off + y.c_out <= sum_out && y.w2_off >= 0 &&
                 (int64_t)y.w2_off + (int64_t)y.c_out * y.c_in <= w2_floats;
        if (!ok) return api_fail(GSR_ERR_ARG, "gsr_style_coeffs: a layer does not fit the totals");
        T.l[i] = y;
    }
    hipLaunchKernelGGL(k_style_coeffs, dim3((unsigned)L, (unsigned)B), dim3(kRfCoeffBlock), 0, (hipStream_t)stream, T, S,
                       sum_in, sum_out, latent, mod_weight, mod_bias, w2, s, d);
    return rf_done();
}

int gsr_style_upmod(int B, int C, int H, int W, int up, int x_batch, const float* x, const float* s, int64_t s_stride,
                    float* y, void* stream) {
    int64_t quads;
    unsigned grid;
    if (!rf_image_ok(B, C, H, W, quads, grid) || (x_batch != 1 && x_batch != B) || s_stride < C || (up && (H & 1)))
        return api_fail(GSR_ERR_ARG, "gsr_style_upmod: bad sizes (the output width must be a multiple of 4)");
    if (!x || !s || !y) return api_fail(GSR_ERR_ARG, "gsr_style_upmod: null required pointer");
    if (!rf_aligned(y) || (!up && !rf_aligned(x))) return api_fail(GSR_ERR_ARG, "gsr_style_upmod: misaligned pointer");
    hipLaunchKernelGGL(k_style_upmod, dim3(grid), dim3(kRfBlock), 0, (hipStream_t)stream, quads, C, H, W, up ? 1 : 0,
                       x_batch, x, s, s_stride, y);
    return rf_done();
}

int gsr_style_epilogue(int B, int C, int H, int W, const float* x, const float* d, int64_t d_stride, const float* noise,
                       int noise_batch, const float* noise_weight, const float* bias, const float* scale,
                       const float* shift, const float* post, int64_t post_stride, float* y, void* stream) {
    int64_t quads;
    unsigned grid;
    if (!rf_image_ok(B, C, H, W, quads, grid) || (noise_batch != 0 && noise_batch != 1 && noise_batch != B) ||
        (d && d_stride < C) || (post && post_stride < C))
        return api_fail(GSR_ERR_ARG, "gsr_style_epilogue: bad sizes (the width must be a multiple of 4)");
    if (!x || !y || !bias || (noise_batch && !(noise && noise_weight)) || (!scale != !shift))
        return api_fail(GSR_ERR_ARG, "gsr_style_epilogue: null required pointer");
    if (!rf_aligned(x) || !rf_aligned(y) || (noise_batch && !rf_aligned(noise)) || !rf_aligned(scale) || !rf_aligned(shift))
        return api_fail(GSR_ERR_ARG, "gsr_style_epilogue: misaligned pointer");
    hipLaunchKernelGGL(k_style_epilogue, dim3(grid), dim3(kRfBlock), 0, (hipStream_t)stream, quads, C, H, W, x, d,
                       d_stride, noise_batch ? noise : nullptr, noise_batch, noise_weight, bias, scale, shift, post,
                       post_stride, y);
    return rf_done();
}

int gsr_style_torgb(int B, int C, int O, int H, int W, const float* x, const float* weight, const float* s,
                    int64_t s_stride, const float* bias, const float* skip, int skip_up, int sigmoid, float* out,
                    void* stream) {
    int64_t quads;
    unsigned grid;
    if (!rf_image_ok(1, 1, H, W, quads, grid) || B <= 0 || B > 65535 || C <= 0 || C > kRfMaxChannels || O <= 0 ||
        O > kRfMaxOut || s_stride < C || (skip && skip_up && (H & 1)))
        return api_fail(GSR_ERR_ARG, "gsr_style_torgb: bad sizes (width a multiple of 4, C <= 512, out_dim <= 4)");
    if (!x || !weight || !s || !bias || !out) return api_fail(GSR_ERR_ARG, "gsr_style_torgb: null required pointer");
    if (!rf_aligned(x) || !rf_aligned(out) || (skip && !skip_up && !rf_aligned(skip)))
        return api_fail(GSR_ERR_ARG, "gsr_style_torgb: misaligned pointer");
    const dim3 g(grid, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const int up = skip_up ? 1 : 0, sg = sigmoid ? 1 : 0;
#define GSR_RF_TORGB(N)                                                                                              \
    hipLaunchKernelGGL(k_style_torgb<N>, g, dim3(kRfBlock), 0, st, quads, C, H, W, x, weight, s, s_stride, bias, skip, \
                       up, sg, out)
    switch (O) {
        case 1: GSR_RF_TORGB(1); break;
        case 2: GSR_RF_TORGB(2); break;
        case 3: GSR_RF_TORGB(3); break;
        default: GSR_RF_TORGB(4); break;
    }
#undef GSR_RF_TORGB
    return rf_done();
}

}  // extern "C"
