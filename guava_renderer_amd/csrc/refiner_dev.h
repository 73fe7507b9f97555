// refiner_dev.h -- the arithmetic of the refiner decoder's glue (include/gsr_refiner.h) as host/device
// inline functions: the bilinear x2 taps, the modulation and demodulation coefficients, the StyleConv
// epilogue and the ToRGB sum.  refiner.hip's kernels call them on the device; tools/refiner_check.cpp
// calls the very same functions on the host under the sanitizers.  Every operation is float32, written
// with all of its parentheses and evaluated in the order written (no fma: the pragma below and the
// build's -ffp-contract=off); `/` and sqrtf are correctly rounded.  tests/refiner_cases.py restates
// them in numpy, bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "extract_dev.h"  // ex_sigmoid: the stated sigmoid

#pragma clang fp contract(off)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_RF_HD __host__ __device__ __forceinline__
#else
#define GSR_RF_HD inline
#endif

namespace gsr {

constexpr float kRfSqrt2 = 1.41421356237309515f;  // float32(2 ** 0.5)
constexpr float kRfSlope = 0.2f;                  // LeakyReLU's negative slope
constexpr int kRfMaxLayers = 32;                  // layers of one gsr_style_coeffs call
constexpr int kRfMaxChannels = 512;               // c_in of a layer, C of a ToRGB
constexpr int kRfMaxOut = 4;                      // out_dim of a ToRGB

// One tap pair of the bilinear x2 upsampling (align_corners=False): an output sample lies a quarter of
// an input step from its nearer input sample, y = 0.75f*near + 0.25f*far.  Both products are rounded.
GSR_RF_HD float rf_tap(float near_v, float far_v) { return 0.75f * near_v + 0.25f * far_v; }

// The nearer and the farther input index of output index j along an axis of n input samples: j = 2i
// reads (i, i - 1), j = 2i + 1 reads (i, i + 1), the farther one clamped to [0, n - 1] (so that a border
// sample is rf_tap(x, x), not x).
GSR_RF_HD void rf_up_index(int j, int n, int& near_i, int& far_i) {
    near_i = j >> 1;
    far_i = (j & 1) ? near_i + 1 : near_i - 1;
    if (far_i < 0) far_i = 0;
    if (far_i > n - 1) far_i = n - 1;
}

// up2(x)[r][j] of one H x W plane, rows first, then columns:
//   v(c) = rf_tap(x[rn][c], x[rf][c]),   y = rf_tap(v(cn), v(cf)).
GSR_RF_HD float rf_up2(const float* x, int H, int W, int r, int j) {
    int rn, rf, cn, cf;
    rf_up_index(r, H, rn, rf);
    rf_up_index(j, W, cn, cf);
    const float vn = rf_tap(x[(int64_t)rn * W + cn], x[(int64_t)rf * W + cn]);
    const float vf = rf_tap(x[(int64_t)rn * W + cf], x[(int64_t)rf * W + cf]);
    return rf_tap(vn, vf);
}

// Four consecutive outputs j0 .. j0 + 3 (j0 a multiple of 4) of output row r: they read the input
// columns j0/2 - 1 .. j0/2 + 2, clamped.  The same values as four rf_up2 calls.
GSR_RF_HD void rf_up2_quad(const float* x, int H, int W, int r, int j0, float y[4]) {
    int rn, rf;
    rf_up_index(r, H, rn, rf);
    const int c0 = j0 >> 1;
    float v[4];
    for (int k = 0; k < 4; ++k) {
        int c = c0 - 1 + k;
        c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
        v[k] = rf_tap(x[(int64_t)rn * W + c], x[(int64_t)rf * W + c]);
    }
    y[0] = rf_tap(v[1], v[0]);
    y[1] = rf_tap(v[1], v[2]);
    y[2] = rf_tap(v[2], v[1]);
    y[3] = rf_tap(v[2], v[3]);
}

// Demodulation: d = 1.0f / sqrtf(acc + eps), acc the float32 sum over c_in of (s*s)*w2.  A denormal s
// contributes +0 (d = rsqrt(eps) when every term vanishes); a sum that overflows gives d = +0; s*s
// overflowing (|s| > 1.8e19) against w2 == 0 is inf * 0 = NaN.
GSR_RF_HD float rf_demod_term(float s, float w2) { return (s * s) * w2; }
GSR_RF_HD float rf_demod(float acc, float eps) { return 1.0f / sqrtf(acc + eps); }

// The StyleConv epilogue of one element.  a = kRfSqrt2 * d[b,c] (kRfSqrt2 without a d), n = nw * noise
// (+0 without a noise), bias = bias[c]:
//   v = ((a * x) + n) + bias;   y = v >= 0 ? v : 0.2f * v   (a NaN v takes the second branch)
GSR_RF_HD float rf_epilogue(float x, float a, float n, float bias) {
    const float v = ((a * x) + n) + bias;
    return v >= 0.0f ? v : kRfSlope * v;
}

// y * scale + shift: the SFT step, the product rounded
GSR_RF_HD float rf_sft(float y, float scale, float shift) { return (y * scale) + shift; }

// four consecutive pixels of a row: one 16-byte access
struct alignas(16) RfQuad {
    float v[4];
};
GSR_RF_HD RfQuad rf_load(const float* p) { return *reinterpret_cast<const RfQuad*>(p); }
GSR_RF_HD void rf_store(float* p, const RfQuad& q) { *reinterpret_cast<RfQuad*>(p) = q; }

// ToRGB of four pixels and O outputs: acc[o] = wm[o*C]*x[0]; acc[o] = acc[o] + wm[o*C + c]*x[c], c
// ascending, channel c's four pixels at x + c*xs; then + bias[o].
template <int O>
GSR_RF_HD void rf_torgb(const float* wm, const float* bias, const float* x, int64_t xs, int C, RfQuad acc[O]) {
    const RfQuad x0 = rf_load(x);
    for (int o = 0; o < O; ++o)
        for (int k = 0; k < 4; ++k) acc[o].v[k] = wm[o * C] * x0.v[k];
    for (int c = 1; c < C; ++c) {
        const RfQuad xc = rf_load(x + (int64_t)c * xs);
        for (int o = 0; o < O; ++o)
            for (int k = 0; k < 4; ++k) acc[o].v[k] = acc[o].v[k] + wm[o * C + c] * xc.v[k];
    }
    for (int o = 0; o < O; ++o)
        for (int k = 0; k < 4; ++k) acc[o].v[k] = acc[o].v[k] + bias[o];
}

// ------------------------------------------------------------------ backward (refiner_bwd.hip)

constexpr int kRfChunkQuads = 256;  // lane-quads of one reduction chunk: one workgroup, a quad per lane
constexpr int kRfW2Slabs = 8;       // workgroups per layer that share the g_w2 table of gsr_style_coeffs_backward

// chunks of a plane of H x W (W a multiple of 4): a function of the shape alone
GSR_RF_HD int64_t rf_chunks(int64_t plane_quads) { return (plane_quads + kRfChunkQuads - 1) / kRfChunkQuads; }

// An index one step outside an axis of n output samples is folded back onto the border sample: it is the
// border sample's clamped farther tap (rf_up_index) that lands there.
GSR_RF_HD int rf_fold(int r, int n) { return r < 0 ? 0 : (r > n - 1 ? n - 1 : r); }

// The transposed tap pair along one axis: an input sample collects the four output samples 2i - 1 .. 2i + 2
// with rf_tap's weights, in ascending index order.
GSR_RF_HD float rf_tap_t(float a, float b, float c, float d) {
    return ((0.25f * a + 0.75f * b) + 0.75f * c) + 0.25f * d;
}

// up2T(g)[i][c]: the transpose of up2.  g is the 2h x 2w plane (H = 2h, W = 2w), read through at(r, j).
// Columns first, then rows (up2 runs rows first, so this is its exact reverse):
//   u(k) = rf_tap_t(g[r_k][fold(2c-1)], g[r_k][2c], g[r_k][2c+1], g[r_k][fold(2c+2)]),  r_k = fold(2i-1+k)
//   up2T = rf_tap_t(u(0), u(1), u(2), u(3)).
template <class At>
GSR_RF_HD float rf_up2t(const At& at, int H, int W, int i, int c) {
    const int j0 = rf_fold(2 * c - 1, W), j3 = rf_fold(2 * c + 2, W);
    float u[4];
    for (int k = 0; k < 4; ++k) {
        const int r = rf_fold(2 * i - 1 + k, H);
        u[k] = rf_tap_t(at(r, j0), at(r, 2 * c), at(r, 2 * c + 1), at(r, j3));
    }
    return rf_tap_t(u[0], u[1], u[2], u[3]);
}

// g read from a plane as it is
struct RfAtPlain {
    const float* g;
    int W;
    GSR_RF_HD float operator()(int r, int j) const { return g[(int64_t)r * W + j]; }
};

// the gradient through the sigmoid, from the saved output y
GSR_RF_HD float rf_sigmoid_bwd(float g, float y) { return g * (y * (1.0f - y)); }

// g_acc of a ToRGB read in place: g_out, or g_out through the sigmoid of the saved output y (y != nullptr)
struct RfAtAcc {
    const float* g;
    const float* y;
    int W;
    GSR_RF_HD float operator()(int r, int j) const {
        const int64_t e = (int64_t)r * W + j;
        return y ? rf_sigmoid_bwd(g[e], y[e]) : g[e];
    }
};

// a lane's share of a reduction over pixels: the four products of its quad, summed pairwise
GSR_RF_HD float rf_quad_sum(const RfQuad& t) { return (t.v[0] + t.v[1]) + (t.v[2] + t.v[3]); }
GSR_RF_HD float rf_quad_dot(const RfQuad& a, const RfQuad& b) {
    return (a.v[0] * b.v[0] + a.v[1] * b.v[1]) + (a.v[2] * b.v[2] + a.v[3] * b.v[3]);
}

// The StyleConv epilogue's backward of one element.  v and l are recomputed with the forward's
// expressions and the forward's branch (v >= 0: slope 1; otherwise, a NaN included, 0.2f):
//   g1 = g_y * post (g_y without a post);  y1 = l*scale + shift (l without the SFT maps)
//   gl = g1 * scale (g1 without);  g_v = v >= 0 ? gl : 0.2f * gl
//   g_x = a * g_v;  g_scale = g1 * l;  g_shift = g1
// and the element's terms of the plane sums: g_v * x, g_v, g_y * y1 in float32.  The noise weight's
// gradient reduces the whole tensor to one number, the most cancellation-prone sum of all: its terms
// g_v * noise are formed and added in float64 (rf_noise_term: exact products).
struct RfEpiGrad {
    float g_x, g_scale, g_shift;
    float t_x, g_v, t_post;
};
GSR_RF_HD double rf_noise_term(float g_v, float noise) { return (double)g_v * (double)noise; }
GSR_RF_HD RfEpiGrad rf_epilogue_bwd(float gy, float x, float a, float nw, float noise, float bias, bool sft, float scale,
                                    float shift, bool has_post, float post) {
    const float v = ((a * x) + (nw * noise)) + bias;
    const bool pos = v >= 0.0f;
    const float l = pos ? v : kRfSlope * v;
    const float g1 = has_post ? gy * post : gy;
    const float y1 = sft ? rf_sft(l, scale, shift) : l;
    const float gl = sft ? g1 * scale : g1;
    RfEpiGrad r;
    r.g_v = pos ? gl : kRfSlope * gl;
    r.g_x = a * r.g_v;
    r.g_scale = g1 * l;
    r.g_shift = g1;
    r.t_x = r.g_v * x;
    r.t_post = gy * y1;
    return r;
}

// ToRGB backward, channel c of four pixels: g_x = wm[c]*g[0]; g_x = g_x + wm[o*C + c]*g[o], o ascending.
template <int O>
GSR_RF_HD RfQuad rf_torgb_bwd_x(const float* wm, int C, int c, const RfQuad g[O]) {
    RfQuad r;
    for (int k = 0; k < 4; ++k) r.v[k] = wm[c] * g[0].v[k];
    for (int o = 1; o < O; ++o)
        for (int k = 0; k < 4; ++k) r.v[k] = r.v[k] + wm[o * C + c] * g[o].v[k];
    return r;
}

// Demodulation backward: t = -0.5 * d^3 * g_d, d as the forward stored it.
GSR_RF_HD float rf_demod_bwd(float d, float g_d) { return (-0.5f * ((d * d) * d)) * g_d; }

}  // namespace gsr
