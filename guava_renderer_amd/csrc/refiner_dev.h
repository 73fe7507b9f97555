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

}  // namespace gsr
