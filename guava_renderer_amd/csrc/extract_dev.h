// extract_dev.h -- the per-texel arithmetic of the UV Gaussian extraction (include/gsr_extract.h): the
// stated exp, the head activations and their gradients, and the tile / slot arithmetic, as host/device
// inline functions.  extract.hip's kernels call them on the device; tools/extract_check.cpp calls the
// very same functions on the host under the sanitizers.  Every operation is float32, written with all
// of its parentheses; the build compiles with -ffp-contract=off, `/` and sqrtf are correctly rounded.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_EX_HD __host__ __device__ __forceinline__
#else
#define GSR_EX_HD inline
#endif

namespace gsr {

constexpr int kExTile = 64;              // texels per tile: one per lane of a wave
constexpr float kExOverflow = 88.72284f;  // ex_exp(x) = +inf above
constexpr float kExUnderflow = -104.0f;   // ex_exp(x) = +0 below
constexpr float kExRotEps = 1e-12f;       // F.normalize's eps
constexpr float kExRotLo = 1e-24f;        // the sum of squares' range in which the norm is refined
constexpr float kExRotHi = 1e30f;

// 2^k, k in [-126, 127], from the exponent field
GSR_EX_HD float ex_pow2(int k) {
    const uint32_t u = (uint32_t)(k + 127) << 23;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// The stated exp (no library call).  n = floorf(x*log2e + 0.5f); Cody-Waite reduction with two
// constants, r = (x - n*LN2_HI) - n*LN2_LO (n*LN2_HI is exact: LN2_HI = 355/512, |n| <= 150); Cephes'
// degree-5 polynomial by Horner, y = (p*(r*r) + r) + 1; scaling by 2^n in two power-of-two steps,
// (y * 2^(n>>1)) * 2^(n - (n>>1)): the first product is exact, so a subnormal result is rounded once.
// NaN -> NaN, x > kExOverflow -> +inf, x < kExUnderflow -> +0.
// Within 0.68 * 2^-23 relative of exp wherever exp(x) is a normal float (tests/test_gaussian_extract_ref.py).
GSR_EX_HD float ex_exp(float x) {
    if (x != x) return x;
    if (x > kExOverflow) return INFINITY;
    if (x < kExUnderflow) return 0.0f;
    const float n = floorf(x * 1.44269504f + 0.5f);
    const float r = (x - n * 0.693359375f) - n * -2.12194440e-4f;
    const float z = r * r;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float y = (p * z + r) + 1.0f;
    const int k = (int)n;  // n in [-150, 128]
    const int k1 = k >> 1, k2 = k - k1;
    return (y * ex_pow2(k1)) * ex_pow2(k2);
}

// y = 1 / (1 + ex_exp(-x))
GSR_EX_HD float ex_sigmoid(float x) { return 1.0f / (1.0f + ex_exp(-x)); }

// dx = (g*(1 - y))*y, y recomputed from the raw input
GSR_EX_HD float ex_sigmoid_bwd(float x, float g) {
    const float y = ex_sigmoid(x);
    return (g * (1.0f - y)) * y;
}

// dx = g*y
GSR_EX_HD float ex_exp_bwd(float x, float g) { return g * ex_exp(x); }

// s = a + b and its rounding error e: a + b = s + e exactly (Knuth's two-sum)
GSR_EX_HD float ex_two_sum(float a, float b, float& e) {
    const float s = a + b;
    const float bb = s - a;
    e = (a - (s - bb)) + (b - bb);
    return s;
}

// p = a*a and its rounding error e: a*a = p + e exactly (Dekker's split by 4097, no fma), for |a| < 1e30
GSR_EX_HD float ex_square(float a, float& e) {
    const float p = a * a;
    const float t = 4097.0f * a;
    const float hi = t - (t - a);
    const float lo = a - hi;
    e = ((hi * hi - p) + (hi + hi) * lo) + lo * lo;
    return p;
}

// The quaternion's norm.  S = ((x0*x0 + x1*x1) + x2*x2) + x3*x3 and n0 = sqrtf(S) are the plain float32
// evaluation.  That alone is up to 2 * 2^-24 off the exact norm (seven roundings under the root), and
// x_k / n then up to 4 * 2^-24 off (measured 3.05), above the 2 * 2^-24 this operation promises.  So for
// kExRotLo <= S <= kExRotHi the norm is refined to the correctly rounded one: c collects the rounding
// errors of the four squares and the three adds, (p, pe) is the exact square of n0, and one Newton
// step gives n = n0 + (((S - p) - pe) + c) / (n0 + n0).  Outside that range (overflow, underflow, NaN)
// the error terms mean nothing and n = n0.  d = fmaxf(n, 1e-12f) (a NaN n gives 1e-12f).
GSR_EX_HD float ex_rot_norm(const float x[4], float& d) {
    float e0, e1, e2, e3, f1, f2, f3, pe;
    const float p0 = ex_square(x[0], e0), p1 = ex_square(x[1], e1);
    const float p2 = ex_square(x[2], e2), p3 = ex_square(x[3], e3);
    const float s1 = ex_two_sum(p0, p1, f1);
    const float s2 = ex_two_sum(s1, p2, f2);
    const float S = ex_two_sum(s2, p3, f3);
    const float c = ((e0 + e1) + (e2 + e3)) + ((f1 + f2) + f3);
    const float n0 = sqrtf(S);
    float n = n0;
    if (S >= kExRotLo && S <= kExRotHi) {
        const float p = ex_square(n0, pe);
        n = n0 + (((S - p) - pe) + c) / (n0 + n0);
    }
    d = fmaxf(n, kExRotEps);
    return n;
}

// y_k = x_k / d
GSR_EX_HD void ex_rot(const float x[4], float y[4]) {
    float d;
    ex_rot_norm(x, d);
    for (int k = 0; k < 4; ++k) y[k] = x[k] / d;
}

// F.normalize's gradient: n >= 1e-12f: s = ((g0*y0 + g1*y1) + g2*y2) + g3*y3, dx_k = (g_k - y_k*s)/d;
// otherwise (the clamp branch) dx_k = g_k/d
GSR_EX_HD void ex_rot_bwd(const float x[4], const float g[4], float dx[4]) {
    float d;
    const float n = ex_rot_norm(x, d);
    if (n >= kExRotEps) {
        float y[4];
        for (int k = 0; k < 4; ++k) y[k] = x[k] / d;
        const float s = ((g[0] * y[0] + g[1] * y[1]) + g[2] * y[2]) + g[3] * y[3];
        for (int k = 0; k < 4; ++k) dx[k] = (g[k] - y[k] * s) / d;
    } else {
        for (int k = 0; k < 4; ++k) dx[k] = g[k] / d;
    }
}

// The keep predicate of texel t: inside [0, T), mask set, and (pruning) opacity > threshold, strictly,
// on the float32 opacity this operation itself produces (the sigmoid of the raw logit when `raw`).
// opacity may be null: no opacity predicate.  Reads mask[t] and opacity[t] only.
GSR_EX_HD bool ex_keep(const uint8_t* mask, const float* opacity, int raw, float threshold, int T, int t) {
    if (t < 0 || t >= T || mask[t] == 0) return false;
    if (!opacity) return true;
    const float o = raw ? ex_sigmoid(opacity[t]) : opacity[t];
    return o > threshold;
}

// tiles of T texels
GSR_EX_HD int ex_tiles(int T) { return (int)(((int64_t)T + kExTile - 1) / kExTile); }

// kept lanes below `lane` in the tile's 64-bit keep ballot
GSR_EX_HD int ex_rank(uint64_t ballot, int lane) {
    const uint64_t below = ballot & (((uint64_t)1 << lane) - 1);
    return __builtin_popcountll(below);
}

// row stride (floats) of the staged tile of K = C + 11 columns: odd, so that 64 lanes writing one
// column fall into distinct LDS banks
GSR_EX_HD int ex_stride(int K) { return K | 1; }

// The rows [count + dropped_before, ... + dropped_here) that a pruning tile writes as zeros: with the
// unpruned scan u and the pruned scan p of the same tile, dropped_before = u[tile] - p[tile] and
// dropped_here = (u[tile+1] - u[tile]) - (p[tile+1] - p[tile]); over the tiles these ranges partition
// [count, N).
GSR_EX_HD void ex_zero_rows(const int32_t* u, const int32_t* p, int tile, int count, int& first, int& n) {
    first = count + (u[tile] - p[tile]);
    n = (u[tile + 1] - u[tile]) - (p[tile + 1] - p[tile]);
}

}  // namespace gsr
