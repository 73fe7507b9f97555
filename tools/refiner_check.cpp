// Host check of the refiner decoder's arithmetic (guava_renderer_amd/csrc/refiner_dev.h): the very
// functions the kernels call, run on the CPU under the address and undefined-behaviour sanitizers over
// edge inputs, every plane exactly sized on the heap so that a tap outside its plane is an error:
// one-row and two-column planes (every output on a clamped border), H != W, denormal and huge
// modulation coefficients, and a sum of squares of zero, where eps alone is under the square root.
// Build and run on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I guava_renderer_amd/csrc tools/refiner_check.cpp -o refiner_check && ./refiner_check
// Prints its counts and "clean" and exits 0, or the sanitizer's report of the first bad operation
// (non-zero exit); a value that disagrees with the header's stated results also fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "refiner_dev.h"

static long n_up = 0, n_demod = 0, n_epi = 0, n_rgb = 0, n_bad = 0;

static void expect(bool ok, const char* what, double a, double b) {
    if (!ok) {
        n_bad++;
        printf("FAIL %s (%g, %g)\n", what, a, b);
    }
}

static float rnd() { return (float)rand() / (float)RAND_MAX * 4.0f - 2.0f; }

// exactly sized; 16-byte aligned when it holds whole quads (RfQuad accesses), else read by scalars only
static float* plane(size_t n) {
    return (float*)(n % 4 ? malloc(n * sizeof(float)) : aligned_alloc(16, n * sizeof(float)));
}

// torch's bilinear x2 (align_corners=False) in double
static double up2_ref(const float* x, int H, int W, int r, int j) {
    auto axis = [](int o, int n, int& i0, int& i1, double& l) {
        double src = (o + 0.5) / 2.0 - 0.5;
        if (src < 0) src = 0;
        i0 = (int)src;
        i1 = i0 + 1 < n ? i0 + 1 : n - 1;
        l = src - i0;
    };
    int r0, r1, c0, c1;
    double lr, lc;
    axis(r, H, r0, r1, lr);
    axis(j, W, c0, c1, lc);
    const double top = (1 - lc) * x[r0 * W + c0] + lc * x[r0 * W + c1];
    const double bot = (1 - lc) * x[r1 * W + c0] + lc * x[r1 * W + c1];
    return (1 - lr) * top + lr * bot;
}

static void check_up(int H, int W, float fill) {
    float* x = plane((size_t)H * W);
    float big = 0.0f;
    for (int i = 0; i < H * W; ++i) {
        x[i] = fill != 0.0f ? fill : rnd();
        big = std::fmax(big, std::fabs(x[i]));
    }
    for (int r = 0; r < 2 * H; ++r)
        for (int j0 = 0; j0 < 2 * W; j0 += 4) {
            float q[4];
            gsr::rf_up2_quad(x, H, W, r, j0, q);
            for (int k = 0; k < 4; ++k) {
                const float one = gsr::rf_up2(x, H, W, r, j0 + k);
                n_up++;
                expect(one == q[k], "the quad form is the single form", one, q[k]);
                expect(std::fabs((double)one - up2_ref(x, H, W, r, j0 + k)) <= 4.0 * 0x1p-24 * big + 1e-45,
                       "up2 within 4 * 2^-24 of torch's bilinear", one, up2_ref(x, H, W, r, j0 + k));
                if (fill != 0.0f) expect(one == fill, "a constant plane stays constant", one, fill);
            }
        }
    free(x);
}

static void check_index() {
    for (int n = 1; n <= 5; ++n)
        for (int j = 0; j < 2 * n; ++j) {
            int a, b;
            gsr::rf_up_index(j, n, a, b);
            expect(a >= 0 && a < n && b >= 0 && b < n && std::abs(a - b) <= 1, "taps inside the axis", a, b);
        }
}

static void check_demod() {
    const float eps = 1e-8f, lone = 1.0f / sqrtf(eps);
    const float den = std::numeric_limits<float>::denorm_min(), mn = std::numeric_limits<float>::min();
    const float ss[] = {0.0f, -0.0f, den, -den, mn, 1e-30f, 1.0f, -3.5f, 1e19f, 3e38f};
    for (float s : ss)
        for (float w2 : {0.0f, den, 1e-3f, 1.0f, 1e10f}) {
            const float t = gsr::rf_demod_term(s, w2), d = gsr::rf_demod(t, eps);
            n_demod++;
            if (std::isinf(s * s) && w2 == 0.0f) {  // |s| > 1.8e19 against an all-zero filter: inf * 0
                expect(t != t && d != d, "an overflowing square times a zero table is NaN, as stated", t, d);
                continue;
            }
            expect(t >= 0.0f && !(d != d) && d >= 0.0f && d <= lone, "0 <= d <= rsqrt(eps)", t, d);
            if (std::fabs(s) <= 1e-30f) expect(d == lone, "a vanishing s leaves rsqrt(eps)", s, d);
            if (std::isinf(t)) expect(d == 0.0f, "an overflowing sum gives d = 0", t, d);
            if (std::isfinite(t) && t > 0.0f) {
                const double r = 1.0 / std::sqrt((double)t + (double)eps);
                expect(std::fabs(d - r) <= 3.0 * 0x1p-24 * r, "d within 3 * 2^-24", d, r);
            }
        }
    expect(gsr::rf_demod(0.0f, eps) == lone && std::isfinite(lone), "eps alone under the root", lone, 0);
    expect(std::isinf(gsr::rf_demod(0.0f, 0.0f)), "no eps, no sum: +inf, not a trap", 0, 0);
}

static void check_epilogue() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float xs[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-45f, -1e-45f, 3e38f, -3e38f, inf, -inf, nan};
    for (float x : xs)
        for (float a : {gsr::kRfSqrt2, 0.0f, 1e-40f, 1e4f})
            for (float n : {0.0f, -0.25f})
                for (float b : {0.0f, 0.5f, -0.5f}) {
                    const float y = gsr::rf_epilogue(x, a, n, b);
                    const float v = ((a * x) + n) + b;
                    n_epi++;
                    if (v != v)
                        expect(y != y, "NaN stays NaN", v, y);
                    else
                        expect(y == (v >= 0.0f ? v : 0.2f * v), "LeakyReLU of the stated sum", v, y);
                    const float z = gsr::rf_sft(y, 2.0f, -1.0f);
                    expect((z != z) == (y != y), "y*2 - 1 is NaN only for a NaN y", y, z);
                }
    expect(gsr::kRfSqrt2 == (float)std::sqrt(2.0), "kRfSqrt2 is float32(sqrt 2)", gsr::kRfSqrt2, std::sqrt(2.0));
}

template <int O>
static void check_torgb(int C, int H, int W) {
    const int64_t HW = (int64_t)H * W;
    float* x = plane((size_t)C * HW);
    float* wm = plane((size_t)O * C);
    float* bias = plane(O);
    for (int64_t i = 0; i < C * HW; ++i) x[i] = rnd();
    for (int i = 0; i < O * C; ++i) wm[i] = rnd() * (i % 3 == 0 ? 1e-40f : 1.0f);  // some denormal products
    for (int o = 0; o < O; ++o) bias[o] = rnd();
    for (int64_t e = 0; e < HW; e += 4) {  // the last quad ends at the plane's last float
        gsr::RfQuad acc[O];
        gsr::rf_torgb<O>(wm, bias, x + e, HW, C, acc);
        for (int o = 0; o < O; ++o)
            for (int k = 0; k < 4; ++k) {
                double r = bias[o], mag = std::fabs(bias[o]);
                for (int c = 0; c < C; ++c) {
                    r += (double)wm[o * C + c] * x[c * HW + e + k];
                    mag += std::fabs((double)wm[o * C + c] * x[c * HW + e + k]);
                }
                n_rgb++;
                expect(std::fabs(acc[o].v[k] - r) <= (C + 2) * 0x1p-24 * mag + 1e-38, "torgb within (C + 2) * 2^-24", acc[o].v[k], r);
                const float sg = gsr::ex_sigmoid(acc[o].v[k]);
                expect(sg >= 0.0f && sg <= 1.0f, "sigmoid in [0, 1]", acc[o].v[k], sg);
            }
    }
    free(x);
    free(wm);
    free(bias);
}

int main() {
    srand(7);
    check_index();
    const int hs[] = {1, 2, 3, 5}, ws[] = {2, 4, 6, 14};
    for (int H : hs)
        for (int W : ws) {
            check_up(H, W, 0.0f);
            for (float c : {1.0f, -3.7f, 1.1754944e-38f, 1e-45f, 3e38f, 0.333333343f, 1.99999988f}) check_up(H, W, c);
        }
    check_demod();
    check_epilogue();
    for (int C : {1, 7, 512}) {
        check_torgb<1>(C, 1, 4);
        check_torgb<2>(C, 2, 4);
        check_torgb<3>(C, 3, 8);
        check_torgb<4>(C, 1, 12);
    }
    printf("up2 samples %ld, demod cases %ld, epilogue cases %ld, torgb outputs %ld\n", n_up, n_demod, n_epi, n_rgb);
    if (n_bad) {
        printf("%ld FAILED\n", n_bad);
        return 1;
    }
    printf("clean\n");
    return 0;
}
