// Host check of the refiner decoder's backward arithmetic (guava_renderer_amd/csrc/refiner_dev.h): the
// very functions refiner_bwd.hip's kernels call, run on the CPU under the address and
// undefined-behaviour sanitizers, every plane exactly sized on the heap so that a tap outside its plane
// is an error:
//   up2T      one-row, two-column and H != W planes; the adjoint identity <up2(x), g> = <x, up2T(g)> in
//             double; a constant g gives every input pixel exactly 4*g; the sigmoid-fused reader
//   epilogue  backward over +-0, subnormals, +-3e38, +-inf and NaN: the forward's branch, no trap
//   torgb     backward at C in {1, 7, 512}, O = 1..4, the last quad ending on the plane's last float
// Build and run on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I guava_renderer_amd/csrc tools/refiner_bwd_check.cpp -o refiner_bwd_check && ./refiner_bwd_check
// Prints its counts and "clean" and exits 0, or the sanitizer's report of the first bad operation
// (non-zero exit); a value that disagrees with the header's stated results also fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "refiner_dev.h"

static long n_up = 0, n_epi = 0, n_rgb = 0, n_bad = 0;

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

// h x w input plane, 2h x 2w output plane (2w a multiple of 4)
static void check_up2t(int h, int w, float fill) {
    const int H = 2 * h, W = 2 * w;
    float* x = plane((size_t)h * w);
    float* g = plane((size_t)H * W);
    float* y = plane((size_t)H * W);  // a sigmoid output for the fused reader
    for (int i = 0; i < h * w; ++i) x[i] = rnd();
    for (int i = 0; i < H * W; ++i) {
        g[i] = fill != 0.0f ? fill : rnd();
        y[i] = 0.5f + 0.2f * rnd();
    }
    double lhs = 0.0, rhs = 0.0, mag = 0.0;
    for (int r = 0; r < H; ++r)
        for (int j0 = 0; j0 < W; j0 += 4) {
            float q[4];
            gsr::rf_up2_quad(x, h, w, r, j0, q);
            for (int k = 0; k < 4; ++k) {
                lhs += (double)q[k] * g[r * W + j0 + k];
                mag += std::fabs((double)q[k] * g[r * W + j0 + k]);
            }
        }
    for (int i = 0; i < h; ++i)
        for (int c = 0; c < w; ++c) {
            const float t = gsr::rf_up2t(gsr::RfAtPlain{g, W}, H, W, i, c);
            n_up++;
            rhs += (double)x[i * w + c] * t;
            if (fill != 0.0f) expect(t == 4.0f * fill, "a constant g gives exactly 4*g", t, 4.0f * fill);
            // the fused reader: the same gather over g * (y * (1 - y)) computed first
            const float ts = gsr::rf_up2t(gsr::RfAtAcc{g, y, W}, H, W, i, c);
            const float tp = gsr::rf_up2t(gsr::RfAtAcc{g, nullptr, W}, H, W, i, c);
            expect(tp == t, "the plain reader and the acc reader without y agree", tp, t);
            expect(std::isfinite(ts), "the sigmoid reader is finite", ts, 0);
        }
    // each side rounds every sample within 4 * 2^-24 of its exact value
    expect(std::fabs(lhs - rhs) <= 16.0 * 0x1p-24 * mag + 1e-30, "<up2(x), g> = <x, up2T(g)>", lhs, rhs);
    free(x);
    free(g);
    free(y);
}

static void check_fold() {
    for (int n = 2; n <= 10; n += 2) {
        expect(gsr::rf_fold(-1, n) == 0 && gsr::rf_fold(n, n) == n - 1 && gsr::rf_fold(n - 1, n) == n - 1 &&
                   gsr::rf_fold(0, n) == 0,
               "an index one step outside folds onto the border", n, 0);
        // every (output, input) tap pair of the forward is one of the transposed gather's pairs
        const int h = n / 2;
        for (int j = 0; j < n; ++j) {
            int near_i, far_i;
            gsr::rf_up_index(j, h, near_i, far_i);
            for (int pass = 0; pass < 2; ++pass) {
                const int i = pass ? far_i : near_i;
                bool found = false;
                for (int k = 0; k < 4; ++k) found = found || gsr::rf_fold(2 * i - 1 + k, n) == j;
                expect(found, "a forward tap is gathered back", j, i);
            }
        }
    }
}

static void check_epilogue() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float xs[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-45f, -1e-45f, 1e-39f, -1e-39f, 3e38f, -3e38f, inf, -inf, nan};
    for (float x : xs)
        for (float gy : xs)
            for (float a : {gsr::kRfSqrt2, 0.0f, 1e-40f, 1e4f})
                for (int sft = 0; sft < 2; ++sft)
                    for (int post = 0; post < 2; ++post) {
                        const float nw = 0.7f, noise = -0.25f, bias = 0.5f, scale = 1.5f, shift = -0.5f, ps = -2.0f;
                        const gsr::RfEpiGrad r =
                            gsr::rf_epilogue_bwd(gy, x, a, nw, noise, bias, sft != 0, scale, shift, post != 0, ps);
                        n_epi++;
                        const float v = ((a * x) + (nw * noise)) + bias;
                        const float l = gsr::rf_epilogue(x, a, nw * noise, bias);
                        const float g1 = post ? gy * ps : gy, gl = sft ? g1 * scale : g1;
                        const float gv = v >= 0.0f ? gl : 0.2f * gl;  // a NaN v takes the 0.2 branch
                        auto same = [](float p, float q) { return (p != p && q != q) || p == q; };
                        expect(same(r.g_v, gv), "g_v follows the forward's branch", r.g_v, gv);
                        expect(same(r.g_x, a * gv), "g_x = a * g_v", r.g_x, a * gv);
                        expect(same(r.g_shift, g1) && same(r.g_scale, g1 * l), "g_shift = g1, g_scale = g1 * l", r.g_shift, g1);
                        expect(same(r.t_post, gy * (sft ? gsr::rf_sft(l, scale, shift) : l)), "g_post's term", r.t_post, 0);
                        expect(same(r.t_x, gv * x), "g_d's term", r.t_x, gv * x);
                        const double tn = gsr::rf_noise_term(r.g_v, noise);
                        expect((tn != tn && gv != gv) || tn == (double)gv * (double)noise, "g_nw's term, exact in double", tn, gv);
                        if (v != v && gl == gl && std::isfinite(gl)) expect(r.g_v == 0.2f * gl, "NaN v: slope 0.2", r.g_v, gl);
                    }
    gsr::RfQuad t = {{1.0f, 2.0f, 3.0f, 4.0f}}, u = {{0.5f, 0.25f, 2.0f, 1.0f}};
    expect(gsr::rf_quad_sum(t) == 10.0f && gsr::rf_quad_dot(t, u) == 11.0f, "the quad sums", gsr::rf_quad_sum(t),
           gsr::rf_quad_dot(t, u));
    expect(gsr::rf_demod_bwd(2.0f, 3.0f) == -12.0f, "t = -0.5 * d^3 * g_d", gsr::rf_demod_bwd(2.0f, 3.0f), -12.0);
    expect(gsr::rf_chunks(1) == 1 && gsr::rf_chunks(256) == 1 && gsr::rf_chunks(257) == 2 && gsr::rf_chunks(65536) == 256,
           "chunks of 256 lane-quads", 0, 0);
}

template <int O>
static void check_torgb(int C, int H, int W) {
    const int64_t HW = (int64_t)H * W;
    float* x = plane((size_t)C * HW);
    float* gx = plane((size_t)C * HW);
    float* gout = plane((size_t)O * HW);
    float* y = plane((size_t)O * HW);
    float* wm = plane((size_t)O * C);
    std::vector<double> m((size_t)O * C, 0.0), mref((size_t)O * C, 0.0), mmag((size_t)O * C, 0.0);
    for (int64_t i = 0; i < C * HW; ++i) x[i] = rnd();
    for (int64_t i = 0; i < O * HW; ++i) {
        gout[i] = rnd();
        y[i] = 0.5f + 0.2f * rnd();
    }
    for (int i = 0; i < O * C; ++i) wm[i] = rnd() * (i % 3 == 0 ? 1e-40f : 1.0f);  // some denormal products
    for (int64_t e = 0; e < HW; e += 4) {  // the last quad ends at the plane's last float
        gsr::RfQuad g[O];
        for (int o = 0; o < O; ++o) {
            g[o] = gsr::rf_load(gout + o * HW + e);
            const gsr::RfQuad yq = gsr::rf_load(y + o * HW + e);
            for (int k = 0; k < 4; ++k) g[o].v[k] = gsr::rf_sigmoid_bwd(g[o].v[k], yq.v[k]);
        }
        for (int c = 0; c < C; ++c) {
            const gsr::RfQuad xq = gsr::rf_load(x + c * HW + e);
            const gsr::RfQuad r = gsr::rf_torgb_bwd_x<O>(wm, C, c, g);
            gsr::rf_store(gx + c * HW + e, r);
            for (int k = 0; k < 4; ++k) {
                double ref = 0.0, mag = 0.0;
                for (int o = 0; o < O; ++o) {
                    ref += (double)wm[o * C + c] * g[o].v[k];
                    mag += std::fabs((double)wm[o * C + c] * g[o].v[k]);
                }
                n_rgb++;
                expect(std::fabs(r.v[k] - ref) <= (O + 1) * 0x1p-24 * mag + 1e-38, "g_x within (O + 1) * 2^-24", r.v[k], ref);
            }
            for (int o = 0; o < O; ++o) {
                m[o * C + c] += gsr::rf_quad_dot(g[o], xq);
                for (int k = 0; k < 4; ++k) {
                    mref[o * C + c] += (double)g[o].v[k] * xq.v[k];
                    mmag[o * C + c] += std::fabs((double)g[o].v[k] * xq.v[k]);
                }
            }
        }
    }
    for (int i = 0; i < O * C; ++i)
        expect(std::fabs(m[i] - mref[i]) <= 4.0 * 0x1p-24 * mmag[i] + 1e-38, "the lane's terms of m[o,c]", m[i], mref[i]);
    free(x);
    free(gx);
    free(gout);
    free(y);
    free(wm);
}

int main() {
    srand(11);
    check_fold();
    const int hs[] = {1, 2, 3, 5}, ws[] = {2, 4, 6, 14};
    for (int h : hs)
        for (int w : ws) {
            check_up2t(h, w, 0.0f);
            for (float c : {1.0f, -3.5f, 0.15625f, 1.1754944e-38f, 0x1p125f}) check_up2t(h, w, c);
        }
    check_epilogue();
    for (int C : {1, 7, 512}) {
        check_torgb<1>(C, 1, 4);
        check_torgb<2>(C, 2, 4);
        check_torgb<3>(C, 3, 8);
        check_torgb<4>(C, 1, 12);
    }
    printf("up2T samples %ld, epilogue backward cases %ld, torgb backward outputs %ld\n", n_up, n_epi, n_rgb);
    if (n_bad) {
        printf("%ld FAILED\n", n_bad);
        return 1;
    }
    printf("clean\n");
    return 0;
}
