// Host check of the UV Gaussian extraction's per-texel functions (guava_renderer_amd/csrc/extract_dev.h):
// the very functions the kernels call, run over hostile inputs under the address and undefined-behaviour
// sanitizers (a float converted to int out of range, a shift out of range, an access outside an array),
// with the mask, the opacity plane, the tile scan and the tables exactly sized on the heap.  Build and
// run on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I guava_renderer_amd/csrc tools/extract_check.cpp -o extract_check && ./extract_check
// Prints its counts and "clean" and exits 0, or the sanitizer's report of the first bad operation
// (non-zero exit); a value that disagrees with the header's stated results also fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "extract_dev.h"

static long n_exp = 0, n_quat = 0, n_layout = 0, n_texel = 0, n_bad = 0;

static void expect(bool ok, const char* what, double a, double b) {
    if (!ok) {
        n_bad++;
        printf("FAIL %s (%g, %g)\n", what, a, b);
    }
}

static void check_logit(float x) {
    const float e = gsr::ex_exp(x), s = gsr::ex_sigmoid(x);
    const float ds = gsr::ex_sigmoid_bwd(x, 1.5f), de = gsr::ex_exp_bwd(x, -2.0f);
    n_exp++;
    (void)de;
    if (x != x) {
        expect(e != e && s != s && ds != ds, "NaN logit must give NaN", e, s);
        return;
    }
    expect(e >= 0.0f && s >= 0.0f && s <= 1.0f, "exp >= 0 and sigmoid in [0, 1]", e, s);
    if (x > gsr::kExOverflow) expect(std::isinf(e) && s == 1.0f, "above the overflow point", e, s);
    if (x < gsr::kExUnderflow) expect(e == 0.0f && s == 0.0f, "below the underflow point", e, s);
    if (std::fabs(x) < 80.0f) {
        const double r = std::exp((double)x);
        expect(std::fabs((double)e - r) <= 2.0 * 0x1p-23 * r, "exp within 2 * 2^-23", e, r);
        const double q = 1.0 / (1.0 + std::exp(-(double)x));
        expect(std::fabs((double)s - q) <= 3.0 * 0x1p-23 * q, "sigmoid within 3 * 2^-23", s, q);
    }
    if (x == 0.0f) expect(e == 1.0f && s == 0.5f && ds == 0.375f, "at zero", e, s);
}

static void check_quat(const float q[4]) {
    float y[4], dx[4], d;
    const float g[4] = {0.5f, -1.0f, 2.0f, 0.25f};
    const float n = gsr::ex_rot_norm(q, d);
    gsr::ex_rot(q, y);
    gsr::ex_rot_bwd(q, g, dx);
    n_quat++;
    expect(d >= gsr::kExRotEps, "d >= eps", d, n);
    bool fin = true, zero = true;
    for (int k = 0; k < 4; ++k) fin = fin && std::isfinite(q[k]), zero = zero && q[k] == 0.0f;
    if (zero) {
        for (int k = 0; k < 4; ++k) {
            expect(y[k] == 0.0f, "zero quaternion gives zeros", y[k], k);
            expect(dx[k] == g[k] / gsr::kExRotEps, "clamp branch: g/eps", dx[k], k);
        }
    }
    if (fin && std::isinf(n))  // the sum of squares overflowed: x / inf
        for (int k = 0; k < 4; ++k) expect(y[k] == 0.0f && dx[k] == 0.0f, "overflowed norm gives zeros", y[k], dx[k]);
    if (fin && n >= 1e-3f && n < 1e18f) {
        double s = 0;
        for (int k = 0; k < 4; ++k) s += (double)y[k] * y[k];
        expect(std::fabs(s - 1.0) < 1e-6, "unit norm", s, n);
    }
}

// The kernels' tile walk over one layout, every array exactly sized: count per tile, scan, slots,
// scatter into tables of exactly N rows, and the pruning's zero rows.
static void check_layout(int T, const std::vector<uint8_t>& mask_v, float threshold) {
    n_layout++;
    const int nt = gsr::ex_tiles(T);
    uint8_t* mask = (uint8_t*)malloc((size_t)T);
    float* opac = (float*)malloc(sizeof(float) * (size_t)T);
    memcpy(mask, mask_v.data(), (size_t)T);
    for (int t = 0; t < T; ++t) opac[t] = -6.0f + 12.0f * (float)((t * 37) % 101) / 100.0f;  // raw logits
    int32_t* u = (int32_t*)malloc(sizeof(int32_t) * (size_t)(nt + 1));
    int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (size_t)(nt + 1));
    for (int pass = 0; pass < 2; ++pass) {
        int32_t* base = pass ? p : u;
        base[0] = 0;
        for (int tile = 0; tile < nt; ++tile) {
            uint64_t ballot = 0;
            for (int lane = 0; lane < gsr::kExTile; ++lane)
                if (gsr::ex_keep(mask, pass ? opac : nullptr, 1, threshold, T, tile * gsr::kExTile + lane))
                    ballot |= (uint64_t)1 << lane;
            base[tile + 1] = base[tile] + __builtin_popcountll(ballot);
        }
    }
    const int N = u[nt], count = p[nt];
    int want_n = 0;
    for (int t = 0; t < T; ++t) want_n += mask[t] != 0;
    expect(N == want_n && count <= N, "scan total", N, want_n);
    // rows written: exactly once each
    uint8_t* hit = (uint8_t*)calloc((size_t)N + 1, 1);  // (+1: malloc(0) is not an array)
    int32_t* row_texel = (int32_t*)malloc(sizeof(int32_t) * ((size_t)N + 1));
    int last = -1;
    for (int tile = 0; tile < nt; ++tile) {
        uint64_t ballot = 0;
        for (int lane = 0; lane < gsr::kExTile; ++lane)
            if (gsr::ex_keep(mask, opac, 1, threshold, T, tile * gsr::kExTile + lane)) ballot |= (uint64_t)1 << lane;
        for (int lane = 0; lane < gsr::kExTile; ++lane) {
            n_texel++;
            if (!((ballot >> lane) & 1)) continue;
            const int row = p[tile] + gsr::ex_rank(ballot, lane);
            expect(row >= 0 && row < N, "row inside the table", row, N);
            if (row < 0 || row >= N) continue;
            hit[row]++;
            row_texel[row] = tile * gsr::kExTile + lane;
            expect(row == last + 1, "rows ascend in texel order", row, last);
            last = row;
        }
        int first, n;
        gsr::ex_zero_rows(u, p, tile, count, first, n);
        expect(n >= 0 && first >= count && first + n <= N, "zero rows inside [count, N)", first, n);
        for (int r = first; r < first + n && r >= 0 && r < N; ++r) hit[r]++;
    }
    for (int r = 0; r < N; ++r) expect(hit[r] == 1, "every row written exactly once", r, hit[r]);
    expect(last + 1 == count, "count", last + 1, count);
    // the staged tile: stride odd and wide enough for every colour count
    for (int C = 3; C <= 64; ++C) {
        const int K = C + 11, s = gsr::ex_stride(K);
        expect((s & 1) == 1 && s >= K && s <= K + 1, "stride", s, K);
    }
    free(mask);
    free(opac);
    free(u);
    free(p);
    free(hit);
    free(row_texel);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float dmin = std::numeric_limits<float>::denorm_min(), fmin = std::numeric_limits<float>::min();
    const float fmax = std::numeric_limits<float>::max();
    const float logits[] = {nan, inf, -inf, 200.0f, -200.0f, 0.0f, -0.0f, dmin, -dmin, fmin, -fmin, fmax, -fmax,
                            88.72283f, 88.72284f, 88.7229f, -87.3f, -87.4f, -88.8f, -103.2f, -103.9f, -104.0f,
                            -104.1f, 1e-8f, -1e-8f, 0.34657359f, -0.34657359f, 0.34657362f, 1.0f, -1.0f, 17.0f, -17.0f,
                            3e9f, -3e9f, 2147483648.0f, -2147483904.0f};
    for (float x : logits) check_logit(x);
    for (int i = -10500; i <= 9000; ++i) check_logit(0.01f * (float)i + 0.003f);

    const float comps[] = {0.0f, -0.0f, dmin, -dmin, 1e-20f, 3e-13f, 1e-12f, 1.0f, -2.5f, 1e19f, -1e19f, fmax, inf, -inf, nan};
    for (float a : comps)
        for (float b : comps)
            for (float c : comps)
                for (float d : comps) {
                    const float q[4] = {a, b, c, d};
                    check_quat(q);
                }

    const int sizes[] = {1, 63, 64, 65, 128, 1000, 2304, 4097};
    for (int T : sizes)
        for (int kind = 0; kind < 6; ++kind) {
            std::vector<uint8_t> m((size_t)T, 0);
            if (kind == 1) std::fill(m.begin(), m.end(), (uint8_t)1);
            if (kind == 2) m[0] = 1;
            if (kind == 3) m[(size_t)T - 1] = 1;
            if (kind == 4)
                for (int t = 0; t < T; ++t) m[(size_t)t] = (uint8_t)(((t * 2654435761u) >> 7) % 4 != 0);
            if (kind == 5)
                for (int t = 0; t < T; ++t) m[(size_t)t] = (uint8_t)((t % 193) < 65 ? 255 : 0);
            const float thresholds[] = {-1.0f, 0.001f, 0.5f, 1.0f, nan};
            for (float thr : thresholds) check_layout(T, m, thr);
        }
    // texels outside [0, T) are never read
    {
        uint8_t* one = (uint8_t*)malloc(1);
        one[0] = 1;
        expect(!gsr::ex_keep(one, nullptr, 0, 0.0f, 1, 1) && !gsr::ex_keep(one, nullptr, 0, 0.0f, 1, -1) &&
                   gsr::ex_keep(one, nullptr, 0, 0.0f, 1, 0),
               "texel range", 0, 0);
        free(one);
    }
    printf("logits %ld, quaternions %ld, layouts %ld (texel slots %ld), wrong results %ld\n", n_exp, n_quat, n_layout,
           n_texel, n_bad);
    if (n_bad) return 1;
    printf("clean\n");
    return 0;
}
