// Host check of the feature lifting's per-sample guards (guava_renderer_amd/csrc/lift_dev.h): the very
// functions the kernels call, run over hostile inputs with every array exactly sized on the heap, so
// that the address and undefined-behaviour sanitizers see any access or conversion the guards let
// through (a non-finite or huge coordinate converted to int, a tap outside the image, a face or vertex
// index outside its array).  Build and run on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I guava_renderer_amd/csrc tools/lift_check.cpp -o lift_check && ./lift_check
// Prints "clean" and exits 0, or the sanitizer's report of the first bad access (non-zero exit); a value
// that disagrees with the guards' stated results (zeros where zeros are promised) also fails.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "lift_dev.h"

using gsr::LiftSample;

static long n_samples = 0, n_zero = 0, n_partial = 0, n_bad = 0;

static float *plane = nullptr, *grad = nullptr;  // exactly W*H floats each (set_image)

static void set_image(int W, int H) {
    free(plane);
    free(grad);
    plane = (float*)malloc(sizeof(float) * (size_t)W * H);
    grad = (float*)calloc((size_t)W * H, sizeof(float));
    for (int i = 0; i < W * H; ++i) plane[i] = 1.0f + (float)(i % 7);
}

// loads every in-image tap of `s` from the exactly sized W*H plane, as the forward does, and touches the
// same elements of the exactly sized gradient plane, as the backward's scatter does
static float run_taps(const LiftSample& s, int W, int H) {
    (void)H;
    float v = 0.0f;
    if (s.mask) {
        v = gsr::lift_sample_plane(s, plane, W);
        for (int k = 0; k < 4; ++k)
            if (s.mask & (1u << k)) grad[gsr::lift_tap_offset(s, k, W)] += s.w[k];
    }
    n_samples++;
    n_zero += s.mask == 0u;
    n_partial += s.mask != 0u && s.mask != 15u;
    return v;
}

static void expect(bool ok, const char* what, double a, double b) {
    if (!ok) {
        n_bad++;
        printf("FAIL %s (%g, %g)\n", what, a, b);
    }
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sizes[][2] = {{1, 1}, {2, 3}, {7, 5}, {24, 16}, {512, 512}, {16384, 2}};
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        const float fw = (float)W, fh = (float)H;
        set_image(W, H);
        const float xs[] = {nan,   inf,   -inf,        1e30f,       -1e30f,     3e9f,        -3e9f,       -1.0f,
                            -0.5f, 0.0f,  fw - 1.0f,   fw - 0.5f,   fw,         -1.0000001f, -0.9999999f, 0.5f,
                            std::nextafterf(fw, 0.0f), std::nextafterf(fw, 2 * fw), fw - 1.5f, 2147483648.0f, -2147483904.0f,
                            1e-45f, -1e-45f, -0.0f};
        const float ys[] = {nan, inf, -inf, 1e30f, -1e30f, -1.0f, -0.5f, 0.0f, fh - 1.0f, fh - 0.5f, fh,
                            std::nextafterf(fh, 0.0f), std::nextafterf(-1.0f, 0.0f), 0.25f};
        for (float ix : xs)
            for (float iy : ys)
                for (int border = 0; border < 2; ++border) {
                    const LiftSample s = gsr::lift_taps(ix, iy, W, H, border);
                    const float v = run_taps(s, W, H);
                    const bool fin = std::isfinite(ix) && std::isfinite(iy);
                    const bool inside = ix > -1.0f && ix < fw && iy > -1.0f && iy < fh;
                    if (!fin) expect(s.mask == 0u && v == 0.0f, "non-finite coordinate must give zeros", ix, iy);
                    if (fin && border) expect((s.mask & 1u) != 0u, "border mode always has tap 00", ix, iy);
                    if (fin && !border && !inside) expect(s.mask == 0u, "zeros mode outside must give zeros", ix, iy);
                    if (fin && !border && inside) expect(s.x0 >= -1 && s.x0 < W && s.y0 >= -1 && s.y0 < H, "x0/y0 range", ix, iy);
                }
        // through the projection: hostile vertices and cameras
        const float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const float cs[] = {nan, inf, -inf, 1e30f, -1e30f, 0.0f, -1e-7f, 1.0f, -1.0f, 1e-30f, 3.4e38f};
        for (float x : cs)
            for (float y : cs)
                for (float z : cs) {
                    const float vert[3] = {x, y, z};
                    float xn, yn;
                    const LiftSample s = gsr::lift_vertex_sample(vert, M, 1.0f / 24.0f, 1.0f / 24.0f, W, H, xn, yn);
                    run_taps(s, W, H);
                    float ix, iy;
                    gsr::lift_project(M, 0.5f, 0.5f, W, H, x, y, z, xn, yn, ix, iy);
                    run_taps(gsr::lift_taps(ix, iy, W, H, 0), W, H);
                }
    }
    // the UV path's index guards: every array exactly sized
    {
        const int V = 5, F = 4, W = 8, H = 8;
        const int face_cases[] = {-1, INT_MIN, -2, 0, 1, 2, 3, F, F + 1, INT_MAX};
        const int T = (int)(sizeof(face_cases) / sizeof(int));
        set_image(W, H);
        const int vidx[] = {0, V - 1, -1, V, INT_MAX, INT_MIN};
        float* verts = (float*)malloc(sizeof(float) * 3 * V);
        for (int i = 0; i < 3 * V; ++i) verts[i] = 0.01f * (float)i;
        for (int i = 0; i < V; ++i) verts[3 * i + 2] = 2.0f;
        verts[3] = nan;  // vertex 1
        int32_t* texel_face = (int32_t*)malloc(sizeof(int32_t) * T);
        float* bary = (float*)malloc(sizeof(float) * 3 * T);
        for (int t = 0; t < T; ++t) {
            texel_face[t] = face_cases[t];
            bary[3 * t] = 0.25f, bary[3 * t + 1] = 0.5f, bary[3 * t + 2] = 0.25f;
        }
        uint8_t* vis = (uint8_t*)malloc(F);
        const float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        for (int bad : vidx)
            for (int slot = 0; slot < 3; ++slot)
                for (int with_vis = 0; with_vis < 2; ++with_vis) {
                    int32_t* faces = (int32_t*)malloc(sizeof(int32_t) * 3 * F);
                    for (int i = 0; i < 3 * F; ++i) faces[i] = (i * 2) % V;
                    faces[3 * 2 + slot] = bad;  // face 2 carries the hostile index
                    faces[3 * 3] = 1;           // face 3 uses the NaN vertex
                    for (int f = 0; f < F; ++f) vis[f] = (uint8_t)(f != 1);
                    for (int t = 0; t < T; ++t) {
                        const LiftSample s = gsr::lift_uv_sample(verts, faces, texel_face, bary, with_vis ? vis : nullptr, M,
                                                                 0.5f, 0.5f, V, F, W, H, t);
                        run_taps(s, W, H);
                        const int f = face_cases[t];
                        if (f < 0 || f >= F) expect(s.mask == 0u, "face outside [0, F) must give zeros", f, t);
                        if (f == 2 && (bad < 0 || bad >= V)) expect(s.mask == 0u, "vertex index outside [0, V)", bad, t);
                        if (f == 3) expect(s.mask == 0u, "NaN vertex must give zeros", f, t);
                        if (f == 1 && with_vis) expect(s.mask == 0u, "invisible face must give zeros", f, t);
                        if (f == 0) expect(s.mask != 0u, "a sound texel samples", f, t);
                    }
                    free(faces);
                }
        free(verts);
        free(texel_face);
        free(bary);
        free(vis);
    }
    free(plane);
    free(grad);
    printf("samples %ld, all-zero %ld, with one to three taps outside %ld, wrong results %ld\n", n_samples, n_zero,
           n_partial, n_bad);
    if (n_bad) return 1;
    printf("clean\n");
    return 0;
}
