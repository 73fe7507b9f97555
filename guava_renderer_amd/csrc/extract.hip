// extract.hip -- UV Gaussian extraction (include/gsr_extract.h) for gfx950: the UV point decoder's maps
// to the per-Gaussian tables, with the head activations, the mask gather, the RGB sigmoid and the
// opacity pruning fused, and the gradient back into the maps.  The per-texel arithmetic and the tile /
// slot arithmetic are extract_dev.h's, shared with the host check.
//
// Work unit everywhere: a tile of 64 consecutive texels, one per lane.  A kept lane's table row is
// tile_base[tile] + popcount(ballot(keep) & lanes_below): no index list, nothing to validate, no atomics.
//
//   k_extract_count    a wave per tile: popcount of the keep ballot -> tile_base[1 + tile]
//   k_extract_scan     one workgroup: in-place inclusive scan of those counts (tile_base[0] = 0)
//   k_extract_planar   a workgroup per (frame, tile).  Lanes over texels read the planes (a tile's 256 B
//                      per plane is one request; wave w takes the planes w, w + 4, ..., the wave that
//                      meets the first rotation plane takes all four), activate in registers and stage
//                      the values at the lane's rank in an LDS tile of odd row stride; then the threads
//                      walk the tile's contiguous row range of each table with dword stores.
//   k_extract_rows     rows in, rows out: the ranks go through LDS, the rows are copied directly.
//   k_extract_planar_bwd / k_extract_rows_bwd   the reverse: the tile's row range of the five gradient
//                      tables -> LDS, one lane per texel applies the activation's gradient from the
//                      re-read raw planes and stores dx, or +0 outside the mask, to every plane.
// A pruning forward also writes the zero rows: tile i zeroes the rows that its dropped texels would have
// had behind the kept ones (ex_zero_rows), which over the tiles is exactly [count, N).
#include <hip/hip_runtime.h>

#include "../../include/gsr.h"
#include "../../include/gsr_extract.h"
#include "extract_dev.h"
#include "gsr_internal.h"

namespace gsr {

constexpr int kExBlock = 256;

struct ExArgs {
    int B, T, N, C, ntiles;
    int rgb;
    float threshold;
    const uint8_t* mask;
    const int32_t* tile_base;       // placement
    const int32_t* tile_base_mask;  // pruning: the unpruned scan
    GsrExtractSet in;               // maps (forward), maps (backward)
    GsrExtractSet tab;              // tables (forward), table gradients (backward)
    GsrExtractSet dmap;             // backward: map gradients
    const int32_t* texel_face;
    const float* texel_bary;
    int32_t* binding_face;
    float* face_bary;
};

// f(row, col) for every element of a rows x W row-major range, the 256 threads over consecutive elements
template <class F>
__device__ __forceinline__ void ex_for_elements(int rows, int W, F f) {
    int row = (int)threadIdx.x / W, col = (int)threadIdx.x - row * W;
    const int dr = kExBlock / W, dc = kExBlock - dr * W;
    while (row < rows) {
        f(row, col);
        row += dr;
        col += dc;
        if (col >= W) {
            col -= W;
            ++row;
        }
    }
}

struct ExTile {
    int b, tile, t, lane, wave, rank, cnt, base;
    bool keep;
};

template <bool PRUNE, bool RAW>
__device__ __forceinline__ ExTile ex_tile(const ExArgs& a) {
    ExTile x;
    x.tile = (int)(blockIdx.x % (unsigned)a.ntiles);
    x.b = (int)(blockIdx.x / (unsigned)a.ntiles);
    x.lane = threadIdx.x & 63;
    x.wave = threadIdx.x >> 6;
    x.t = x.tile * kExTile + x.lane;
    x.keep = ex_keep(a.mask, PRUNE ? a.in.opacities : nullptr, RAW ? 1 : 0, a.threshold, a.T, x.t);
    const uint64_t ballot = __ballot(x.keep);
    x.rank = ex_rank(ballot, x.lane);
    x.cnt = __popcll(ballot);
    x.base = a.tile_base[x.tile];
    return x;
}

// binding_face / face_bary of the kept texels (frame 0's workgroups, wave 0), and a pruning tile's zero rows
template <bool PRUNE>
__device__ __forceinline__ void ex_binding_and_zeros(const ExArgs& a, const ExTile& x) {
    if (a.binding_face && x.b == 0 && x.wave == 0 && x.keep) {
        const int row = x.base + x.rank;
        if (row >= 0 && row < a.N) {
            a.binding_face[row] = a.texel_face[x.t];
            for (int k = 0; k < 3; ++k) a.face_bary[3 * (int64_t)row + k] = a.texel_bary[3 * (int64_t)x.t + k];
        }
    }
    if (PRUNE) {
        int first, n;
        ex_zero_rows(a.tile_base_mask, a.tile_base, x.tile, a.tile_base[a.ntiles], first, n);
        if (n <= 0) return;
        const int N = a.N;
        auto zero = [&](float* dst, int W) {
            if (!dst) return;
            ex_for_elements(n, W, [&](int row, int col) {
                const int r = first + row;
                if (r >= 0 && r < N) dst[((int64_t)x.b * N + r) * W + col] = 0.0f;
            });
        };
        zero(a.tab.colors, a.C);
        zero(a.tab.opacities, 1);
        zero(a.tab.scales, 3);
        zero(a.tab.rotations, 4);
        zero(a.tab.local_pos, 3);
        if (x.b == 0 && a.binding_face) {
            zero(a.face_bary, 3);
            ex_for_elements(n, 1, [&](int row, int) {
                const int r = first + row;
                if (r >= 0 && r < N) a.binding_face[r] = 0;
            });
        }
    }
}

__global__ void __launch_bounds__(kExBlock) k_extract_count(int T, int ntiles, int raw, float threshold,
                                                            const uint8_t* __restrict__ mask,
                                                            const float* __restrict__ opacity,
                                                            int32_t* __restrict__ tile_base) {
    const int tile = (int)blockIdx.x * (kExBlock / kExTile) + (int)(threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const int lane = threadIdx.x & 63;
    const bool keep = ex_keep(mask, opacity, raw, threshold, T, tile * kExTile + lane);
    const uint64_t ballot = __ballot(keep);
    if (lane == 0) tile_base[1 + tile] = __popcll(ballot);
}

__global__ void __launch_bounds__(1024) k_extract_scan(int ntiles, int32_t* __restrict__ tile_base) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    if (threadIdx.x == 0) tile_base[0] = 0;
    for (int c0 = 0; c0 < ntiles; c0 += 1024) {
        const int i = c0 + (int)threadIdx.x;
        int v = i < ntiles ? tile_base[1 + i] : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(v, d);
            if (lane >= d) v += y;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        if (wave == 0) {
            int w = lane < 16 ? wsum[lane] : 0;
            for (int d = 1; d < 16; d <<= 1) {
                const int y = __shfl_up(w, d);
                if (lane >= d) w += y;
            }
            if (lane < 16) wsum[lane] = w;
        }
        __syncthreads();
        const int off = wave ? wsum[wave - 1] : 0;
        if (i < ntiles) tile_base[1 + i] = carry + off + v;
        carry += wsum[15];
        __syncthreads();
    }
}

template <bool PRUNE>
__global__ void __launch_bounds__(kExBlock) k_extract_planar(ExArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ExTile x = ex_tile<PRUNE, true>(a);
    const int C = a.C, K = C + 11, stride = ex_stride(K), N = a.N;
    const int64_t T = a.T;
    if (a.tab.colors && x.cnt > 0) {
        if (x.keep) {
            float* row = lds + x.rank * stride;
            for (int p = x.wave; p < K; p += 4) {
                if (p < C) {
                    const float v = a.in.colors[((int64_t)x.b * C + p) * T + x.t];
                    row[p] = (a.rgb && p < 3) ? ex_sigmoid(v) : v;
                } else if (p == C) {
                    row[p] = ex_sigmoid(a.in.opacities[(int64_t)x.b * T + x.t]);
                } else if (p <= C + 3) {
                    row[p] = ex_exp(a.in.scales[((int64_t)x.b * 3 + (p - C - 1)) * T + x.t]);
                } else if (p == C + 4) {
                    float q[4], y[4];
                    for (int k = 0; k < 4; ++k) q[k] = a.in.rotations[((int64_t)x.b * 4 + k) * T + x.t];
                    ex_rot(q, y);
                    for (int k = 0; k < 4; ++k) row[p + k] = y[k];
                } else if (p >= C + 8) {
                    row[p] = a.in.local_pos[((int64_t)x.b * 3 + (p - C - 8)) * T + x.t];
                }
            }
        }
        __syncthreads();
        auto store = [&](float* dst, int W, int c0) {
            ex_for_elements(x.cnt, W, [&](int row, int col) {
                const int r = x.base + row;
                if (r >= 0 && r < N) dst[((int64_t)x.b * N + r) * W + col] = lds[row * stride + c0 + col];
            });
        };
        store(a.tab.colors, C, 0);
        store(a.tab.opacities, 1, C);
        store(a.tab.scales, 3, C + 1);
        store(a.tab.rotations, 4, C + 4);
        store(a.tab.local_pos, 3, C + 8);
    }
    ex_binding_and_zeros<PRUNE>(a, x);
}

template <bool PRUNE>
__global__ void __launch_bounds__(kExBlock) k_extract_rows(ExArgs a) {
    __shared__ int s_rank[kExTile];
    const ExTile x = ex_tile<PRUNE, false>(a);
    const int C = a.C, N = a.N, T = a.T;
    if (a.tab.colors && x.cnt > 0) {
        if (x.wave == 0) s_rank[x.lane] = x.keep ? x.rank : -1;
        __syncthreads();
        const int t0 = x.tile * kExTile;
        const int rows = min(kExTile, T - t0);
        auto copy = [&](const float* src, float* dst, int W, bool rgb) {
            ex_for_elements(rows, W, [&](int row, int col) {
                const int s = s_rank[row];
                const int r = x.base + s;
                if (s < 0 || r < 0 || r >= N) return;
                const float v = src[((int64_t)x.b * T + t0 + row) * W + col];
                dst[((int64_t)x.b * N + r) * W + col] = (rgb && col < 3) ? ex_sigmoid(v) : v;
            });
        };
        copy(a.in.colors, a.tab.colors, C, a.rgb != 0);
        copy(a.in.opacities, a.tab.opacities, 1, false);
        copy(a.in.scales, a.tab.scales, 3, false);
        copy(a.in.rotations, a.tab.rotations, 4, false);
        copy(a.in.local_pos, a.tab.local_pos, 3, false);
    }
    ex_binding_and_zeros<PRUNE>(a, x);
}

__global__ void __launch_bounds__(kExBlock) k_extract_planar_bwd(ExArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ExTile x = ex_tile<false, true>(a);
    const int C = a.C, K = C + 11, stride = ex_stride(K), N = a.N;
    const int64_t T = a.T;
    if (x.cnt > 0) {
        auto load = [&](const float* src, int W, int c0) {
            ex_for_elements(x.cnt, W, [&](int row, int col) {
                const int r = x.base + row;
                lds[row * stride + c0 + col] = (src && r >= 0 && r < N) ? src[((int64_t)x.b * N + r) * W + col] : 0.0f;
            });
        };
        load(a.tab.colors, C, 0);
        load(a.tab.opacities, 1, C);
        load(a.tab.scales, 3, C + 1);
        load(a.tab.rotations, 4, C + 4);
        load(a.tab.local_pos, 3, C + 8);
    }
    __syncthreads();
    if (x.t >= a.T) return;
    const float* g = lds + x.rank * stride;  // read only by kept lanes
    for (int p = x.wave; p < K; p += 4) {
        if (p < C) {
            if (!a.dmap.colors) continue;
            const int64_t e = ((int64_t)x.b * C + p) * T + x.t;
            float d = 0.0f;
            if (x.keep) d = (a.rgb && p < 3) ? ex_sigmoid_bwd(a.in.colors[e], g[p]) : g[p];
            a.dmap.colors[e] = d;
        } else if (p == C) {
            if (!a.dmap.opacities) continue;
            const int64_t e = (int64_t)x.b * T + x.t;
            a.dmap.opacities[e] = x.keep ? ex_sigmoid_bwd(a.in.opacities[e], g[p]) : 0.0f;
        } else if (p <= C + 3) {
            if (!a.dmap.scales) continue;
            const int64_t e = ((int64_t)x.b * 3 + (p - C - 1)) * T + x.t;
            a.dmap.scales[e] = x.keep ? ex_exp_bwd(a.in.scales[e], g[p]) : 0.0f;
        } else if (p == C + 4) {
            if (!a.dmap.rotations) continue;
            float dx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (x.keep) {
                float q[4], gq[4];
                for (int k = 0; k < 4; ++k) {
                    q[k] = a.in.rotations[((int64_t)x.b * 4 + k) * T + x.t];
                    gq[k] = g[p + k];
                }
                ex_rot_bwd(q, gq, dx);
            }
            for (int k = 0; k < 4; ++k) a.dmap.rotations[((int64_t)x.b * 4 + k) * T + x.t] = dx[k];
        } else if (p >= C + 8) {
            if (!a.dmap.local_pos) continue;
            a.dmap.local_pos[((int64_t)x.b * 3 + (p - C - 8)) * T + x.t] = x.keep ? g[p] : 0.0f;
        }
    }
}

__global__ void __launch_bounds__(kExBlock) k_extract_rows_bwd(ExArgs a) {
    __shared__ int s_rank[kExTile];
    const ExTile x = ex_tile<false, false>(a);
    const int C = a.C, N = a.N, T = a.T;
    if (x.wave == 0) s_rank[x.lane] = x.keep ? x.rank : -1;
    __syncthreads();
    const int t0 = x.tile * kExTile;
    const int rows = min(kExTile, T - t0);
    auto scatter = [&](const float* src, float* dst, int W, bool rgb) {
        if (!dst) return;
        ex_for_elements(rows, W, [&](int row, int col) {
            const int s = s_rank[row];
            const int r = x.base + s;
            const int64_t e = ((int64_t)x.b * T + t0 + row) * W + col;
            float d = 0.0f;
            if (s >= 0 && r >= 0 && r < N) {
                const float gv = src ? src[((int64_t)x.b * N + r) * W + col] : 0.0f;
                d = (rgb && col < 3) ? ex_sigmoid_bwd(a.in.colors[e], gv) : gv;
            }
            dst[e] = d;
        });
    };
    scatter(a.tab.colors, a.dmap.colors, C, a.rgb != 0);
    scatter(a.tab.opacities, a.dmap.opacities, 1, false);
    scatter(a.tab.scales, a.dmap.scales, 3, false);
    scatter(a.tab.rotations, a.dmap.rotations, 4, false);
    scatter(a.tab.local_pos, a.dmap.local_pos, 3, false);
}

static int ex_done() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

static bool ex_sizes_ok(int B, int T, int N, int C, int layout) {
    if (B <= 0 || T <= 0 || N < 0 || N > T || C < 3 || C > 64) return false;
    if (layout != GSR_EXTRACT_PLANAR_RAW && layout != GSR_EXTRACT_ROWS_ACTIVATED) return false;
    return (int64_t)B * T * (C + 11) < ((int64_t)1 << 31);
}

static bool ex_set_ok(const GsrExtractSet* s) {
    return s && s->colors && s->opacities && s->scales && s->rotations && s->local_pos;
}

static size_t ex_lds_bytes(int C) { return sizeof(float) * (size_t)kExTile * ex_stride(C + 11); }

static int ex_prepare(int T, int raw, const uint8_t* mask, const float* opacities, float threshold, int32_t* tile_base,
                      hipStream_t s) {
    const int ntiles = ex_tiles(T);
    const int per = kExBlock / kExTile;
    hipLaunchKernelGGL(k_extract_count, dim3((unsigned)((ntiles + per - 1) / per)), dim3(kExBlock), 0, s, T, ntiles, raw,
                       threshold, mask, opacities, tile_base);
    hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(1024), 0, s, ntiles, tile_base);
    return ex_done();
}

template <bool PRUNE>
static int ex_forward(const ExArgs& a, int layout, bool tables, hipStream_t s) {
    const unsigned grid = (unsigned)((int64_t)(tables ? a.B : 1) * a.ntiles);
    if (layout == GSR_EXTRACT_PLANAR_RAW)
        hipLaunchKernelGGL(k_extract_planar<PRUNE>, dim3(grid), dim3(kExBlock), tables ? ex_lds_bytes(a.C) : 0, s, a);
    else
        hipLaunchKernelGGL(k_extract_rows<PRUNE>, dim3(grid), dim3(kExBlock), 0, s, a);
    return ex_done();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_extract_tiles(int T) { return T <= 0 ? 0 : ex_tiles(T); }

int gsr_extract_prepare(int T, const uint8_t* mask, int32_t* tile_base, void* stream) {
    if (T <= 0 || T > INT32_MAX - kExTile) return api_fail(GSR_ERR_ARG, "gsr_extract_prepare: bad sizes");
    if (!mask || !tile_base) return api_fail(GSR_ERR_ARG, "gsr_extract_prepare: null required pointer");
    return ex_prepare(T, 0, mask, nullptr, 0.0f, tile_base, (hipStream_t)stream);
}

int gsr_extract_prepare_pruned(int T, int layout, const uint8_t* mask, const float* opacities, float threshold,
                               int32_t* tile_base, void* stream) {
    if (T <= 0 || T > INT32_MAX - kExTile || (layout != GSR_EXTRACT_PLANAR_RAW && layout != GSR_EXTRACT_ROWS_ACTIVATED))
        return api_fail(GSR_ERR_ARG, "gsr_extract_prepare_pruned: bad sizes or layout");
    if (!mask || !opacities || !tile_base)
        return api_fail(GSR_ERR_ARG, "gsr_extract_prepare_pruned: null required pointer");
    return ex_prepare(T, layout == GSR_EXTRACT_PLANAR_RAW, mask, opacities, threshold, tile_base, (hipStream_t)stream);
}

int gsr_extract_forward(int B, int T, int N, int C, int layout, unsigned flags, const uint8_t* mask,
                        const int32_t* tile_base, const GsrExtractSet* maps, const GsrExtractSet* tables,
                        const int32_t* texel_face, const float* texel_bary, int32_t* binding_face, float* face_bary,
                        void* stream) {
    const bool want_tables = maps || tables, want_binding = texel_face || texel_bary || binding_face || face_bary;
    if (!want_tables) B = 1;
    if (!ex_sizes_ok(B, T, N, C, layout)) return api_fail(GSR_ERR_ARG, "gsr_extract_forward: bad sizes, C or layout");
    if (N == 0) return 0;  // empty tables: their pointers may be null
    if (!mask || !tile_base || (!want_tables && !want_binding) || (want_tables && !(ex_set_ok(maps) && ex_set_ok(tables))) ||
        (want_binding && !(texel_face && texel_bary && binding_face && face_bary)))
        return api_fail(GSR_ERR_ARG, "gsr_extract_forward: null required pointer");
    ExArgs a{};
    a.B = B, a.T = T, a.N = N, a.C = C, a.ntiles = ex_tiles(T), a.rgb = (flags & GSR_EXTRACT_RGB_SIGMOID) ? 1 : 0;
    a.mask = mask, a.tile_base = tile_base;
    if (want_tables) a.in = *maps, a.tab = *tables;
    a.texel_face = texel_face, a.texel_bary = texel_bary, a.binding_face = binding_face, a.face_bary = face_bary;
    return ex_forward<false>(a, layout, want_tables, (hipStream_t)stream);
}

int gsr_extract_forward_pruned(int T, int N, int C, int layout, unsigned flags, float threshold, const uint8_t* mask,
                               const int32_t* tile_base_mask, const int32_t* tile_base_pruned,
                               const GsrExtractSet* maps, const GsrExtractSet* tables, const int32_t* texel_face,
                               const float* texel_bary, int32_t* binding_face, float* face_bary, void* stream) {
    const bool want_binding = texel_face || texel_bary || binding_face || face_bary;
    if (!ex_sizes_ok(1, T, N, C, layout)) return api_fail(GSR_ERR_ARG, "gsr_extract_forward_pruned: bad sizes, C or layout");
    if (N == 0) return 0;
    if (!mask || !tile_base_mask || !tile_base_pruned || !ex_set_ok(maps) || !ex_set_ok(tables) ||
        (want_binding && !(texel_face && texel_bary && binding_face && face_bary)))
        return api_fail(GSR_ERR_ARG, "gsr_extract_forward_pruned: null required pointer");
    ExArgs a{};
    a.B = 1, a.T = T, a.N = N, a.C = C, a.ntiles = ex_tiles(T), a.rgb = (flags & GSR_EXTRACT_RGB_SIGMOID) ? 1 : 0;
    a.threshold = threshold;
    a.mask = mask, a.tile_base = tile_base_pruned, a.tile_base_mask = tile_base_mask;
    a.in = *maps, a.tab = *tables;
    a.texel_face = texel_face, a.texel_bary = texel_bary, a.binding_face = binding_face, a.face_bary = face_bary;
    return ex_forward<true>(a, layout, true, (hipStream_t)stream);
}

int gsr_extract_backward(int B, int T, int N, int C, int layout, unsigned flags, const uint8_t* mask,
                         const int32_t* tile_base, const GsrExtractSet* maps, const GsrExtractSet* dtables,
                         const GsrExtractSet* dmaps, void* stream) {
    if (!ex_sizes_ok(B, T, N, C, layout)) return api_fail(GSR_ERR_ARG, "gsr_extract_backward: bad sizes, C or layout");
    const bool rgb = (flags & GSR_EXTRACT_RGB_SIGMOID) != 0;
    const bool planar = layout == GSR_EXTRACT_PLANAR_RAW;
    if (!mask || !tile_base || !dtables || !dmaps || !maps || (planar && !ex_set_ok(maps)) || (rgb && !maps->colors))
        return api_fail(GSR_ERR_ARG, "gsr_extract_backward: null required pointer");
    ExArgs a{};
    a.B = B, a.T = T, a.N = N, a.C = C, a.ntiles = ex_tiles(T), a.rgb = rgb ? 1 : 0;
    a.mask = mask, a.tile_base = tile_base;
    a.in = *maps, a.tab = *dtables, a.dmap = *dmaps;
    const unsigned grid = (unsigned)((int64_t)B * a.ntiles);
    if (planar)
        hipLaunchKernelGGL(k_extract_planar_bwd, dim3(grid), dim3(kExBlock), ex_lds_bytes(C), (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_extract_rows_bwd, dim3(grid), dim3(kExBlock), 0, (hipStream_t)stream, a);
    return ex_done();
}

}  // extern "C"
