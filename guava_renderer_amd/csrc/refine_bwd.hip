// refine_bwd.hip -- backward of the fused refiner head (include/gsr.h gsr_refine_backward_*).
//
// The refine forward composites gsr_refine_prepare'd rows f' = M f with the unchanged blend kernel
// (M: identity on channels [0, keep), the conv weight W on [keep, keep + n_out), zero below) and
// finishes with bias + leaky ReLU, so its backward is the existing render / projection backward run on
// the prepared rows, between two small kernels:
//  * k_refine_bwd_image (the image end): the gradient image in prepared channel space
//      G'[c] = dL/draw[c] (c < keep),  G'[keep + o] = dz[o] = dL/dout[o] (out[o] > 0 ? 1 : slope),
//      0 for every remaining channel (k_render_bwd reads all 32),
//    plus the per-frame reductions dbias_b[o] = sum_px dz[o] and S[b][o] = sum_px final_T dz[o] (the
//    gradient of the prepared background, which dW needs).  A streaming kernel: channel-major 4-byte
//    accesses, 256 contiguous bytes per wave instruction.
//  * k_refine_bwd_rows (the row end), from d' = dL/df' [n][32] of the middle:
//      dL/df[c]  = (c < keep ? d'[c] : 0) + sum_o W[o][c] d'[keep + o]
//      dW[o][c]  = sum_rows d'[row][keep + o] f[row][c]
//    both on v_mfma_f32_32x32x2_f32 (exact f32 products, k-ordered f32 accumulation; operand and C/D
//    layout as render_fwd.hip's store_strip documents: A[i = l & 31][k = l >> 5], B[k][j = l & 31],
//    acc[r] = D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31]).
// Every sum is deterministic: wave reductions, an LDS row per workgroup, one partial per workgroup in
// caller-provided scratch, summed in a fixed order by the finishing kernels.  No float atomics.  The
// splits depend on the problem size only (never on the device's CU count), so the sums reproduce
// across machines.
#include "gsr_internal.h"

namespace gsr {

typedef float floatx16 __attribute__((ext_vector_type(16)));

#ifndef GSR_REFINE_DF_VALU
#define GSR_REFINE_DF_VALU 0  // 1: dL/df on the VALU instead of a second MFMA (A/B builds, tools/build_ab.py)
#endif

struct RefineImageArgs {
    int HW, n_out, keep;
    float slope;
    const uint32_t* ctrl;        // the workspace's control words (overflow, forward-only)
    const float* final_T;        // [B][HW]
    const float* out_refine;     // [B][n_out][HW]
    const float* dout;           // [B][n_out][HW]
    const float* dkeep;          // [B][keep][HW] or null
    float* G;                    // [B][32][HW]
    float* partials;             // [B][gridDim.x][64]: dbias partial (32), S partial (32)
    float* frame_sums;           // [B][64]
};

// One pixel per lane, kRefinePixPerWg pixels per workgroup (4 per thread, 256 apart).
__global__ __launch_bounds__(256) void k_refine_bwd_image(RefineImageArgs p) {
    __shared__ float red[4][64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t HW = p.HW;
    // an overflowed (or forward-only) forward has zero gradients, as in k_render_bwd: out_refine is
    // NaN then and must reach neither G' nor the sums
    const bool dead = p.ctrl[kCtrlOverflow] != 0u || p.ctrl[kCtrlFwdOnly] != 0u;
    int64_t pix[4];
    bool ok[4];
    float T[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        pix[k] = (int64_t)blockIdx.x * kRefinePixPerWg + k * 256 + tid;
        ok[k] = pix[k] < HW;
        T[k] = (ok[k] && !dead) ? p.final_T[b * HW + pix[k]] : 0.0f;
    }
    float* G = p.G + (int64_t)b * GSR_C * HW;
    for (int c = 0; c < p.keep; c++) {
        const float* src = p.dkeep ? p.dkeep + ((int64_t)b * p.keep + c) * HW : nullptr;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (ok[k]) G[c * HW + pix[k]] = (src && !dead) ? src[pix[k]] : 0.0f;
    }
    for (int o = 0; o < p.n_out; o++) {
        const float* so = p.out_refine + ((int64_t)b * p.n_out + o) * HW;
        const float* sd = p.dout + ((int64_t)b * p.n_out + o) * HW;
        float a = 0.0f, s = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!ok[k]) continue;
            float dz = 0.0f;
            // the sign of the forward's own output; 0 (and -0) takes the slope, as F.leaky_relu_'s
            // in-place backward does
            if (!dead) dz = sd[pix[k]] * (so[pix[k]] > 0.0f ? 1.0f : p.slope);
            G[(p.keep + o) * HW + pix[k]] = dz;
            a += dz;
            s += T[k] * dz;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            a += __shfl_xor(a, m);
            s += __shfl_xor(s, m);
        }
        if (lane == 0) {
            red[wave][o] = a;
            red[wave][32 + o] = s;
        }
    }
    for (int c = p.keep + p.n_out; c < GSR_C; c++) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (ok[k]) G[c * HW + pix[k]] = 0.0f;
    }
    __syncthreads();
    if (tid < 64) {
        const float v = (tid & 31) < p.n_out ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0f;
        p.partials[((int64_t)b * gridDim.x + blockIdx.x) * 64 + tid] = v;
    }
}

// frame_sums[b][t] = sum of the frame's partial rows, in a fixed order: 16 interleaved chains, then
// the chains in order.
__global__ __launch_bounds__(1024) void k_refine_bwd_image_finish(int nwg, const float* __restrict__ partials,
                                                                  float* __restrict__ frame_sums) {
    __shared__ float red[16][64];
    const int b = blockIdx.x, t = threadIdx.x & 63, j = threadIdx.x >> 6;
    const float* src = partials + (int64_t)b * nwg * 64;
    float v = 0.0f;
    for (int w = j; w < nwg; w += 16) v += src[(int64_t)w * 64 + t];
    red[j][t] = v;
    __syncthreads();
    if (threadIdx.x < 64) {
        float s = red[0][t];
        for (int k = 1; k < 16; k++) s += red[k][t];
        frame_sums[b * 64 + t] = s;
    }
}

struct RefineRowsArgs {
    int rpf;                     // rows per frame of rows (n / row_frames)
    int rpw;                     // rows per workgroup
    int n_out, keep;
    const float* dprep;          // [row_frames][rpf][32]
    const float* raw;            // raw feature rows, frame f at raw + f * raw_stride
    int64_t raw_stride;
    const float* W;              // [n_out][32]
    float* drows;                // [row_frames][rpf][32]
    float* tiles;                // [row_frames][gridDim.x][32][32] partial dW tiles
};

// Workgroup (x, y) owns rows [x rpw, (x + 1) rpw) of frame y: its four waves take 32-row blocks in
// turn.  Per block: 16 k-steps of the dW tile (a pair of rows per step, lane (h, c) supplying
// A = d'[row_h][keep + c] and B = f[row_h][c]: 256 contiguous bytes per wave load), then dL/df of
// the block as a second MFMA with k = o (A = d'[row c][keep + o_h], B = W[o_h][c] held in registers),
// the kept channels entering as the accumulator's initial value.  Rows past the range feed zeros.
__global__ __launch_bounds__(256) void k_refine_bwd_rows(RefineRowsArgs p) {
    __shared__ float tile[4][GSR_C * GSR_C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
    const int fb = blockIdx.y;
    const int r0 = blockIdx.x * p.rpw;
    const int r1 = min(p.rpf, r0 + p.rpw);
    const float* dp = p.dprep + (int64_t)fb * p.rpf * GSR_C;
    const float* fr = p.raw + fb * p.raw_stride;
    float* out = p.drows + (int64_t)fb * p.rpf * GSR_C;
#if GSR_REFINE_DF_VALU
    float wcol[GSR_C];  // W[o][c] of this lane's channel
#pragma unroll
    for (int o = 0; o < GSR_C; o++) wcol[o] = o < p.n_out ? p.W[o * GSR_C + c] : 0.0f;
#else
    float wreg[16];  // the B operand of k-step s: W[2 s + h][c]
#pragma unroll
    for (int s = 0; s < 16; s++) {
        const int oo = 2 * s + h;
        wreg[s] = oo < p.n_out ? p.W[oo * GSR_C + c] : 0.0f;
    }
#endif
    const bool acol = c < p.n_out;
    const bool kcol = c < p.keep;
    floatx16 acc = {0};
    for (int g0 = r0 + wave * 32; g0 < r1; g0 += 128) {
#pragma unroll
        for (int j = 0; j < 16; j++) {  // (fully unrolled: the block's 32 loads in flight together)
            const int row = g0 + 2 * j + h;
            const bool in = row < r1;
            const float a = (in && acol) ? dp[row * GSR_C + p.keep + c] : 0.0f;
            const float f = in ? fr[row * GSR_C + c] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, f, acc, 0, 0, 0);
        }
#if GSR_REFINE_DF_VALU
        // A/B variant: dL/df on the VALU, the block's d' rows staged in the wave's LDS
        // slab and read back as half-wave broadcasts
        float* st = tile[wave];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int row = g0 + 2 * j + h;
            st[(2 * j + h) * GSR_C + c] = row < r1 ? dp[row * GSR_C + c] : 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll 2
        for (int j = 0; j < 16; j++) {
            const int row = g0 + 2 * j + h;
            const float* sr = st + (2 * j + h) * GSR_C;
            float v = kcol ? sr[c] : 0.0f;
#pragma unroll
            for (int o = 0; o < GSR_C; o++)
                if (o < p.n_out) v = fmaf(wcol[o], sr[p.keep + o], v);
            if (row < r1) out[row * GSR_C + c] = v;
        }
        __builtin_amdgcn_wave_barrier();
        continue;
#else
        floatx16 o;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = g0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            o[r] = (kcol && row < r1) ? dp[row * GSR_C + c] : 0.0f;
        }
        const int rowA = g0 + c;
        const bool inA = rowA < r1;
#pragma unroll
        for (int s = 0; s < 16; s++) {
            if (2 * s < p.n_out) {  // wave-uniform
                const int oo = 2 * s + h;
                const float a2 = (inA && oo < p.n_out) ? dp[rowA * GSR_C + p.keep + oo] : 0.0f;
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, wreg[s], o, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = g0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row < r1) out[row * GSR_C + c] = o[r];
        }
#endif
    }
#pragma unroll
    for (int r = 0; r < 16; r++) tile[wave][((r & 3) + 8 * (r >> 2) + 4 * h) * GSR_C + c] = acc[r];
    __syncthreads();
    float* dst = p.tiles + ((int64_t)fb * gridDim.x + blockIdx.x) * (GSR_C * GSR_C);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = tid + 256 * k;
        dst[i] = ((tile[0][i] + tile[1][i]) + tile[2][i]) + tile[3][i];
    }
}

// Block o: dW[o][c] = the partial tiles summed in workgroup order (32 interleaved chains, then the
// chains in order) + sum_b S[b][o] bg[b][c]; dbias[o] = sum_b of the frames' sums.
__global__ __launch_bounds__(1024) void k_refine_bwd_finish(int ntile, const float* __restrict__ tiles, int B,
                                                           const float* __restrict__ frame_sums,
                                                           const float* __restrict__ bg, int64_t bg_stride,
                                                           float* __restrict__ dW, float* __restrict__ dbias) {
    __shared__ float red[32][GSR_C];
    const int o = blockIdx.x, c = threadIdx.x & 31, j = threadIdx.x >> 5;
    float v = 0.0f;
#pragma unroll 4
    for (int t = j; t < ntile; t += 32) v += tiles[(int64_t)t * (GSR_C * GSR_C) + o * GSR_C + c];
    red[j][c] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        float s = red[0][c];
        for (int k = 1; k < 32; k++) s += red[k][c];
        for (int b = 0; b < B; b++) s += frame_sums[b * 64 + 32 + o] * bg[b * bg_stride + c];
        dW[o * GSR_C + c] = s;
    } else if (threadIdx.x == 32 && dbias) {
        float s = 0.0f;
        for (int b = 0; b < B; b++) s += frame_sums[b * 64 + o];
        dbias[o] = s;
    }
}

int refine_image_workgroups(int W, int H) {
    return (int)(((int64_t)W * H + kRefinePixPerWg - 1) / kRefinePixPerWg);
}

// rows per workgroup: 256, doubled until a frame of rows needs at most 512 workgroups -- a function
// of the row count alone
int refine_rows_per_workgroup(int rows_per_frame) {
    int rpw = 256;
    while ((rows_per_frame + rpw - 1) / rpw > 512) rpw <<= 1;
    return rpw;
}

void launch_refine_bwd_image(int B, int W, int H, const uint32_t* ctrl, const float* final_T, const float* out_refine,
                             const float* dout, const float* dkeep, int n_out, int keep, float slope, float* G,
                             float* partials, float* frame_sums, hipStream_t s) {
    const int nwg = refine_image_workgroups(W, H);
    RefineImageArgs a{W * H, n_out, keep, slope, ctrl, final_T, out_refine, dout, dkeep, G, partials, frame_sums};
    hipLaunchKernelGGL(k_refine_bwd_image, dim3(nwg, B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_refine_bwd_image_finish, dim3(B), dim3(1024), 0, s, nwg, partials, frame_sums);
}

void launch_refine_bwd_rows(int n, int row_frames, const float* dprep, const float* raw, int64_t raw_stride,
                            const float* W, int n_out, int keep, int B, const float* frame_sums, const float* bg,
                            int64_t bg_stride, float* tiles, float* drows, float* dW, float* dbias, hipStream_t s) {
    const int rpf = n / row_frames;
    const int rpw = refine_rows_per_workgroup(rpf);
    const int nwg = (rpf + rpw - 1) / rpw;
    if (n > 0) {
        RefineRowsArgs a{rpf, rpw, n_out, keep, dprep, raw, raw_stride, W, drows, tiles};
        hipLaunchKernelGGL(k_refine_bwd_rows, dim3(nwg, row_frames), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_refine_bwd_finish, dim3(n_out), dim3(1024), 0, s, n > 0 ? nwg * row_frames : 0, tiles, B,
                       frame_sums, bg, bg_stride, dW, dbias);
}

}  // namespace gsr
