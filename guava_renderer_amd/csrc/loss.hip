// loss.hip -- GUAVA's training-loss terms beyond gsr_image_loss (include/gsr_loss.h): the foreground
// mask, the head / hand crop losses and the UV-Gaussian regularisers of the reference's
// Optimization_Loss (utils/loss_utils.py:89-159; cal_box_loss :140-159), for gfx950.
//
// Three streaming passes, one thread per element, 256-thread workgroups, 1 KB of LDS each (the loss
// partial's fixed-shape tree, as k_image_loss in ssim.hip), so occupancy is bounded by registers only:
//   k_guava_frame     per pixel: reads the 32 feature channels ONCE, writes nine image channels to the
//                     workspace (raw RGB, the refined image r' = W.feat with the mask applied, the
//                     masked target t) and the frame terms' loss partial.  This is the only read of
//                     the 32-channel frames in the step.
//   k_guava_crop_fwd  per destination sample (image k, group g, frame b, dy, dx): the bilinear gather
//                     of the image and of t from the nine channels, the crop term's loss partial and
//                     the sample's signed weight  w_k gw[g] sgn(.) / (n_valid 3 S^2); optionally the
//                     resampled crops themselves.  n_valid is counted by every workgroup from the B
//                     boxes of its group (wave-uniform loads, no host read).
//   k_guava_bwd       per pixel: k_image_loss's gradient assembly from the nine channels (the signs
//                     need nothing else), plus the crop terms' adjoint as a GATHER: for every kept box
//                     that holds the pixel, the destination rows and columns that may touch it (a
//                     conservative range), each tested with axis_tap() -- the very function the forward
//                     uses -- so a destination sample's weight lands exactly where the forward read it.
//                     No atomics; dL_dfeat is written once.
// The resampling rule is torch's upsample_bilinear2d with align_corners=False (axis_tap).
#include "../../include/gsr.h"
#include "../../include/gsr_loss.h"
#include "gsr_internal.h"

namespace gsr {

constexpr int kImgCh = 9;  // workspace image channels: 0-2 raw RGB, 3-5 refined r', 6-8 masked target t

__device__ __forceinline__ float sgn1(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

struct Tap {
    int i0, i1;
    float l0, l1;
};

// one axis of upsample_bilinear2d(align_corners=False): destination index d, input extent n >= 1
__device__ __forceinline__ Tap axis_tap(int d, int n, float scale) {
    float src = scale * ((float)d + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Tap t;
    t.i0 = min((int)src, n - 1);  // (src >= 0: truncation is floor; the min never binds for d < S)
    t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

struct Box {
    int l, t, nw, nh;
    bool ok;
};

// box (left, right, top, bottom) of group g, frame b, clamped to the image
__device__ __forceinline__ Box load_box(const int32_t* __restrict__ boxes, int g, int b, int B, int H, int W) {
    const int32_t* q = boxes + ((int64_t)g * B + b) * 4;
    const int l = min(max(q[0], 0), W), r = min(max(q[1], 0), W);
    const int t = min(max(q[2], 0), H), bo = min(max(q[3], 0), H);
    Box x;
    x.l = l; x.t = t; x.nw = r - l; x.nh = bo - t;
    x.ok = x.nw > 0 && x.nh > 0;
    return x;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void k_guava_frame(int HW, const float* __restrict__ feat,
                                                     const float* __restrict__ target,
                                                     const float* __restrict__ rw, float l1w, float rfw,
                                                     float inv_n, const float* __restrict__ mask, float bg,
                                                     int mask_refined, float* __restrict__ img,
                                                     float* __restrict__ partials) {
    __shared__ float red[256];
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    float part = 0.f;
    if (p < HW) {
        const float* f = feat + (int64_t)b * 32 * HW + p;
        const float* t = target + (int64_t)b * 3 * HW + p;
        float* out = img + (int64_t)b * kImgCh * HW + p;
        float fc[32];
#pragma unroll
        for (int c = 0; c < 32; c++) fc[c] = f[(int64_t)c * HW];
        const float m = mask ? mask[(int64_t)b * HW + p] : 1.0f;
        float tt[3];
#pragma unroll
        for (int o = 0; o < 3; o++) {
            tt[o] = t[(int64_t)o * HW];
            if (mask) tt[o] = tt[o] * m + (1.0f - m) * bg;
            part += l1w * fabsf(fc[o] - tt[o]);
            out[(int64_t)o * HW] = fc[o];
            out[(int64_t)(6 + o) * HW] = tt[o];
        }
        if (rw) {
#pragma unroll
            for (int o = 0; o < 3; o++) {
                float r = 0.f;
#pragma unroll
                for (int c = 0; c < 32; c++) r = fmaf(rw[32 * o + c], fc[c], r);
                if (mask && mask_refined) r = r * m + (1.0f - m) * bg;
                part += rfw * fabsf(r - tt[o]);
                out[(int64_t)(3 + o) * HW] = r;
            }
        }
    }
    const float s = block_sum(part, red);
    if (threadIdx.x == 0) partials[(int64_t)b * gridDim.x + blockIdx.x] = s * inv_n;
}

// grid (ceil(S*S / 256), K*G*B); sw [K,G,B,3,S,S]
__global__ __launch_bounds__(256) void k_guava_crop_fwd(int B, int H, int W, int G, int S, float l1w, float rfw,
                                                        const int32_t* __restrict__ boxes,
                                                        const float* __restrict__ gw,
                                                        const float* __restrict__ img, float* __restrict__ sw,
                                                        float* __restrict__ crops_image,
                                                        float* __restrict__ crops_target,
                                                        int32_t* __restrict__ n_valid,
                                                        float* __restrict__ partials) {
    __shared__ float red[256];
    const int kgb = blockIdx.y;
    const int b = kgb % B, g = (kgb / B) % G, k = kgb / (B * G);
    const int SS = S * S, HW = H * W;
    const int s = blockIdx.x * 256 + threadIdx.x;
    const Box bx = load_box(boxes, g, b, B, H, W);
    int nv = 0;
    for (int bb = 0; bb < B; bb++) nv += load_box(boxes, g, bb, B, H, W).ok ? 1 : 0;
    if (n_valid && k == 0 && b == 0 && s == 0) n_valid[g] = nv;
    // (bx.ok implies nv >= 1)
    const float wgt = bx.ok ? (float)((double)(k == 0 ? l1w : rfw) * (double)gw[g] / ((double)nv * 3.0 * (double)SS))
                            : 0.f;
    float part = 0.f;
    if (s < SS) {
        const int64_t o = (int64_t)kgb * 3 * SS + s;
        const int64_t ot = ((int64_t)g * B + b) * 3 * SS + s;
        if (bx.ok) {
            const int dy = s / S, dx = s - dy * S;
            const Tap ty = axis_tap(dy, bx.nh, (float)bx.nh / (float)S);
            const Tap tx = axis_tap(dx, bx.nw, (float)bx.nw / (float)S);
            const int64_t r0 = (int64_t)(bx.t + ty.i0) * W + bx.l, r1 = (int64_t)(bx.t + ty.i1) * W + bx.l;
            const float* im = img + ((int64_t)b * kImgCh + 3 * k) * HW;
            const float* tg = img + ((int64_t)b * kImgCh + 6) * HW;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* pi = im + (int64_t)c * HW;
                const float* pt = tg + (int64_t)c * HW;
                const float v = ty.l0 * (tx.l0 * pi[r0 + tx.i0] + tx.l1 * pi[r0 + tx.i1]) +
                                ty.l1 * (tx.l0 * pi[r1 + tx.i0] + tx.l1 * pi[r1 + tx.i1]);
                const float u = ty.l0 * (tx.l0 * pt[r0 + tx.i0] + tx.l1 * pt[r0 + tx.i1]) +
                                ty.l1 * (tx.l0 * pt[r1 + tx.i0] + tx.l1 * pt[r1 + tx.i1]);
                const float d = v - u;
                part += fabsf(d);
                sw[o + (int64_t)c * SS] = wgt * sgn1(d);
                if (crops_image) crops_image[o + (int64_t)c * SS] = v;
                if (crops_target && k == 0) crops_target[ot + (int64_t)c * SS] = u;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                sw[o + (int64_t)c * SS] = 0.f;
                if (crops_image) crops_image[o + (int64_t)c * SS] = 0.f;
                if (crops_target && k == 0) crops_target[ot + (int64_t)c * SS] = 0.f;
            }
        }
    }
    const float sum = block_sum(part, red);
    if (threadIdx.x == 0) partials[(int64_t)kgb * gridDim.x + blockIdx.x] = sum * wgt;
}

// the destination indices of one axis that may read source index sx: src in [sx - 1, sx + 1), one
// sample of slack on both sides, clamped to [0, S - 1]
__device__ __forceinline__ void dest_range(int sx, float scale, int S, int* lo, int* hi) {
    const float a = ((float)sx - 0.5f) / scale - 0.5f, b = ((float)sx + 1.5f) / scale - 0.5f;
    *lo = min(max((int)floorf(a) - 1, 0), S - 1);
    *hi = min(max((int)ceilf(fminf(b, (float)S)) + 1, 0), S - 1);
}

__device__ __forceinline__ float tap_weight(const Tap& t, int s) {
    return (t.i0 == s ? t.l0 : 0.f) + (t.i1 == s ? t.l1 : 0.f);
}

__global__ __launch_bounds__(256) void k_guava_bwd(int B, int H, int W, const float* __restrict__ rw, float l1w,
                                                   float rfw, float inv_n, const float* __restrict__ mask,
                                                   int mask_refined, int G, int S,
                                                   const int32_t* __restrict__ boxes,
                                                   const float* __restrict__ img, const float* __restrict__ sw,
                                                   const float* __restrict__ cg, const float* __restrict__ extra,
                                                   float* __restrict__ dL) {
    const int HW = H * W;
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float* in = img + (int64_t)b * kImgCh * HW + p;
    float tt[3], graw[3], s[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < 3; o++) {
        tt[o] = in[(int64_t)(6 + o) * HW];
        graw[o] = l1w * inv_n * sgn1(in[(int64_t)o * HW] - tt[o]);
    }
    if (rw) {
#pragma unroll
        for (int o = 0; o < 3; o++) s[o] = rfw * inv_n * sgn1(in[(int64_t)(3 + o) * HW] - tt[o]);
    }
    if (G > 0) {
        const int K = rw ? 2 : 1;
        const int SS = S * S;
        const int y = p / W, x = p - y * W;
        double acc[6] = {0., 0., 0., 0., 0., 0.};
        for (int g = 0; g < G; g++) {
            const Box bx = load_box(boxes, g, b, B, H, W);
            if (!bx.ok || x < bx.l || x >= bx.l + bx.nw || y < bx.t || y >= bx.t + bx.nh) continue;
            const int sx = x - bx.l, sy = y - bx.t;
            const float scx = (float)bx.nw / (float)S, scy = (float)bx.nh / (float)S;
            int xlo, xhi, ylo, yhi;
            dest_range(sx, scx, S, &xlo, &xhi);
            dest_range(sy, scy, S, &ylo, &yhi);
            for (int dy = ylo; dy <= yhi; dy++) {
                const float wy = tap_weight(axis_tap(dy, bx.nh, scy), sy);
                if (wy == 0.f) continue;
                for (int dx = xlo; dx <= xhi; dx++) {
                    const float wx = tap_weight(axis_tap(dx, bx.nw, scx), sx);
                    if (wx == 0.f) continue;
                    const double w = (double)wy * (double)wx;
                    for (int k = 0; k < K; k++) {
                        const int64_t o = (((int64_t)k * G + g) * B + b) * 3 * SS + (int64_t)dy * S + dx;
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            float v = sw[o + (int64_t)c * SS];
                            if (cg) v += cg[o + (int64_t)c * SS];
                            acc[3 * k + c] += w * (double)v;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 3; o++) {
            graw[o] += (float)acc[o];
            s[o] += (float)acc[3 + o];
        }
    }
    if (rw && mask && mask_refined) {
        const float m = mask[(int64_t)b * HW + p];
#pragma unroll
        for (int o = 0; o < 3; o++) s[o] *= m;
    }
    float* g = dL + (int64_t)b * 32 * HW + p;
#pragma unroll
    for (int c = 0; c < 32; c++) {
        float v = rw ? fmaf(rw[c], s[0], fmaf(rw[32 + c], s[1], rw[64 + c] * s[2])) : 0.f;
        if (c < 3) {
            v += graw[c];
            if (extra) v += extra[(int64_t)b * 3 * HW + (int64_t)c * HW + p];
        }
        g[(int64_t)c * HW] = v;
    }
}

__global__ __launch_bounds__(256) void k_uv_regularizers(int N, const float* __restrict__ lp,
                                                         const float* __restrict__ sc, float th_xyz, float w_xyz,
                                                         float th_sc, float w_sc, float inv_n,
                                                         float* __restrict__ partials, float* __restrict__ d_lp,
                                                         float* __restrict__ d_sc) {
    __shared__ float red[256];
    const int n = blockIdx.x * 256 + threadIdx.x;
    float p0 = 0.f, p1 = 0.f;
    if (n < N) {
        const float x = lp[3 * (int64_t)n], y = lp[3 * (int64_t)n + 1], z = lp[3 * (int64_t)n + 2];
        const float r = sqrtf(x * x + y * y + z * z);
        float k = 0.f;  // (r > threshold >= 0 implies r > 0; a zero row has gradient 0)
        if (r - th_xyz > 0.f && r > 0.f) {
            p0 = r - th_xyz;
            k = w_xyz * inv_n / r;
        }
        d_lp[3 * (int64_t)n] = k * x;
        d_lp[3 * (int64_t)n + 1] = k * y;
        d_lp[3 * (int64_t)n + 2] = k * z;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = fmaxf(sc[3 * (int64_t)n + c] - th_sc, 0.f);
        const float q = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        p1 = q;
        const float kq = q > 0.f ? w_sc * inv_n / q : 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) d_sc[3 * (int64_t)n + c] = kq * v[c];
    }
    const float s0 = block_sum(p0, red);
    __syncthreads();  // red is reused
    const float s1 = block_sum(p1, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s0 * (w_xyz * inv_n);
        partials[gridDim.x + blockIdx.x] = s1 * (w_sc * inv_n);
    }
}

static bool sizes_ok(int B, int H, int W, int G, int S) {
    if (B <= 0 || H <= 0 || W <= 0 || G < 0 || B > 65535) return false;
    if ((int64_t)H * W > (int64_t)1 << 28) return false;
    if (G > 0 && (S <= 0 || S > 2048 || (int64_t)2 * G * B > 65535)) return false;
    return true;
}

static int64_t image_floats(int B, int H, int W) { return (int64_t)B * kImgCh * H * W; }

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_guava_loss_workspace_bytes(int B, int H, int W, int G, int S) {
    if (!sizes_ok(B, H, W, G, S)) return 0;
    return sizeof(float) * (size_t)(image_floats(B, H, W) + (G > 0 ? (int64_t)2 * G * B * 3 * S * S : 0));
}

int gsr_guava_loss_partials(int B, int H, int W, int G, int S) {
    if (!sizes_ok(B, H, W, G, S)) return 0;
    return B * ((H * W + 255) / 256) + (G > 0 ? 2 * G * B * ((S * S + 255) / 256) : 0);
}

int gsr_guava_loss_forward(int B, int H, int W, const float* feat, const float* target, const float* refine_w,
                           float l1_weight, float refine_weight, const float* mask, float bg, int mask_refined,
                           int G, int S, const int32_t* boxes, const float* group_weight, float* crops_image,
                           float* crops_target, int32_t* n_valid, float* loss_partials, void* workspace,
                           void* stream) {
    if (!sizes_ok(B, H, W, G, S)) return api_fail(GSR_ERR_ARG, "gsr_guava_loss_forward: bad sizes");
    if (!feat || !target || !loss_partials || !workspace)
        return api_fail(GSR_ERR_ARG, "gsr_guava_loss_forward: null required pointer");
    if (G > 0 && (!boxes || !group_weight))
        return api_fail(GSR_ERR_ARG, "gsr_guava_loss_forward: G > 0 needs boxes and group_weight");
    const int HW = H * W;
    const double n = 3.0 * (double)B * (double)HW;
    float* img = (float*)workspace;
    hipLaunchKernelGGL(k_guava_frame, dim3((HW + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, HW, feat,
                       target, refine_w, l1_weight, refine_weight, (float)(1.0 / n), mask, bg, mask_refined, img,
                       loss_partials);
    if (G > 0) {
        const int K = refine_w ? 2 : 1;
        float* sw = img + image_floats(B, H, W);
        float* cpart = loss_partials + (int64_t)B * ((HW + 255) / 256);
        const int nbx = (S * S + 255) / 256;
        if (K == 1)  // the partial slots of the absent refined image
            if (hipMemsetAsync(cpart + (int64_t)G * B * nbx, 0, sizeof(float) * (size_t)G * B * nbx,
                               (hipStream_t)stream) != hipSuccess)
                return api_fail(GSR_ERR_HIP, "gsr_guava_loss_forward: memset failed");
        hipLaunchKernelGGL(k_guava_crop_fwd, dim3(nbx, K * G * B), dim3(256), 0, (hipStream_t)stream, B, H, W, G, S,
                           l1_weight, refine_weight, boxes, group_weight, img, sw, crops_image, crops_target,
                           n_valid, cpart);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

int gsr_guava_loss_backward(int B, int H, int W, const float* refine_w, float l1_weight, float refine_weight,
                            const float* mask, int mask_refined, int G, int S, const int32_t* boxes,
                            const float* crops_grad, const float* extra_grad, float* dL_dfeat,
                            const void* workspace, void* stream) {
    if (!sizes_ok(B, H, W, G, S)) return api_fail(GSR_ERR_ARG, "gsr_guava_loss_backward: bad sizes");
    if (!dL_dfeat || !workspace) return api_fail(GSR_ERR_ARG, "gsr_guava_loss_backward: null required pointer");
    if (G > 0 && !boxes) return api_fail(GSR_ERR_ARG, "gsr_guava_loss_backward: G > 0 needs boxes");
    const int HW = H * W;
    const double n = 3.0 * (double)B * (double)HW;
    const float* img = (const float*)workspace;
    hipLaunchKernelGGL(k_guava_bwd, dim3((HW + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, B, H, W, refine_w,
                       l1_weight, refine_weight, (float)(1.0 / n), mask, mask_refined, G, S, boxes, img,
                       img + image_floats(B, H, W), G > 0 ? crops_grad : nullptr, extra_grad, dL_dfeat);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

int gsr_uv_regularizers_partials(int N) { return N > 0 ? (N + 255) / 256 : 0; }

int gsr_uv_regularizers(int N, const float* local_pos, const float* uv_scales, float xyz_threshold,
                        float xyz_weight, float scale_threshold, float scale_weight, float* loss_partials,
                        float* d_local_pos, float* d_uv_scales, void* stream) {
    if (N <= 0) return api_fail(GSR_ERR_ARG, "gsr_uv_regularizers: N must be positive");
    if (!local_pos || !uv_scales || !loss_partials || !d_local_pos || !d_uv_scales)
        return api_fail(GSR_ERR_ARG, "gsr_uv_regularizers: null pointer");
    hipLaunchKernelGGL(k_uv_regularizers, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, local_pos,
                       uv_scales, xyz_threshold, xyz_weight, scale_threshold, scale_weight, (float)(1.0 / (double)N),
                       loss_partials, d_local_pos, d_uv_scales);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : api_fail(GSR_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
