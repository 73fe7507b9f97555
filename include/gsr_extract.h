/*
 * gsr_extract.h -- C ABI of the UV Gaussian extraction (csrc/extract.hip) for gfx950: from the UV point
 * decoder's output maps to the per-Gaussian tables [B,N,k] that the deform, the trainer and the UV
 * regularisers start from.  It covers, fused, the reference's
 *   head activations   models/modules/net_module/feature_decoder.py:120-135  sigmoid / exp / F.normalize
 *   layout change      the five permute(0,2,3,1).contiguous() copies that follow
 *   boolean gathers    models/UbodyAvatar/ubody_gaussian.py:150-156  x[:, uv_mask_flat, :]
 *   RGB sigmoid        ubody_gaussian.py:186-187  sigmoid of the first three colour channels
 *   pruning            ubody_gaussian.py:229-243  opacity > threshold, B = 1, forward only
 * and the gradient of all but the pruning.
 *
 * Layouts.  T = U*U texels, N table rows per frame, C colour channels (3 <= C <= 64), widths
 * k = (C, 1, 3, 4, 3) for (colors, opacities, scales, rotations, local_pos).
 *   GSR_EXTRACT_PLANAR_RAW      maps float [B,k,T]: the heads' raw outputs, before the activations
 *   GSR_EXTRACT_ROWS_ACTIVATED  maps float [B,T,k]: the decoder's outputs as the reference returns them;
 *                               the operation is then the row gather plus the optional RGB sigmoid
 * Tables are float [B,N,k] in both.
 *
 * Semantics (tests/gaussian_extract_ref.py restates them in numpy).  Every operation is
 * float32, rounded as written, no fma, `/` and sqrtf correctly rounded.  Per kept texel (planar raw):
 *   opacity      y = 1 / (1 + ex_exp(-x))
 *   scale        y = ex_exp(x)
 *   rotation     S = ((x0*x0 + x1*x1) + x2*x2) + x3*x3;  n0 = sqrtf(S);  d = fmaxf(n, 1e-12f);  y_k = x_k / d.
 *                n is n0 refined to the correctly rounded norm when 1e-24f <= S <= 1e30f:
 *                  c = ((e0 + e1) + (e2 + e3)) + ((f1 + f2) + f3), e_k the rounding error of x_k*x_k
 *                  (Dekker's split by 4097: t = 4097*a, hi = t - (t - a), lo = a - hi,
 *                  e = ((hi*hi - p) + (hi + hi)*lo) + lo*lo), f_j that of the j-th add of S (two-sum:
 *                  bb = s - a, f = (a - (s - bb)) + (b - bb));
 *                  (p, pe) = n0*n0 and its error;  n = n0 + (((S - p) - pe) + c) / (n0 + n0).
 *                Otherwise n = n0.  Without the refinement y_k is up to 4 * 2^-24 relative off the exact
 *                quotient (measured 3.05), with it within 2 * 2^-24 (one rounding each for n and the
 *                divide; measured 1.99).  A sum of squares that overflows gives n = d = +inf and
 *                y_k = x_k / inf = +-0 for finite x_k; fmaxf drops a NaN n, d = 1e-12f, where torch's
 *                clamp_min would propagate it.
 *   colour c<3   the opacity's sigmoid when GSR_EXTRACT_RGB_SIGMOID is set (both layouts), else copied
 *   colour c>=3  copied
 *   local pos    copied
 *   ex_exp       extract_dev.h: n = floorf(x*1.44269504f + 0.5f);
 *                r = (x - n*0.693359375f) - n*-2.12194440e-4f;  z = r*r;
 *                p = ((((c5*r + c4)*r + c3)*r + c2)*r + c1)*r + c0  (Cephes' expf coefficients);
 *                y = (p*z + r) + 1;  result (y * 2^(n>>1)) * 2^(n - (n>>1)).
 *                NaN -> NaN;  x > 88.72284f -> +inf;  x < -104 -> +0.  Within 2*2^-23 relative of exp where
 *                the exact result is a normal float (measured 0.68); the sigmoid within 3*2^-23 (1.24).
 * Backward (deterministic: a map element has at most one table row; y, n, d are recomputed from the
 * raw maps, the forward saves nothing):
 *   sigmoid      dx = (g*(1 - y))*y
 *   exp          dx = g*y
 *   copy         dx = g
 *   rotation     n >= 1e-12f:  s = ((g0*y0 + g1*y1) + g2*y2) + g3*y3;  dx_k = (g_k - y_k*s)/d
 *                otherwise:    dx_k = g_k/d
 *   a texel outside the mask gets +0 in every plane.
 *
 * Placement.  A tile is 64 consecutive texels.  tile_base int32 [tiles + 1] is the exclusive scan of
 * the per-tile counts of kept texels, the total in its last word (gsr_extract_prepare*).  The row of
 * a kept texel is tile_base[tile] + the number of kept texels below it in its tile: rows ascend in
 * texel order, the order of the reference's boolean gather.  Forward and backward share it.
 * Pruning keeps a texel when mask && opacity > threshold (strictly, on this operation's own float32
 * opacity).  The tables keep their N rows (the unpruned count); rows [count, N) are written as zeros,
 * count = tile_base_pruned[tiles], a device word.
 *
 * All arrays are contiguous device memory.  Everything is enqueued on `stream`; no entry synchronises
 * the host, reads anything back, uses atomics or a memset; every output element is written exactly
 * once.  A row index outside [0, N) (an N that is not the tile_base's total) is never stored to.
 * Return codes: 0 = success, < 0 = -gsr_status (gsr_last_error()).  GSR_ERR_ARG with nothing launched:
 * a NULL required pointer, B, T or C <= 0, N < 0 or N > T, C outside [3, 64], an unknown layout, or
 * B*T*(C + 11) >= 2^31.  N == 0 launches nothing and succeeds (the backward still writes its zeros).
 */
#ifndef GSR_EXTRACT_H
#define GSR_EXTRACT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_EXTRACT_PLANAR_RAW 0
#define GSR_EXTRACT_ROWS_ACTIVATED 1
#define GSR_EXTRACT_RGB_SIGMOID 1u /* flags bit 0 */

/* five device pointers: maps, tables or their gradients, by the entry's description */
typedef struct GsrExtractSet {
    float* colors;
    float* opacities;
    float* scales;
    float* rotations;
    float* local_pos;
} GsrExtractSet;

/* tiles of T texels ((T + 63) / 64; 0 for T <= 0): tile_base holds one word more */
int gsr_extract_tiles(int T);

/* mask uint8 [T] (0 / non-zero) -> tile_base int32 [tiles + 1].  Once per UV layout. */
int gsr_extract_prepare(int T, const uint8_t* mask, int32_t* tile_base, void* stream);

/* the same with the pruning predicate; opacities float [T] is the opacity map of the one frame (its
 * memory is the same in both layouts); layout says whether the sigmoid applies */
int gsr_extract_prepare_pruned(int T, int layout, const uint8_t* mask, const float* opacities, float threshold,
                               int32_t* tile_base, void* stream);

/* maps -> tables [B,N,k].  texel_face int32 [T] and texel_bary float [T,3] (both or neither) are
 * compacted alike into binding_face int32 [N] and face_bary float [N,3].  maps and tables may both be
 * NULL: only binding_face / face_bary are built (B is then ignored). */
int gsr_extract_forward(int B, int T, int N, int C, int layout, unsigned flags, const uint8_t* mask,
                        const int32_t* tile_base, const GsrExtractSet* maps, const GsrExtractSet* tables,
                        const int32_t* texel_face, const float* texel_bary, int32_t* binding_face, float* face_bary,
                        void* stream);

/* B = 1.  tile_base_mask: gsr_extract_prepare's (total N); tile_base_pruned: gsr_extract_prepare_pruned's
 * with the same mask, maps->opacities, threshold and layout.  Rows [count, N) of every output are zeros. */
int gsr_extract_forward_pruned(int T, int N, int C, int layout, unsigned flags, float threshold, const uint8_t* mask,
                               const int32_t* tile_base_mask, const int32_t* tile_base_pruned,
                               const GsrExtractSet* maps, const GsrExtractSet* tables, const int32_t* texel_face,
                               const float* texel_bary, int32_t* binding_face, float* face_bary, void* stream);

/* dtables [B,N,k] -> dmaps in the maps' layout, overwritten in full.  A NULL member of dmaps is not
 * wanted and not written; a NULL member of dtables is a zero gradient.  maps: the forward's inputs
 * (rows activated: only maps->colors is read, and only with the RGB flag). */
int gsr_extract_backward(int B, int T, int N, int C, int layout, unsigned flags, const uint8_t* mask,
                         const int32_t* tile_base, const GsrExtractSet* maps, const GsrExtractSet* dtables,
                         const GsrExtractSet* dmaps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
