/*
 * gsr_loss.h -- C ABI of the GUAVA training-loss terms beyond gsr_image_loss (include/gsr_ssim.h):
 * the foreground mask, the head / hand crop losses and the UV-Gaussian regularisers of the
 * reference's Optimization_Loss (utils/loss_utils.py:89-159), for gfx950 (csrc/loss.hip).
 *
 * All images are contiguous float32 device arrays; feat [B,32,H,W], target [B,3,H,W], mask [B,1,H,W].
 * With  t = target * mask + (1 - mask) * bg   (mask NULL: t = target)  and  r = W . feat  (W [3,32],
 * NULL: no refined image),  r' = r * mask + (1 - mask) * bg  when mask_refined != 0, else r:
 *
 *   frame terms  l1_weight * mean|feat[:, :3] - t| + refine_weight * mean|r' - t|   (means over B*3*H*W)
 *   crop terms   for each group g < G, frame b and image k < K (k = 0: feat[:, :3], weight l1_weight;
 *                k = 1: r', weight refine_weight; K = 2 with W, else 1): the box boxes[g,b] =
 *                (left, right, top, bottom), clamped to [0,W] / [0,H], cuts the image and t; both
 *                cuts are resampled to S x S by torch's upsample_bilinear2d(align_corners=False):
 *                per axis with extent n,  scale = n / S,  src = max(scale * (d + 0.5) - 0.5, 0),
 *                i0 = floor(src), i1 = i0 + (i0 < n - 1), l1 = src - i0, l0 = 1 - l1.  A box with
 *                right <= left or bottom <= top is skipped.  Group g adds
 *                  weight_k * group_weight[g] * sum|crop(image) - crop(t)| / (n_valid_g * 3 * S^2)
 *                with n_valid_g the number of frames whose box of group g is kept, counted on the
 *                device (0: the group adds nothing).
 *
 * gsr_guava_loss_forward writes the loss partials (sum them: fixed order, deterministic) and keeps
 * the masked images and the per-sample signed weights in `workspace`; gsr_guava_loss_backward then
 * writes dL_dfeat [B,32,H,W] (written once, not accumulated) = d loss / d feat + (channels 0-2)
 * extra_grad.  The crop terms' backward is the resampling rule's exact adjoint, gathered per source
 * pixel (no atomics: two runs give identical bits).  Between the two calls the caller may evaluate
 * further terms on the resampled crops (crops_image / crops_target, e.g. SSIM) and hand their
 * gradient to the backward as crops_grad.  With mask == NULL and G == 0 the partials and dL_dfeat
 * equal gsr_image_loss's bit for bit.
 * Return codes: 0 = success, < 0 = -gsr_status (gsr_last_error()).
 */
#ifndef GSR_LOSS_H
#define GSR_LOSS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of `workspace` (both calls; sized for K = 2) and floats of `loss_partials` */
size_t gsr_guava_loss_workspace_bytes(int B, int H, int W, int G, int S);
int gsr_guava_loss_partials(int B, int H, int W, int G, int S);

/* boxes int32 [G,B,4] and group_weight float [G] on the device (G == 0: both may be NULL).
 * crops_image [K,G,B,3,S,S] and crops_target [G,B,3,S,S]: optional outputs, the resampled cuts of
 * the images and of t (skipped slots zero-filled); n_valid int32 [G]: optional output. */
int gsr_guava_loss_forward(int B, int H, int W, const float* feat, const float* target, const float* refine_w,
                           float l1_weight, float refine_weight, const float* mask, float bg, int mask_refined,
                           int G, int S, const int32_t* boxes, const float* group_weight, float* crops_image,
                           float* crops_target, int32_t* n_valid, float* loss_partials, void* workspace,
                           void* stream);

/* After gsr_guava_loss_forward with the same sizes, refine_w, weights, mask_refined, boxes and
 * workspace.  crops_grad [K,G,B,3,S,S] (optional): a gradient w.r.t. crops_image, added to the L1
 * terms' before the adjoint (slots of skipped boxes are ignored). */
int gsr_guava_loss_backward(int B, int H, int W, const float* refine_w, float l1_weight, float refine_weight,
                            const float* mask, int mask_refined, int G, int S, const int32_t* boxes,
                            const float* crops_grad, const float* extra_grad, float* dL_dfeat,
                            const void* workspace, void* stream);

/* The UV-Gaussian regularisers (utils/loss_utils.py:129-130) of local_pos [N,3] and uv_scales [N,3]
 * (contiguous):
 *   xyz_weight   * mean_n relu(|local_pos_n| - xyz_threshold)
 *   scale_weight * mean_n |relu(uv_scales_n - scale_threshold)|
 * loss_partials [2, gsr_uv_regularizers_partials(N)] (row 0: xyz term, row 1: scale term; sum each
 * row), d_local_pos / d_uv_scales [N,3] written.  The norm's gradient at the zero vector is 0. */
int gsr_uv_regularizers_partials(int N);
int gsr_uv_regularizers(int N, const float* local_pos, const float* uv_scales, float xyz_threshold,
                        float xyz_weight, float scale_threshold, float scale_weight, float* loss_partials,
                        float* d_local_pos, float* d_uv_scales, void* stream);

#ifdef __cplusplus
}
#endif
#endif
