/*
 * gsr_refiner.h -- C ABI of the refiner decoder's glue (csrc/refiner.hip) for gfx950: what surrounds the
 * convolutions of the StyleGAN2 decoder of the reference's StyleUNet
 * (models/modules/net_module/styleunet/styleunet.py), forward (csrc/refiner.hip) and backward
 * (csrc/refiner_bwd.hip, the second half of this file), float32, NCHW contiguous:
 *   weight modulation   ModulatedConv2d.forward :541-561   Linear, multiply, pow, sum, rsqrt, multiply
 *   grouped conv        the same, F.conv2d(groups=B)       becomes a plain batched conv (below)
 *   upsample            F.interpolate(x2, bilinear)        fused into the conv's input pass
 *   StyleConv epilogue  StyleConv.forward :504-516         *sqrt(2), noise, bias, LeakyReLU
 *   SFT                 :305, :402                         out * scale + shift
 *   ToRGB               ToRGB.forward :578-585, :205       modulated 1x1 conv, bias, skip, sigmoid
 * The convolutions themselves are not here: they stay with the caller's dense conv.
 *
 * A modulated conv with demodulation is, exactly,
 *   conv(x, W * s * d) = d[b,o] * conv(s[b,i] * x[b,i], W),
 *   d[b,o] = rsqrt(sum_i s[b,i]^2 * sum_k W[o,i,k]^2 + eps),
 * an input scale, an ordinary conv with the shared weight and an output scale.
 *
 * Semantics (csrc/refiner_dev.h holds the functions, tests/refiner_cases.py restates
 * them in numpy bit for bit).  Every operation is float32, evaluated as written, no fma.
 *   tap          rf_tap(n, f) = 0.75f*n + 0.25f*f
 *   up2          bilinear x2, align_corners=False.  Output index j of an axis reads the input indices
 *                near = j >> 1 and far = near + 1 (j odd) or near - 1 (j even), far clamped to the axis.
 *                Rows first, then columns:  v(c) = rf_tap(x[rn][c], x[rf][c]);  y = rf_tap(v(cn), v(cf)).
 *   coeffs       s[b,j] = dot(latent[b,:], modulation.weight[j,:]) + modulation.bias[j]; the dot is a
 *                float32 sum in the kernel's own order (64 strided partial sums, then a butterfly), within
 *                (S + 2) * 2^-24 * (sum|w*l| + |b|) of the exact value.
 *                d[b,o] = 1.0f / sqrtf(acc + eps), acc the float32 sum over i (the same order) of
 *                (s[b,i]*s[b,i]) * w2[o,i] on the float32 s just stored: within (c_in + 4) * 2^-24 relative.
 *   upmod        y[b,c] = s[b,c] * up2(x[b,c])  (up = 1)  or  s[b,c] * x[b,c]  (up = 0)
 *   epilogue     a = 1.41421356f * d[b,c];  v = ((a*x + nw*noise) + bias[c]);  y = v >= 0 ? v : 0.2f*v;
 *                then y = y*scale + shift when the SFT maps are given; then y = y*post[b,c] when post is.
 *   torgb        wm[o,c] = W[o,c]*s[b,c];  acc = wm[o,0]*x[0];  acc = acc + wm[o,c]*x[c], c ascending;
 *                acc = acc + bias[o];  acc = acc + skip (as given, or up2 of it);  out = acc or
 *                1 / (1 + ex_exp(-acc))  (ex_exp: include/gsr_extract.h).
 *
 * All arrays are contiguous device memory except `layers` (host memory).  Every pointer to pixels must
 * be 16-byte aligned and every image width a multiple of 4 (each lane moves 4 consecutive pixels of a
 * row with one 16-byte access); anything else is GSR_ERR_ARG, not a slower path.  Everything is
 * enqueued on `stream`; no entry synchronises the host, reads anything back or uses atomics; every
 * output element is written exactly once.
 * Return codes: 0 = success, < 0 = -gsr_status (gsr_last_error()).  GSR_ERR_ARG, with nothing launched:
 * a NULL required pointer, a size <= 0, a misaligned pointer or width, C > 512, out_dim > 4, more than
 * 32 layers, or a layer that does not fit the totals given.
 */
#ifndef GSR_REFINER_H
#define GSR_REFINER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One modulated conv of a decoder.  Its modulation rows are [s_off, s_off + c_in) of the stacked
 * modulation weight / bias and of s; with d_off >= 0 it is demodulated: its d are [d_off, d_off + c_out)
 * and its table of sum_k W[o,i,k]^2, float [c_out, c_in], starts at w2[w2_off]. */
typedef struct GsrStyleLayer {
    int32_t s_off, c_in;
    int32_t d_off, c_out;
    int32_t w2_off;
    float eps;
} GsrStyleLayer;

/* Every modulation of a decoder in one launch.  latent float [B,S]; mod_weight float [sum_in,S];
 * mod_bias float [sum_in]; w2 float [w2_floats]; layers: L entries in HOST memory (copied into the
 * launch); s float [B,sum_in]; d float [B,sum_out] (may be NULL when no layer has d_off >= 0). */
int gsr_style_coeffs(int B, int S, int L, const GsrStyleLayer* layers, int sum_in, int sum_out, int64_t w2_floats,
                     const float* latent, const float* mod_weight, const float* mod_bias, const float* w2, float* s,
                     float* d, void* stream);

/* y float [B,C,H,W] = s[b*s_stride + c] * (up ? up2(x) : x).  x float [x_batch,C,H/2,W/2] (up) or
 * [x_batch,C,H,W]; x_batch is 1 (broadcast over B) or B.  up needs even H and W. */
int gsr_style_upmod(int B, int C, int H, int W, int up, int x_batch, const float* x, const float* s, int64_t s_stride,
                    float* y, void* stream);

/* The StyleConv epilogue on x float [B,C,H,W] -> y (y == x allowed).  d (NULL: no demodulation
 * factor) at d[b*d_stride + c]; noise float [noise_batch,1,H,W], noise_batch 0 (none; noise and
 * noise_weight ignored), 1 or B; noise_weight: one device float; bias float [C]; scale, shift float
 * [B,C,H,W] (both or neither); post (NULL: none) at post[b*post_stride + c]. */
int gsr_style_epilogue(int B, int C, int H, int W, const float* x, const float* d, int64_t d_stride, const float* noise,
                       int noise_batch, const float* noise_weight, const float* bias, const float* scale,
                       const float* shift, const float* post, int64_t post_stride, float* y, void* stream);

/* out float [B,O,H,W] from x float [B,C,H,W], weight float [O,C], s at s[b*s_stride + c], bias float [O].
 * skip (NULL: none) float [B,O,H,W], or [B,O,H/2,W/2] with skip_up (even H and W).  O <= 4, C <= 512. */
int gsr_style_torgb(int B, int C, int O, int H, int W, const float* x, const float* weight, const float* s,
                    int64_t s_stride, const float* bias, const float* skip, int skip_up, int sigmoid, float* out,
                    void* stream);

/*
 * ---------------------------------------------------------------------------------------------------
 * Backward (csrc/refiner_bwd.hip).  The convolutions' own backward stays with the caller; these are the
 * pass behind it (upmod), the pass in front of it (epilogue), the ToRGB and the coefficients.  Same
 * contract as the forward: float32 as written, no fma, 16-byte aligned pixel pointers, widths a multiple
 * of 4, GSR_ERR_ARG with nothing launched otherwise, everything on `stream`, no host synchronisation.
 * No atomics: two calls on the same inputs give the same bits.  Noise gets no gradient.
 * A shape whose launch would need 2^32 threads or more (a lane per 4 pixels) is GSR_ERR_ARG as well.
 *
 * Elementwise outputs and sums with a stated order (restated bit for bit by tests/refiner_bwd_cases.py):
 *   epilogue   a, v = ((a*x + nw*noise) + bias), l = lrelu(v) as the forward;  g1 = g_y*post (g_y without
 *              post);  gl = g1*scale (g1 without SFT);  g_v = v >= 0 ? gl : 0.2f*gl (a NaN v: 0.2f);
 *              g_x = a*g_v;  g_scale = g1*l;  g_shift = g1.
 *   up2T       the transpose of up2, a gather: input sample (i, c) collects the output rows 2i-1 .. 2i+2
 *              and columns 2c-1 .. 2c+2, an index outside the plane folded onto the border (there the
 *              border's clamped tap lands).  T(a,b,c,d) = ((0.25f*a + 0.75f*b) + 0.75f*c) + 0.25f*d in
 *              ascending index order; columns first: u(k) = T(g[r_k][2c-1 .. 2c+2]), then up2T = T(u(0..3)).
 *   upmod      g_x = s[b,c] * up2T(g_y)  (up)  or  s[b,c] * g_y;  with x_batch == 1 (up == 0 only):
 *              g_x[c] = s[0,c]*g_y[0,c], then + s[b,c]*g_y[b,c], b ascending.
 *   torgb      g_acc = g_out, or g_out * (y * (1.0f - y)) with the saved output y of a sigmoid forward;
 *              g_x[b,c] = wm[0,c]*g_acc[0], then + wm[o,c]*g_acc[o], o ascending (wm = W*s as the forward);
 *              g_skip = g_acc (same size) or up2T(g_acc) (half size).
 *   coeffs     t[b,o] = (-0.5f * ((d*d)*d)) * g_d;  acc = t[b,0]*w2[0,i], then + t[b,o]*w2[o,i], o
 *              ascending;  g_s[b,i] = g_s[b,i] + (2.0f*s[b,i]) * acc;
 *              g_w2[o,i] = t[0,o]*(s[0,i]*s[0,i]), then + t[b,o]*(s[b,i]*s[b,i]), b ascending.
 *
 * Sums over the pixels of a plane have a fixed tree, not a stated sequence.  A plane of Q = H*W/4
 * lane-quads is cut into gsr_style_backward_chunks(H, W) = ceil(Q / 256) chunks (the shape alone decides);
 * a lane adds its four terms as (t0 + t1) + (t2 + t3), a wave of 64 lanes by a butterfly, a chunk's four
 * waves as ((w0 + w1) + w2) + w3; a plane's chunks are then added 64 strided partial sums in ascending
 * order and a butterfly.  A term passes through at most
 *   D_plane = 11 + ceil(chunks / 64) + 6
 * additions, so a plane sum is within (D_plane + 1) * 2^-24 * sum|term| of the exact sum of its float32
 * terms.  The terms, as float32 products:
 *   epilogue   S_x = sum g_v*x;  S_v = sum g_v;  S_p = sum g_y*y1, y1 = l*scale + shift (rounded as the
 *              forward rounds it; l without SFT).  Then
 *              g_d[b,c] = 1.41421356f * S_x            (D_plane + 2)
 *              g_post[b,c] = S_p                        (D_plane + 1)
 *              g_bias[c] = S_v[0,c] + S_v[b,c], b ascending           (D_plane + B)
 *              g_noise_weight reduces the whole tensor to one number, the sum most exposed to cancellation,
 *              so it alone is formed in float64: the exact products double(g_v)*double(noise), the same
 *              tree in float64, the B*C plane sums as 64 strided sums over planes ascending and a
 *              butterfly, rounded to float32 once: within 2^-24 * |sum| +
 *              (D_plane + ceil(B*C / 64) + 7) * 2^-53 * sum|term|
 *   upmod      g_s[b,c] = sum g_y * up2(x) (up2 as the forward computes it) or sum g_y * x   (D_plane + 1)
 *   torgb      m[b,o,c] = sum g_acc[o]*x[c];  n[b,o] = sum g_acc[o]   (D_plane + 1 each);
 *              g_weight[o,c] = m[0,o,c]*s[0,c] + ..., b ascending      (D_plane + B + 1) * 2^-24 * sum_b |s| sum|term|
 *              g_s[b,c] = m[b,0,c]*W[0,c] + ..., o ascending           (D_plane + O + 1) * 2^-24 * sum_o |W| sum|term|
 *              g_bias[o] = n[0,o] + n[b,o], b ascending                (D_plane + B)
 * in the form (D + k) * 2^-24 * sum|term| throughout.
 *
 * Workspaces (float, device, no need to clear: every slot read is written first):
 *   epilogue   6 * B*C * (chunks + 1), 16-byte aligned (slots of three floats, a pad and a double)
 *   upmod      B*C * chunks
 *   torgb      B * chunks * (O*C + O)
 */

/* ceil(H * W/4 / 256): the chunks of one plane's reductions; 0 for a shape the kernels refuse. */
int64_t gsr_style_backward_chunks(int H, int W);

/* Backward of gsr_style_epilogue: the forward's operands (x is the conv output the forward READ, so the
 * training forward runs out of place) and g_y float [B,C,H,W].  g_x float [B,C,H,W]; g_scale, g_shift
 * float [B,C,H,W] (required with scale); g_d float [B,C] contiguous (required with d); g_post float [B,C]
 * (required with post); g_bias float [C]; g_noise_weight one float (required with noise_batch != 0). */
int gsr_style_epilogue_backward(int B, int C, int H, int W, const float* g_y, const float* x, const float* d,
                                int64_t d_stride, const float* noise, int noise_batch, const float* noise_weight,
                                const float* bias, const float* scale, const float* shift, const float* post,
                                int64_t post_stride, float* g_x, float* g_scale, float* g_shift, float* g_d,
                                float* g_post, float* g_bias, float* g_noise_weight, float* workspace, void* stream);

/* Backward of gsr_style_upmod: g_y float [B,C,H,W] (H, W of the forward's OUTPUT) -> g_x, shaped as x
 * ([x_batch,C,H/2,W/2] with up, else [x_batch,C,H,W]), and g_s float [B,C] contiguous.  x_batch == 1 only
 * with up == 0.  With up, g_x is written one float per lane and needs no alignment. */
int gsr_style_upmod_backward(int B, int C, int H, int W, int up, int x_batch, const float* g_y, const float* x,
                             const float* s, int64_t s_stride, float* g_x, float* g_s, float* workspace, void* stream);

/* Backward of gsr_style_torgb: g_out float [B,O,H,W]; y: the forward's output when it applied the sigmoid,
 * else NULL.  g_x float [B,C,H,W]; g_skip (NULL: the forward had no skip) float [B,O,H,W], or
 * [B,O,H/2,W/2] with skip_up; g_weight float [O,C]; g_s float [B,C] contiguous; g_bias float [O]. */
int gsr_style_torgb_backward(int B, int C, int O, int H, int W, const float* g_out, const float* y, const float* x,
                             const float* weight, const float* s, int64_t s_stride, int skip_up, float* g_x,
                             float* g_skip, float* g_weight, float* g_s, float* g_bias, float* workspace, void* stream);

/* Backward of gsr_style_coeffs' demodulation, one launch for the layer table: s, d as the forward stored
 * them, g_d float [B,sum_out]; g_s float [B,sum_in] holds the gradient that reached s directly and is
 * updated in place for the demodulated layers; g_w2 float [w2_floats]: every table of a demodulated
 * layer is written, floats outside them are left alone.  c_out <= 512 here.  The three dense products
 * that remain (g_latent = g_s * mod_weight, g_mod_weight = g_s^T * latent, g_mod_bias = sum_b g_s) are
 * the caller's GEMMs. */
int gsr_style_coeffs_backward(int B, int L, const GsrStyleLayer* layers, int sum_in, int sum_out, int64_t w2_floats,
                              const float* s, const float* d, const float* w2, const float* g_d, float* g_s, float* g_w2,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
