/*
 * gsr_refiner.h -- C ABI of the refiner decoder's glue (csrc/refiner.hip) for gfx950: what surrounds the
 * convolutions of the StyleGAN2 decoder of the reference's StyleUNet
 * (models/modules/net_module/styleunet/styleunet.py), forward only, float32, NCHW contiguous:
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

#ifdef __cplusplus
}
#endif
#endif
