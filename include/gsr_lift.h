/*
 * gsr_lift.h -- C ABI of the image-to-avatar feature lifting (csrc/lift.hip) for gfx950: the two
 * projection gathers of the reference's Ubody_Gaussian_inferer (models/UbodyAvatar/ubody_gaussian.py),
 *   sample_prj_feature          (:75-83)   posed vertices -> bilinear samples of a feature map, border padding
 *   convert_pixel_feature_to_uv (:85-114)  UV texels placed on their faces by barycentrics -> samples with
 *                                          zeros padding, times the UV mask and the face visibility
 * and their gradients with respect to the feature map (a bilinear scatter-add).  The sample positions
 * carry no gradient (every EHM parameter of the reference has requires_grad = False).
 *
 * Semantics (tests/feature_lift_ref.py restates them in numpy).  Every operation is
 * float32, rounded as written, no fma, `/` correctly rounded.  Per frame b, with M = w2c[b]:
 *   camera    gsr_mesh.h's, character for character, so lifted samples and mesh pixels coincide:
 *             r(v) = (M[r][0]*x + M[r][1]*y) + (M[r][2]*z + M[r][3])       -> xv, yv, zv
 *             den = zv + 1e-7f;  xn = xv / (den*tanfovx[b]);  ix = ((xn + 1)*W - 1)*0.5f   (y alike, H)
 *   point     vertex path: p = verts[b,v].  UV path, f = texel_face[t], (i0,i1,i2) = faces[f]:
 *             p_k = (bary0*v0_k + bary1*v1_k) + bary2*v2_k
 *   sampling  torch grid_sample, bilinear, align_corners = False, in this order:
 *             1. ix or iy not finite: the sample is all zeros in both modes (a stated divergence:
 *                torch's behaviour there is undefined)
 *             2. border mode: ix = fminf(fmaxf(ix, 0), W-1); iy alike
 *             3. zeros mode: unless ix > -1 && ix < W && iy > -1 && iy < H the sample is zeros (tested
 *                in float, before any conversion to int)
 *             4. x0 = floorf(ix), wx1 = ix - x0, wx0 = (x0 + 1) - ix; y alike;
 *                w00 = wx0*wy0, w10 = wx1*wy0 (tap x0+1, y0), w01 = wx0*wy1, w11 = wx1*wy1
 *             5. out_c = ((t00 + t10) + t01) + t11,  t = w*feat[b,c,y,x] for a tap inside the image
 *                and +0.0f for a tap outside it; a tap outside the image is never loaded
 *   UV zeros  a texel is written as zeros when texel_face[t] < 0 (how the caller encodes
 *             uvmap_mask == 0), when texel_face[t] >= F, when a vertex index of the face lies outside
 *             [0, V), or when face_visible[b,f] == 0 (checked only when face_visible is given)
 *   backward  dfeat[b,c,y,x] = the sum over samples and in-image taps of w*dout, with the forward's
 *             float32 weights; pixels that no tap reaches get 0.  The sum is accumulated with float
 *             atomic adds, so its last bits depend on the arrival order: two calls need not agree
 *             bitwise (as the rasterizer's backward).  The forward entries are bitwise reproducible.
 *
 * All arrays are contiguous device memory.  Everything is enqueued on `stream`; no entry synchronises
 * the host or reads anything back.  Return codes: 0 = success, < 0 = -gsr_status (gsr_last_error()).
 * GSR_ERR_ARG with nothing launched: a NULL required pointer, a size <= 0, W or H > 16384, or any of
 * B*C*H*W, B*V*C, B*C*T (and B*V, B*F, B*T) >= 2^31.
 */
#ifndef GSR_LIFT_H
#define GSR_LIFT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Border mode.  verts float [B,V,3], w2c float [B,4,4] row-major, tanfovx / tanfovy float [B],
 * feat float [B,C,H,W] -> out float [B,V,C]; ndc float [B,V,2] (or NULL) receives (xn, yn). */
int gsr_lift_vertices(int B, int V, int C, int W, int H, const float* verts, const float* w2c, const float* tanfovx,
                      const float* tanfovy, const float* feat, float* out, float* ndc, void* stream);

/* Zeros mode.  faces int32 [F,3], texel_face int32 [T], texel_bary float [T,3] (shared by the frames),
 * face_visible uint8 [B,F] or NULL (no visibility term) -> out float [B,C,T]; every element is
 * written exactly once.  With T = U*U this is the reference's [B,C,U,U]. */
int gsr_lift_uv(int B, int V, int F, int T, int C, int W, int H, const float* verts, const int32_t* faces,
                const int32_t* texel_face, const float* texel_bary, const float* w2c, const float* tanfovx,
                const float* tanfovy, const float* feat, const uint8_t* face_visible, float* out, void* stream);

/* bytes of `workspace` of the two backward entries (0: bad sizes) */
size_t gsr_lift_backward_workspace_bytes(int B, int C, int W, int H);

/* dout float [B,V,C] -> dfeat float [B,C,H,W], overwritten in full */
int gsr_lift_vertices_backward(int B, int V, int C, int W, int H, const float* verts, const float* w2c,
                               const float* tanfovx, const float* tanfovy, const float* dout, float* dfeat,
                               void* workspace, void* stream);

/* dout float [B,C,T] -> dfeat float [B,C,H,W], overwritten in full */
int gsr_lift_uv_backward(int B, int V, int F, int T, int C, int W, int H, const float* verts, const int32_t* faces,
                         const int32_t* texel_face, const float* texel_bary, const float* w2c, const float* tanfovx,
                         const float* tanfovy, const uint8_t* face_visible, const float* dout, float* dfeat,
                         void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
