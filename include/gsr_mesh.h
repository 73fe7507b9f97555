/*
 * gsr_mesh.h -- C ABI of the mesh visibility rasterizer (csrc/mesh_raster.hip) for gfx950: the
 * pix_to_face / zbuf / bary_coords of PyTorch3D's rasterize_meshes at blur_radius = 0,
 * faces_per_pixel = 1, perspective_correct = True (no backface culling, no z clipping), which the
 * reference's BaseMeshRenderer.render_fragments (utils/graphics_utils.py:471-492) feeds to the UV
 * visibility mask of Ubody_Gaussian_inferer (models/UbodyAvatar/ubody_gaussian.py:85-114,140-143).
 *
 * Semantics (tests/mesh_raster_ref.py restates them in numpy).  Every operation is
 * float32, rounded as written, no fma, `/` correctly rounded.  Per frame b, with M = w2c[b]:
 *   view      r(v) = (M[r][0]*x + M[r][1]*y) + (M[r][2]*z + M[r][3])       -> xv, yv, zv
 *   pixel     den = zv + 1e-7f;  xn = xv / (den*tanfovx[b]);  px = ((xn + 1)*W - 1)*0.5   (y alike, H)
 *             pixel (xi, yi) has its centre at (px, py) = (xi, yi)
 *   culls     a face is skipped when a vertex index is outside [0, V), when max(z0,z1,z2) < 0, when
 *             one of its nine projected coordinates is not finite, or when
 *             |area| <= 1e-8f * (W*H*0.25f),  area = (x2-x0)*(y1-y0) - (y2-y0)*(x1-x0)
 *   box       xi in [ceil(xmin), floor(xmax)] clipped to [0, W-1]; yi alike
 *   inside    E(p;a,b) = (p.x-a.x)*(b.y-a.y) - (p.y-a.y)*(b.x-a.x);  w0 = E(p;v1,v2)/area,
 *             w1 = E(p;v2,v0)/area,  w2 = E(p;v0,v1)/area;  inside <=> all three > 0
 *   depth     t0 = (w0*z1)*z2, t1 = (z0*w1)*z2, t2 = (z0*z1)*w2;  d = max((t0+t1)+t2, 1e-8f);
 *             b_i = t_i/d;  pz = (b0*z0 + b1*z1) + b2*z2;  the pair is kept iff pz >= 0
 *   winner    the smallest pz per pixel; among equal pz bits the lowest face index.  The result does
 *             not depend on scheduling: two calls give identical bits.
 *
 * Outputs (each may be NULL = not wanted), contiguous:
 *   pix_to_face  int32 [B,H,W]    face index, or b*F + face with packed != 0; -1 where empty
 *   zbuf         float [B,H,W]    pz of the winner; -1 where empty
 *   bary         float [B,H,W,3]  the winner's b_i; -1 where empty
 *   face_visible uint8 [B,F]      1 iff the face wins at least one pixel of frame b
 * No host synchronisation; everything is enqueued on `stream`.
 * Return codes: 0 = success, < 0 = -gsr_status (gsr_last_error()).
 */
#ifndef GSR_MESH_H
#define GSR_MESH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of `workspace` for up to B frames (0: bad sizes).  A workspace sized for B serves every
 * call with fewer frames and the same V, F, W, H. */
size_t gsr_mesh_raster_workspace_bytes(int B, int V, int F, int W, int H);

/* verts float [B,V,3], faces int32 [F,3] (shared by the frames), w2c float [B,4,4] row-major,
 * tanfovx / tanfovy float [B]: all on the device.  Fails with GSR_ERR_ARG (nothing launched) on a
 * NULL required pointer, a size <= 0, W or H > 16384, B*V, B*F or B*H*W >= 2^31. */
int gsr_mesh_raster(int B, int V, int F, int W, int H, const float* verts, const int32_t* faces, const float* w2c,
                    const float* tanfovx, const float* tanfovy, int packed, int32_t* pix_to_face, float* zbuf,
                    float* bary, uint8_t* face_visible, void* workspace, void* stream);

/* texel_visible uint8 [B,N] = face_visible[b, binding_face[n]]  (binding_face int32 [N] on the
 * device; an index outside [0, F) gives 0): the reference's visble_all_faces[:, uvmap_f_idx]. */
int gsr_mesh_visible_texels(int B, int F, int N, const uint8_t* face_visible, const int32_t* binding_face,
                            uint8_t* texel_visible, void* stream);

/* Counters of the last gsr_mesh_raster on `workspace`, read back with a blocking copy (call it after
 * the stream is synchronised): out[0] faces rasterized by their own lane, out[1] faces handed to the
 * wave-per-face kernel, out[2] faces culled (out[0] + out[1] + out[2] = B*F), out[3] covered pixels. */
int gsr_mesh_raster_stats(const void* workspace, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
