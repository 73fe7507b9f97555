// deform_internal.h -- library-internal entry points of deform.hip for ehm.hip (not part of the C ABI).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/gsr_deform.h"

namespace gsr {
// One single-frame blend over the tiled bases (k_lbs_blend_tiled1's arguments, deform.hip)
struct Blend1Job {
    int M, NB, NP, pose2rot;
    const float* vt;
    const float* betas;
    const float4* sd_tiled;
    const float* feat;
    const float4* pd_tiled;
    float* v_shaped;
    float* v_posed;
    const float* pose;
};
// whether launch_blend takes k_lbs_blend_tiled1 for these arguments, and that launch's job
bool blend_tiled1_applies(int B, int NB, int NP, const float* vp, const GsrLbsSparse* sp);
Blend1Job blend1_job(int M, int NB, int NP, const float* vt, const float* betas, const float* feat, float* vs,
                     float* vp, const GsrLbsSparse* sp, const float* pose, int pose2rot);
// One model's share of gsr_ehm_forward's batched path (B > 16 frames, tiled bases, CSR regressor)
struct EhmBatchModel {
    int V, J, NB;
    const float* v_template;  // [V,3], or [B,V,3] when vt_stride != 0
    int64_t vt_stride;
    const float* betas;  // [B,NB] row-major (packed rows), or null
    const float* pose;   // [B,J,3] axis-angle
    const int32_t* parents_host;
    const GsrLbsSparse* sp;
    char* ws;  // the model's lbs workspace
};
// whether ehm_batch_run takes this call (else the per-call path: lbs_run, blend_joints_run, ...)
bool ehm_batch_applies(int B, const GsrLbsSparse* sp_h, const GsrLbsSparse* sp_b, int NBh, int NBb);
// gsr_ehm_forward after the pack launch for B > 16: Rodrigues / coefficient tiles of both models,
// paired blend, FLAME chain (+ its joints, + the body template's joints), skin-splice, body pose
// blend, body chain (+ joints), skin.  body_betas_tiles: workspace of gsr_lbs_coef_tile_bytes(B, NBb).
int ehm_batch_run(int B, const EhmBatchModel& head, const EhmBatchModel& body, float* body_betas_tiles,
                  float* head_joints_t, float* body_vt, float* body_tj, const float* joints_offset,
                  const int32_t* head_index, const float* r_eyelid, const float* l_eyelid, const float* eyelid,
                  const float* head_scale, int hj0, int hj1, int bj0, int bj1, uint32_t* bad_index_flag,
                  float* verts, float* joints_transformed, float* joints, float* vert_transforms,
                  float* joint_transforms, void* stream);
// bytes of the tiled copy of B coefficient rows of width K (the matrix-core blend's A operand)
size_t lbs_coef_tile_bytes(int B, int K);
// gsr_blend_joints_sp; blend_done: its blend was launched already (as lbs_run's companion)
int blend_joints_run(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride,
                     const float* betas, const float* shapedirs_t, const float* J_regressor,
                     const float* joints_offset, float* v_shaped, float* joints, const GsrLbsSparse* sp,
                     void* stream, bool blend_done);
// gsr_lbs_sp; with skin = false it stops after the kinematic chain, leaving the joint transforms and
// v_posed in the workspace for lbs_skin_splice
int lbs_run(int B, int V, int J, int NB, const float* v_template, int64_t v_template_stride, const float* betas,
            const float* shapedirs_t, const float* pose, int pose2rot, const float* posedirs,
            const float* J_regressor, const int32_t* parents_host, const float* lbs_weights_t,
            const float* joints_offset, float* verts, float* joints_transformed, float* joints,
            float* vert_transforms, float* joint_transforms, float* v_shaped, char* workspace,
            const GsrLbsSparse* sp, void* stream, bool skin, const Blend1Job* companion = nullptr,
            bool* companion_done = nullptr);
// (companion: a single-frame blend independent of this call's, launched together with this call's
// blend when both take k_lbs_blend_tiled1; *companion_done says whether it was)
// the head's ELL skinning fused into gsr_splice_head's arithmetic (one launch); 1 = not applicable
// (no ELL weights: the caller skins and splices separately), 0 = launched, < 0 = error
int lbs_skin_splice(int B, int Vh, int Jh, const GsrLbsSparse* sp_h, const char* ws_h, int Vb,
                    const int32_t* head_index, const float* r_eyelid, const float* l_eyelid, const float* eyelid,
                    const float* head_scale, const float* head_joints, int hj0, int hj1, const float* body_joints,
                    int Jb, int bj0, int bj1, float* body_v_shaped, uint32_t* bad_index_flag, void* stream);
}  // namespace gsr
