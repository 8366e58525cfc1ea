/* sgr_scene_frame.h -- per-frame extension of the scene-graph compose of include/sgr_scene.h.
 *
 * The reference renders a different set of models every frame (parse_camera, lib/models/street_gaussian_model.py:
 * 230-250: the background, then the actors whose [start_frame, end_frame] holds the frame; render_object renders the
 * actors only, street_gaussian_renderer.py:42-57) and, with use_pose_correction, passes the background through the
 * camera pose correction of the image (get_xyz / get_rotation, :311-312, 340-341; PoseCorrection.correct_gaussian_xyz /
 * correct_gaussian_rotation, lib/models/camera_pose.py:89-114).  A subset is simply the `segs` array of the frame, in
 * rasterization order, whose pointers address the blocks of persistent (e.g. flat) parameter tensors; the frame
 * descriptor below adds the correction and the gradient blocks of the ABSENT models, which the backward writes as 0 in
 * the same call so that every element of a flat gradient is written exactly once, with no memset of whole tensors.
 *
 * The correction contract, per Gaussian of an SGR_SEG_STATIC segment, in float32 with contraction off; c = correction:
 *   qc = c[0:4] / max(|c[0:4]|, 1e-12)                      F.normalize (camera_pose.py:93)
 *   qq = qc / |qc|,  R = R(qq)                              quaternion_to_matrix (lib/utils/general_utils.py:125-146);
 *        |q| = sqrt(((q_w^2 + q_x^2) + q_y^2) + q_z^2) in both normalisations
 *   x'_a = ((x_0 R_a0 + x_1 R_a1) + x_2 R_a2) + c[4 + a]    [x, 1] @ [R | t; 0 0 0 1]^T (camera_pose.py:98-100)
 *   rot' = qc (x) normalize(rot_raw)                        quaternion_raw_multiply, not renormalised (:109)
 * normalize(rot_raw) is the uncorrected output of sgr_scene_compose_forward; actor segments are never corrected.
 *
 * The backward computes the per-Gaussian gradients through the corrected path and, when correction_grad is given, the
 * 7 gradients of c from 16 sums over the corrected Gaussians (G_ab = sum dx'_a x_b, T_a = sum dx'_a, Q = sum dq' (x)
 * conj(normalize(rot_raw))): per-chunk partials (256 Gaussians, a fixed butterfly order), then groups of 256 chunks
 * summed in a fixed tree order, then the groups summed by one workgroup in a fixed order, then one lane chains through
 * both normalisations.  The order depends only on the number of corrected chunks: the same bits for any stream.
 *
 * All pointers are DEVICE pointers unless noted.  Plain C, no torch types. */
#ifndef SGR_SCENE_FRAME_H
#define SGR_SCENE_FRAME_H
#include <stddef.h>
#include <stdint.h>
#include "sgr_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `count` floats at `ptr` that the backward writes as 0.0f (the gradient block of a model absent from the frame). */
typedef struct sgr_zero_span {
    float* ptr;
    size_t count;
} sgr_zero_span;

typedef struct sgr_scene_frame {
    const float* correction;   /* 7 floats: pose_correction_rots[id] (w, x, y, z; not normalised), pose_correction_trans[id];
                                  NULL = no correction */
    float* correction_grad;    /* backward: 7 floats, written once (0 when no static segment is in the frame); NULL = not wanted */
    int32_t n_zero;            /* backward: entries of `zero` */
    const sgr_zero_span* zero; /* backward: HOST array of spans; the spans must not overlap each other or any gradient
                                  array of `grads` */
} sgr_scene_frame;

/* sgr_scene_compose_forward with a frame descriptor; frame == NULL is sgr_scene_compose_forward.  The forward reads
 * only frame->correction. */
int sgr_scene_compose_forward_ex(int K, const sgr_scene_segment* segs, int M, int S, float* means3D, float* rotations,
                                 float* scales, float* opacities, float* shs, float* semantics,
                                 const sgr_scene_frame* frame, sgr_alloc_fn scratch, void* scratch_user, void* stream);

/* sgr_scene_compose_backward with a frame descriptor; frame == NULL is sgr_scene_compose_backward.  The zero spans are
 * written even when the frame holds no Gaussian. */
int sgr_scene_compose_backward_ex(int K, const sgr_scene_segment* segs, const sgr_scene_segment_grads* grads, int M,
                                  int S, const float* dL_dmeans3D, const float* dL_drotations, const float* dL_dscales,
                                  const float* dL_dopacities, const float* dL_dshs, const float* dL_dsemantics,
                                  const sgr_scene_frame* frame, sgr_alloc_fn scratch, void* scratch_user, void* stream);

#ifdef __cplusplus
}
#endif
#endif
