/* sgr_actor_pose.h -- C ABI of the per-frame actor poses: what the reference's parse_camera
 * (lib/models/street_gaussian_model.py:254-265) computes per actor through ActorPose.get_tracking_translation /
 * get_tracking_rotation (lib/models/actor_pose.py:83-173), for every actor of a frame in one launch that never
 * synchronises with the host (street_gaussians_amd/actor_pose.py builds the records on the host, in numpy).
 *
 * Layouts (DEVICE arrays, float32, contiguous).  A CELL is one (frame f, column c) of the tracklet table, numbered
 * f * O + c, 0 <= cell < n_cells = F * O:
 *   input_trans [n_cells, 3]   input_rots [n_cells, 4] (w, x, y, z)
 *   opt_trans   [n_cells, 3]   opt_rots   [n_cells]     both given (tracking is optimised, `opt_track`) or both NULL
 *   ego [4, 4] row-major (R = ego[:3, :3], t = ego[:3, 3])   poses [K, 7]: out_rot (w, x, y, z), out_trans
 *
 * One thread per actor; per actor, in float32 with contraction off, division and square root correctly rounded.
 * cosf / sinf / atan2f are the device library's (not pinned bit for bit); everything marked [exact] below is pinned
 * bit for bit given its inputs.
 *
 * SAMPLE (sgr_actor_pose_sample: cells a, b, th1, th2 and the float32 weights wa, wb, wd, r) -> (T, Q):
 *   trans_x = input_trans[x] + opt_trans[x] (opt_track) or input_trans[x],  x = a, b
 *   T = (trans_a * wa + trans_b * wb) / wd                       [exact] two products, one sum, one division
 *   without opt_track:  qa = input_rots[a],  qb = input_rots[b]
 *   with opt_track:     qa = mul_theta(input_rots[a], opt_rots[th1]),  qb = mul_theta(qa, opt_rots[th2])
 *   mul_theta(q, t): c = cosf(t), s = sinf(t);                   [exact] given c, s
 *       (qw c - qz s,  qx c + qy s,  qy c - qx s,  qz c + qw s)
 *   Q = slerp(qa, qb, r)
 *
 * SLERP(q0, q1, r) (quaternion_slerp, lib/utils/general_utils.py:277-303, with roma's unitquat_slerp written out):
 *   a = q0 / max(|q0|, 1e-12),  b = q1 / max(|q1|, 1e-12)        |q| = sqrt(((w^2 + x^2) + y^2) + z^2)
 *   p = conj(a) (x) b;  p = -p when p_w < 0                       shortest arc
 *   s = sqrt((p_x^2 + p_y^2) + p_z^2);  h = atan2f(s, p_w);  ang = 2 h
 *   c1 = ang < 1e-3 ? 0.5 - ang^2 / 48 : sinf(h) / ang            sin(ang / 2) / ang and its series
 *   v = (p_xyz / c1) * r                                          r * log map of p
 *   m = |v|;  c2 = m < 1e-3 ? 0.5 - m^2 / 48 : sinf(m / 2) / m
 *   e = (cosf(m / 2), v c2);  Q = a (x) e                         exp map, then the product
 * No 0/0 occurs at ang = 0 or m = 0 in value or gradient: the backward drops the d|x|/dx terms at |x| = 0, whose
 * factors are zero there (the derivatives of c1 and c2 vanish at 0), which is the analytic limit.
 *
 * RECORD (sgr_actor_pose_record): n_samples = 1: (T, Q) = sample 0.  n_samples = 2 (validation frames of a scene with
 * optimised tracking, actor_pose.py:124-136, :160-173): (T1, Q1), (T2, Q2) = samples 0, 1 and
 *   T = (T1 * Wa + T2 * Wb) / Wd                                  [exact]
 *   Q = slerp(Q1, Q2, R)
 *
 * WORLD POSE (street_gaussian_model.py:262-265):
 *   qe = matrix_to_quaternion(R) (general_utils.py:159-218):     [exact]
 *       d = (((1 + m00) + m11) + m22, ((1 + m00) - m11) - m22, ((1 - m00) + m11) - m22, ((1 - m00) - m11) + m22)
 *       q_abs_i = d_i > 0 ? sqrt(d_i) : 0;  i* = the first i with the largest q_abs_i
 *       row i* of [[q0^2, m21-m12, m02-m20, m10-m01], [m21-m12, q1^2, m10+m01, m02+m20],
 *                  [m02-m20, m10+m01, q2^2, m12+m21], [m10-m01, m20+m02, m21+m12, q3^2]]  /  (2 max(q_abs_i*, 0.1))
 *   out_rot = qe (x) Q, the raw product, not normalised           [exact]
 *       (x): ow = ((aw bw - ax bx) - ay by) - az bz;  ox = ((aw bx + ax bw) + ay bz) - az by
 *            oy = ((aw by - ax bz) + ay bw) + az bx;  oz = ((aw bz + ax by) - ay bx) + az bw
 *   out_trans_i = ((R_i0 T_0 + R_i1 T_1) + R_i2 T_2) + t_i        [exact]
 *
 * Behaviours of the reference that this restates and does not repair:
 *   1. idx1 / idx2 are the closest and second closest tracklet entries of the actor, not ordered in time; a timestamp
 *      outside the track extrapolates (r < 0) and nothing clamps it.
 *   2. With opt_track the second angle is read at opt_rots[frame_ind1, column_ind2] (actor_pose.py:148): frame of the
 *      closest entry, column of the second closest.  That cell may belong to another track or to no track at all; it
 *      still receives a gradient.  The host encodes it in `th2`, so the kernel knows no such rule.
 *   3. With opt_track qb is built from the already rotated qa (actor_pose.py:150), so input_rots[b] is never read and the
 *      relative rotation of the slerp is the rotation by opt_rots[th2] alone.
 *   4. mul_theta's factor is (cos t, 0, 0, sin t): a rotation about z by 2 t, the full angle where a unit quaternion takes
 *      the half angle (general_utils.py:240-259).
 *   5. The weights are float64 differences of timestamps rounded to float32 (a float32 tensor times a numpy float64, and
 *      torch.tensor([step]).float()): the host forms wa = t2 - t, wb = t - t1, wd = t2 - t1, r = (t - t1) / (t2 - t1) in
 *      double and rounds once.
 *
 * BACKWARD.  Gradients go to opt_trans at cells a, b and to opt_rots at cells th1, th2 of every sample; ego and the
 * input_* tensors get none.  Cells of different actors (and of one actor) can coincide (rule 2), so the sum has a fixed
 * order: the first launch writes every actor's 16 contributions to `contrib` and zeroes d_opt_trans / d_opt_rots, the
 * second launch is one wave that adds them in (actor, sample, slot) order, each cell owned by one lane.  No float atomics;
 * two runs are bitwise equal; every element of d_opt_trans [n_cells, 3] and d_opt_rots [n_cells] is written.
 *
 * Nothing allocates and nothing synchronises with the host.  A record with a cell outside [0, n_cells) or n_samples
 * outside {1, 2} gives a NaN pose and no gradient (the host never builds one). */
#ifndef SGR_ACTOR_POSE_H
#define SGR_ACTOR_POSE_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgr_actor_pose_sample {
    int32_t a, b;        /* cells of the closest / second closest tracklet entry */
    int32_t th1, th2;    /* cells of the two angles in opt_rots (ignored without opt_track) */
    float wa, wb, wd, r; /* t2 - t, t - t1, t2 - t1, (t - t1) / (t2 - t1) */
} sgr_actor_pose_sample; /* 32 bytes */

typedef struct sgr_actor_pose_record {
    sgr_actor_pose_sample s[2];
    float Wa, Wb, Wd, R; /* the outer weights (n_samples = 2) */
    int32_t n_samples;   /* 1 or 2 */
    int32_t pad[3];
} sgr_actor_pose_record; /* 96 bytes */

/* floats of `contrib` per actor: per sample d trans_a (3), d trans_b (3), d theta1, d theta2 */
#define SGR_ACTOR_POSE_CONTRIB 16
/* floats of `parts` per actor (tests): T of sample 0 (3), qa (4), qb (4), cos / sin of theta1 and theta2 (4), qe (4), Q (4) */
#define SGR_ACTOR_POSE_PARTS 23

/* poses [K, 7] of K records.  `parts` [K, SGR_ACTOR_POSE_PARTS] or NULL.  K = 0 launches nothing.
 * SGR_E_INVALID: negative sizes, missing arrays, only one of opt_trans / opt_rots. */
int sgr_actor_pose_forward(int K, const sgr_actor_pose_record* records, int n_cells, const float* input_trans,
                           const float* input_rots, const float* opt_trans, const float* opt_rots, const float* ego,
                           float* poses, float* parts, void* stream);

/* workgroups (of 256 threads) of the backward's largest first launch: past it the zeroing of d_opt_trans / d_opt_rots and
 * the actors are walked grid-stride */
int sgr_actor_pose_backward_max_blocks(void);

/* d_opt_trans [n_cells, 3] and d_opt_rots [n_cells] from dposes [K, 7]; contrib [K, SGR_ACTOR_POSE_CONTRIB] is scratch.
 * Needs opt_trans and opt_rots.  K = 0 zeroes the gradients. */
int sgr_actor_pose_backward(int K, const sgr_actor_pose_record* records, int n_cells, const float* input_trans,
                            const float* input_rots, const float* opt_trans, const float* opt_rots, const float* ego,
                            const float* dposes, float* contrib, float* d_opt_trans, float* d_opt_rots, void* stream);

#ifdef __cplusplus
}
#endif
#endif
