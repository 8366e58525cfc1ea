// sgr_quat.h -- the quaternion and rigid-motion arithmetic of the scene-side kernels (compose: sgr_scene.hip, actor poses:
// sgr_actor_pose.hip, density control: sgr_densify.hip and sgr_densify_rules.h), one text per formula of the reference
// (general_utils.py:125-146 and :220-238, F.normalize).  __host__ __device__ inline functions like sgr_math.h, so
// tests/host_math runs the same text on the CPU (tests/test_quat_cpu.py).
//
// Contraction belongs to the CALL SITE's contract and `#pragma clang fp contract` is lexical: a helper keeps the state of
// the place where it is defined, not of its caller.  Every function in which a multiply feeds an add therefore comes in
// two flavours expanded from ONE expression text (SGR_FP_FLAVOURS, sgr_common.h): f<true> evaluates operation by operation (the
// camera correction's declared order, the actor prune rule), f<> takes the state of the including translation unit
// (sgr_actor_pose.hip includes this header below its own file pragma, so there both are op by op).
#pragma once
#include "sgr_common.h"
#include <math.h>

#define SGR_Q_HD static __host__ __device__ __forceinline__

#define SGR_Q_EPS 1e-12f  // F.normalize's eps

struct Q4 { float w, x, y, z; };  // real part first

// No multiply feeds an add in these: one flavour.
SGR_Q_HD Q4 qload(const float* p) { return Q4{p[0], p[1], p[2], p[3]}; }
SGR_Q_HD Q4 qconj(const Q4 a) { return Q4{a.w, -a.x, -a.y, -a.z}; }
SGR_Q_HD Q4 qadd(const Q4 a, const Q4 b) { return Q4{a.w + b.w, a.x + b.x, a.y + b.y, a.z + b.z}; }
SGR_Q_HD Q4 qdiv(const Q4 a, const float n) { return Q4{a.w / n, a.x / n, a.y / n, a.z / n}; }
SGR_Q_HD float sigmoidf_(const float x) { return 1.0f / (1.0f + expf(-x)); }

// ((a.w b.w + a.x b.x) + a.y b.y) + a.z b.z
template <bool NC = false>
SGR_Q_HD float qdot(const Q4 a, const Q4 b) {
    SGR_FP_FLAVOURS(return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;)
}
template <bool NC = false>
SGR_Q_HD float qlen(const Q4 a) { return sqrtf(qdot<NC>(a, a)); }
// quaternion_raw_multiply (general_utils.py:220-238)
template <bool NC = false>
SGR_Q_HD Q4 qmul(const Q4 a, const Q4 b) {
    SGR_FP_FLAVOURS(return Q4{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                             a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};)
}

// torch.nn.functional.normalize: y = a / n, n = max(|a|, eps) (the clamped norm is returned for the backward)
template <bool NC = false>
SGR_Q_HD Q4 qnormalize(const Q4 a, float& n) {
    n = fmaxf(qlen<NC>(a), SGR_Q_EPS);
    return qdiv(a, n);
}
// Its backward: da = (dy - y (y . dy)) / n, or dy / n where the clamp held.  The CALLER says whether it held: torch's
// clamp_min passes the gradient at |a| == eps, so the compose passes `|a| < eps`; the actor poses keep only n and pass
// `n <= eps` (include/sgr_actor_pose.h).  The two differ at |a| == eps exactly, where deriving the decision in here from
// either quantity would change the other caller's bits (tests/test_quat_cpu.py holds both).
template <bool NC = false>
SGR_Q_HD Q4 qnormalize_bwd(const Q4 y, const float n, const Q4 dy, const bool clamped) {
    if (clamped) return qdiv(dy, n);
    const float d = qdot<NC>(y, dy);
    SGR_FP_FLAVOURS(return Q4{(dy.w - y.w * d) / n, (dy.x - y.x * d) / n, (dy.y - y.y * d) / n, (dy.z - y.z * d) / n};)
}

// quaternion_to_matrix (general_utils.py:125-146): divides by |q| (no eps), row-major R; also the unit quaternion and |q|
template <bool NC = false>
SGR_Q_HD void qtomat(const Q4 q, float (&R)[9], Q4& qn, float& norm) {
    norm = qlen<NC>(q);
    qn = qdiv(q, norm);
    const float r = qn.w, x = qn.x, y = qn.y, z = qn.z;
    SGR_FP_FLAVOURS(
        R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - r * z); R[2] = 2.f * (x * z + r * y);
        R[3] = 2.f * (x * y + r * z); R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - r * x);
        R[6] = 2.f * (x * z - r * y); R[7] = 2.f * (y * z + r * x); R[8] = 1.f - 2.f * (x * x + y * y);)
}
// One row of x' = R x + t: ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a, Ra = R + 3 a
template <bool NC = false>
SGR_Q_HD float rot_row(const float* Ra, const float* x, const float ta) {
    SGR_FP_FLAVOURS(return Ra[0] * x[0] + Ra[1] * x[1] + Ra[2] * x[2] + ta;)
}
// x <- R x + t
template <bool NC = false>
SGR_Q_HD void rot_apply(const float* R, const float* t, float (&x)[3]) {
    const float y[3] = {rot_row<NC>(R, x, t[0]), rot_row<NC>(R + 3, x, t[1]), rot_row<NC>(R + 6, x, t[2])};
    x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
}
// (R^T g)_b = (R_0b g_0 + R_1b g_1) + R_2b g_2: the gradient on x of x' = R x + t
template <bool NC = false>
SGR_Q_HD void rot_pullback(const float* R, const float* g, float* out) {
    SGR_FP_FLAVOURS(_Pragma("unroll") for (int b = 0; b < 3; b++) out[b] = R[b] * g[0] + R[3 + b] * g[1] + R[6 + b] * g[2];)
}
// dL/d(unit quaternion q) of x' = R(q) x from G[3a+b] = sum dx'_a x_b (general_utils.py:137-145)
template <bool NC = false>
SGR_Q_HD Q4 dquat_of_R(const Q4 q, const float* G) {
    const float r = q.w, x = q.x, y = q.y, z = q.z;
    Q4 d;
    SGR_FP_FLAVOURS(
        d.w = 2.f * (-z * G[1] + y * G[2] + z * G[3] - x * G[5] - y * G[6] + x * G[7]);
        d.x = 2.f * (y * G[1] + z * G[2] + y * G[3] - 2.f * x * G[4] - r * G[5] + z * G[6] + r * G[7] - 2.f * x * G[8]);
        d.y = 2.f * (-2.f * y * G[0] + x * G[1] + r * G[2] + x * G[3] + z * G[5] - r * G[6] + z * G[7] - 2.f * y * G[8]);
        d.z = 2.f * (-2.f * z * G[0] - r * G[1] + x * G[2] + r * G[3] - 2.f * z * G[4] + y * G[5] + x * G[6] + y * G[7]);)
    return d;
}
