// sgr_actor_pose.hip -- every actor's world pose of a frame in one launch (include/sgr_actor_pose.h) on gfx950.
//
// The work is tiny (tens of actors, a few hundred flops each); what it replaces is per actor four blocking reads and
// about sixty launches, so the design goal is launch count and the absence of host waits, not throughput:
//   - forward: one thread per actor, the record says which cells to read;
//   - backward: one thread per actor recomputes the forward and writes its 16 contributions, the same launch zeroes the
//     dense gradients; a second launch of ONE wave adds the contributions in (actor, sample, slot) order.  A cell is owned
//     by the lane group (cell & 15), its component by (lane & 3), so all adds into one address come from one lane in
//     program order: deterministic without atomics, and 16 independent add chains instead of one.
// The arithmetic is the header's contract, with contraction off for this file (pragma below, and -ffp-contract=off in
// build.py's PER_FILE_FLAGS).
#include <string>

#include "../../include/sgr_actor_pose.h"
#include "sgr_common.h"

#pragma clang fp contract(off)
#include "sgr_quat.h"  // below the pragma: its helpers take this file's state, so f<> and f<true> are the same here

static constexpr int SGR_AP_THREADS = 256;
static constexpr int SGR_AP_MAX_BLOCKS = 1024;

static_assert(sizeof(sgr_actor_pose_sample) == 32 && sizeof(sgr_actor_pose_record) == 96,
              "record layout of include/sgr_actor_pose.h");
static_assert(SGR_ACTOR_POSE_CONTRIB == 16 && SGR_ACTOR_POSE_PARTS == 23, "include/sgr_actor_pose.h");

namespace {

__device__ __forceinline__ Q4 mul_theta(const Q4 a, const float c, const float s) {
    return Q4{a.w * c - a.z * s, a.x * c + a.y * s, a.y * c - a.x * s, a.z * c + a.w * s};
}
// d mul_theta(a, t) / dt
__device__ __forceinline__ Q4 mul_theta_dt(const Q4 a, const float c, const float s) {
    return Q4{-(a.w * s) - a.z * c, a.y * c - a.x * s, -(a.y * s) - a.x * c, a.w * c - a.z * s};
}
// transpose of q -> mul_theta(q, t)
__device__ __forceinline__ Q4 mul_theta_T(const Q4 g, const float c, const float s) {
    return Q4{g.w * c + g.z * s, g.x * c - g.y * s, g.x * s + g.y * c, g.z * c - g.w * s};
}

struct Slerp {  // what the backward needs of one slerp
    Q4 a, b, p;  // normalised inputs, relative quaternion after the sign
    float n0, n1, sg, s, h, ang, c1, r;
    float v[3];
    float m, c2;
};

__device__ Q4 slerp_fwd(const Q4 q0, const Q4 q1, const float r, Slerp& S) {
    S.r = r;
    S.a = qnormalize(q0, S.n0);
    S.b = qnormalize(q1, S.n1);
    Q4 p = qmul(qconj(S.a), S.b);
    S.sg = p.w < 0.f ? -1.f : 1.f;
    p = Q4{p.w * S.sg, p.x * S.sg, p.y * S.sg, p.z * S.sg};
    S.p = p;
    S.s = sqrtf(p.x * p.x + p.y * p.y + p.z * p.z);
    S.h = atan2f(S.s, p.w);
    S.ang = 2.f * S.h;
    S.c1 = S.ang < 1e-3f ? 0.5f - S.ang * S.ang / 48.f : sinf(S.h) / S.ang;
    S.v[0] = p.x / S.c1 * r;
    S.v[1] = p.y / S.c1 * r;
    S.v[2] = p.z / S.c1 * r;
    S.m = sqrtf(S.v[0] * S.v[0] + S.v[1] * S.v[1] + S.v[2] * S.v[2]);
    const float hm = 0.5f * S.m;
    S.c2 = S.m < 1e-3f ? 0.5f - S.m * S.m / 48.f : sinf(hm) / S.m;
    const Q4 e{cosf(hm), S.v[0] * S.c2, S.v[1] * S.c2, S.v[2] * S.c2};
    return qmul(S.a, e);
}

__device__ void slerp_bwd(const Slerp& S, const Q4 gQ, Q4& g0, Q4& g1) {
    const float hm = 0.5f * S.m, shm = sinf(hm), chm = cosf(hm);
    const Q4 e{chm, S.v[0] * S.c2, S.v[1] * S.c2, S.v[2] * S.c2};
    // Q = a (x) e
    Q4 ga = qmul(gQ, qconj(e));
    const Q4 ge = qmul(qconj(S.a), gQ);
    // e = (cos(m / 2), v c2)
    float gv[3] = {ge.x * S.c2, ge.y * S.c2, ge.z * S.c2};
    const float gc2 = ge.x * S.v[0] + ge.y * S.v[1] + ge.z * S.v[2];
    const float dc2 = S.m < 1e-3f ? -S.m / 24.f : (0.5f * chm * S.m - shm) / (S.m * S.m);
    const float gm = -0.5f * shm * ge.w + gc2 * dc2;
    if (S.m > 0.f) {
        gv[0] += gm * (S.v[0] / S.m);
        gv[1] += gm * (S.v[1] / S.m);
        gv[2] += gm * (S.v[2] / S.m);
    }
    // v = p_xyz / c1 * r
    const float k = S.r / S.c1;
    Q4 gp{0.f, gv[0] * k, gv[1] * k, gv[2] * k};
    const float gc1 = -(gv[0] * S.p.x + gv[1] * S.p.y + gv[2] * S.p.z) * k / S.c1;
    const float dc1 = S.ang < 1e-3f ? -S.ang / 24.f : (0.5f * cosf(S.h) * S.ang - sinf(S.h)) / (S.ang * S.ang);
    const float gh = 2.f * gc1 * dc1;
    // h = atan2(s, p_w)
    const float den = S.s * S.s + S.p.w * S.p.w;
    const float gs = gh * (S.p.w / den);
    gp.w = -gh * (S.s / den);
    if (S.s > 0.f) {
        gp.x += gs * (S.p.x / S.s);
        gp.y += gs * (S.p.y / S.s);
        gp.z += gs * (S.p.z / S.s);
    }
    gp = Q4{gp.w * S.sg, gp.x * S.sg, gp.y * S.sg, gp.z * S.sg};
    // p = conj(a) (x) b
    ga = qadd(ga, qconj(qmul(gp, qconj(S.b))));
    const Q4 gb = qmul(S.a, gp);
    // the Slerp keeps only the clamped norms: n <= eps is "the clamp_min holds, a = q / 1e-12"
    g0 = qnormalize_bwd(S.a, S.n0, ga, S.n0 <= SGR_Q_EPS);
    g1 = qnormalize_bwd(S.b, S.n1, gb, S.n1 <= SGR_Q_EPS);
}

__device__ __forceinline__ bool cell_ok(const int c, const int n_cells) { return c >= 0 && c < n_cells; }

__device__ __forceinline__ bool record_ok(const sgr_actor_pose_record& rec, const int n_cells, const bool opt) {
    if (rec.n_samples != 1 && rec.n_samples != 2) return false;
    for (int i = 0; i < rec.n_samples; ++i) {
        const sgr_actor_pose_sample& s = rec.s[i];
        if (!cell_ok(s.a, n_cells) || !cell_ok(s.b, n_cells)) return false;
        if (opt && (!cell_ok(s.th1, n_cells) || !cell_ok(s.th2, n_cells))) return false;
    }
    return true;
}

struct SampleState {  // forward of one sample, kept for its backward
    Q4 qa0, qa;
    float c1, s1, c2, s2;
    Slerp S;
};

__device__ Q4 sample_fwd(const sgr_actor_pose_sample& sm, const float* __restrict__ input_trans,
                         const float* __restrict__ input_rots, const float* __restrict__ opt_trans,
                         const float* __restrict__ opt_rots, float T[3], SampleState& st, Q4& qb_out) {
    const bool opt = opt_trans != nullptr;
    for (int i = 0; i < 3; ++i) {
        float ta = input_trans[3 * sm.a + i], tb = input_trans[3 * sm.b + i];
        if (opt) {
            ta = ta + opt_trans[3 * sm.a + i];
            tb = tb + opt_trans[3 * sm.b + i];
        }
        T[i] = (ta * sm.wa + tb * sm.wb) / sm.wd;
    }
    st.qa0 = qload(input_rots + 4 * sm.a);
    Q4 qb;
    if (opt) {
        const float t1 = opt_rots[sm.th1], t2 = opt_rots[sm.th2];
        st.c1 = cosf(t1); st.s1 = sinf(t1); st.c2 = cosf(t2); st.s2 = sinf(t2);
        st.qa = mul_theta(st.qa0, st.c1, st.s1);
        qb = mul_theta(st.qa, st.c2, st.s2);
    } else {
        st.c1 = st.c2 = 1.f; st.s1 = st.s2 = 0.f;
        st.qa = st.qa0;
        qb = qload(input_rots + 4 * sm.b);
    }
    qb_out = qb;
    return slerp_fwd(st.qa, qb, sm.r, st.S);
}

__device__ Q4 matrix_to_quaternion(const float* __restrict__ E) {
    const float m00 = E[0], m01 = E[1], m02 = E[2], m10 = E[4], m11 = E[5], m12 = E[6], m20 = E[8], m21 = E[9], m22 = E[10];
    const float d[4] = {1.0f + m00 + m11 + m22, 1.0f + m00 - m11 - m22, 1.0f - m00 + m11 - m22, 1.0f - m00 - m11 + m22};
    float qa[4];
    int best = 0;
    for (int i = 0; i < 4; ++i) {
        qa[i] = d[i] > 0.f ? sqrtf(d[i]) : 0.f;
        if (qa[i] > qa[best]) best = i;
    }
    float row[4];
    const float sq = qa[best] * qa[best];
    switch (best) {
        case 0: row[0] = sq; row[1] = m21 - m12; row[2] = m02 - m20; row[3] = m10 - m01; break;
        case 1: row[0] = m21 - m12; row[1] = sq; row[2] = m10 + m01; row[3] = m02 + m20; break;
        case 2: row[0] = m02 - m20; row[1] = m10 + m01; row[2] = sq; row[3] = m12 + m21; break;
        default: row[0] = m10 - m01; row[1] = m20 + m02; row[2] = m21 + m12; row[3] = sq; break;
    }
    const float den = 2.0f * fmaxf(qa[best], 0.1f);
    return Q4{row[0] / den, row[1] / den, row[2] / den, row[3] / den};
}

__global__ void __launch_bounds__(SGR_AP_THREADS)
sgr_actor_pose_forward_kernel(const int K, const sgr_actor_pose_record* __restrict__ records, const int n_cells,
                              const float* __restrict__ input_trans, const float* __restrict__ input_rots,
                              const float* __restrict__ opt_trans, const float* __restrict__ opt_rots,
                              const float* __restrict__ ego, float* __restrict__ poses, float* __restrict__ parts) {
    const int k = blockIdx.x * SGR_AP_THREADS + threadIdx.x;
    if (k >= K) return;
    const sgr_actor_pose_record rec = records[k];
    float* out = poses + 7 * (size_t)k;
    if (!record_ok(rec, n_cells, opt_trans != nullptr)) {
        for (int i = 0; i < 7; ++i) out[i] = __builtin_nanf("");
        if (parts)
            for (int i = 0; i < SGR_ACTOR_POSE_PARTS; ++i) parts[SGR_ACTOR_POSE_PARTS * (size_t)k + i] = __builtin_nanf("");
        return;
    }
    SampleState st;
    float T[3];
    Q4 qb;
    Q4 Q = sample_fwd(rec.s[0], input_trans, input_rots, opt_trans, opt_rots, T, st, qb);
    if (parts) {
        float* p = parts + SGR_ACTOR_POSE_PARTS * (size_t)k;
        p[0] = T[0]; p[1] = T[1]; p[2] = T[2];
        p[3] = st.qa.w; p[4] = st.qa.x; p[5] = st.qa.y; p[6] = st.qa.z;
        p[7] = qb.w; p[8] = qb.x; p[9] = qb.y; p[10] = qb.z;
        p[11] = st.c1; p[12] = st.s1; p[13] = st.c2; p[14] = st.s2;
    }
    if (rec.n_samples == 2) {
        SampleState st2;
        float T2[3];
        Q4 qb2;
        const Q4 Q2 = sample_fwd(rec.s[1], input_trans, input_rots, opt_trans, opt_rots, T2, st2, qb2);
        for (int i = 0; i < 3; ++i) T[i] = (T[i] * rec.Wa + T2[i] * rec.Wb) / rec.Wd;
        Slerp So;
        Q = slerp_fwd(Q, Q2, rec.R, So);
    }
    const Q4 qe = matrix_to_quaternion(ego);
    const Q4 o = qmul(qe, Q);
    out[0] = o.w; out[1] = o.x; out[2] = o.y; out[3] = o.z;
    for (int i = 0; i < 3; ++i)
        out[4 + i] = ego[4 * i + 0] * T[0] + ego[4 * i + 1] * T[1] + ego[4 * i + 2] * T[2] + ego[4 * i + 3];
    if (parts) {
        float* p = parts + SGR_ACTOR_POSE_PARTS * (size_t)k;
        p[15] = qe.w; p[16] = qe.x; p[17] = qe.y; p[18] = qe.z;
        p[19] = Q.w; p[20] = Q.x; p[21] = Q.y; p[22] = Q.z;
    }
}

// gradient of one sample: gT, gQ -> its 8 contributions
__device__ void sample_bwd(const sgr_actor_pose_sample& sm, const SampleState& st, const float gT[3], const Q4 gQ,
                           float* __restrict__ c) {
    for (int i = 0; i < 3; ++i) {
        const float g = gT[i] / sm.wd;
        c[i] = g * sm.wa;
        c[3 + i] = g * sm.wb;
    }
    Q4 gqa, gqb;
    slerp_bwd(st.S, gQ, gqa, gqb);
    // qb = mul_theta(qa, theta2), qa = mul_theta(qa0, theta1)
    c[7] = qdot(gqb, mul_theta_dt(st.qa, st.c2, st.s2));
    gqa = qadd(gqa, mul_theta_T(gqb, st.c2, st.s2));
    c[6] = qdot(gqa, mul_theta_dt(st.qa0, st.c1, st.s1));
}

__global__ void __launch_bounds__(SGR_AP_THREADS)
sgr_actor_pose_backward_kernel(const int K, const sgr_actor_pose_record* __restrict__ records, const int n_cells,
                               const float* __restrict__ input_trans, const float* __restrict__ input_rots,
                               const float* __restrict__ opt_trans, const float* __restrict__ opt_rots,
                               const float* __restrict__ ego, const float* __restrict__ dposes,
                               float* __restrict__ contrib, float* __restrict__ d_opt_trans,
                               float* __restrict__ d_opt_rots) {
    const int tid = blockIdx.x * SGR_AP_THREADS + threadIdx.x;
    const int stride = gridDim.x * SGR_AP_THREADS;
    for (int i = tid; i < 3 * n_cells; i += stride) d_opt_trans[i] = 0.f;
    for (int i = tid; i < n_cells; i += stride) d_opt_rots[i] = 0.f;
    for (int k = tid; k < K; k += stride) {
        float* c = contrib + SGR_ACTOR_POSE_CONTRIB * (size_t)k;
        for (int i = 0; i < SGR_ACTOR_POSE_CONTRIB; ++i) c[i] = 0.f;
        const sgr_actor_pose_record rec = records[k];
        if (!record_ok(rec, n_cells, true)) continue;
        SampleState st, st2;
        Slerp So;
        float T[3], T2[3];
        Q4 qb;
        const Q4 Q1 = sample_fwd(rec.s[0], input_trans, input_rots, opt_trans, opt_rots, T, st, qb);
        const bool two = rec.n_samples == 2;
        if (two) {
            const Q4 Q2 = sample_fwd(rec.s[1], input_trans, input_rots, opt_trans, opt_rots, T2, st2, qb);
            slerp_fwd(Q1, Q2, rec.R, So);
        }
        // world pose: out_rot = qe (x) Q, out_trans = R T + t
        const float* g = dposes + 7 * (size_t)k;
        const Q4 qe = matrix_to_quaternion(ego);
        const Q4 gQ = qmul(qconj(qe), qload(g));
        float gT[3];
        for (int j = 0; j < 3; ++j) gT[j] = ego[0 + j] * g[4] + ego[4 + j] * g[5] + ego[8 + j] * g[6];
        if (two) {
            float gT1[3], gT2[3];
            for (int i = 0; i < 3; ++i) {
                const float q = gT[i] / rec.Wd;
                gT1[i] = q * rec.Wa;
                gT2[i] = q * rec.Wb;
            }
            Q4 gQ1, gQ2;
            slerp_bwd(So, gQ, gQ1, gQ2);
            sample_bwd(rec.s[0], st, gT1, gQ1, c);
            sample_bwd(rec.s[1], st2, gT2, gQ2, c + 8);
        } else {
            sample_bwd(rec.s[0], st, gT, gQ, c);
        }
    }
}

// ONE wave: lane = 4 * group + component; group g owns the cells with (cell & 15) == g, component 0..2 the translation
// axes and 3 the angle.  Every add into one address is made by one lane, in (actor, sample, slot) order.
__global__ void __launch_bounds__(64)
sgr_actor_pose_apply_kernel(const int K, const sgr_actor_pose_record* __restrict__ records, const int n_cells,
                            const float* __restrict__ contrib, float* __restrict__ d_opt_trans,
                            float* __restrict__ d_opt_rots) {
    const int comp = threadIdx.x & 3, grp = threadIdx.x >> 2;
    for (int k = 0; k < K; ++k) {
        const sgr_actor_pose_record rec = records[k];
        if (!record_ok(rec, n_cells, true)) continue;
        for (int s = 0; s < rec.n_samples; ++s) {
            const float* c = contrib + SGR_ACTOR_POSE_CONTRIB * (size_t)k + 8 * s;
            for (int slot = 0; slot < 2; ++slot) {
                if (comp < 3) {
                    const int cell = slot ? rec.s[s].b : rec.s[s].a;
                    if ((cell & 15) == grp) d_opt_trans[3 * cell + comp] += c[3 * slot + comp];
                } else {
                    const int cell = slot ? rec.s[s].th2 : rec.s[s].th1;
                    if ((cell & 15) == grp) d_opt_rots[cell] += c[6 + slot];
                }
            }
        }
    }
}

int check_args(const char* what, int K, const void* records, int n_cells, const void* input_trans, const void* input_rots,
               const void* opt_trans, const void* opt_rots, const void* ego) {
    if (K < 0 || n_cells < 0) return sgr_set_error(SGR_E_INVALID, std::string(what) + ": negative size");
    if (n_cells > INT32_MAX / 4) return sgr_set_error(SGR_E_INVALID, std::string(what) + ": too many cells");
    if ((opt_trans == nullptr) != (opt_rots == nullptr))
        return sgr_set_error(SGR_E_INVALID, std::string(what) + ": opt_trans and opt_rots go together");
    if (K > 0 && (!records || !input_trans || !input_rots || !ego || n_cells == 0))
        return sgr_set_error(SGR_E_INVALID, std::string(what) + ": K > 0 needs records, the tracklet tables and ego");
    return 0;
}

}  // namespace

int sgr_actor_pose_backward_max_blocks(void) { return SGR_AP_MAX_BLOCKS; }

int sgr_actor_pose_forward(int K, const sgr_actor_pose_record* records, int n_cells, const float* input_trans,
                           const float* input_rots, const float* opt_trans, const float* opt_rots, const float* ego,
                           float* poses, float* parts, void* stream_) {
    if (int rc = check_args("actor_pose_forward", K, records, n_cells, input_trans, input_rots, opt_trans, opt_rots, ego))
        return rc;
    if (K == 0) return 0;
    if (!poses) return sgr_set_error(SGR_E_INVALID, "actor_pose_forward: no output");
    const unsigned grid = (unsigned)((K + SGR_AP_THREADS - 1) / SGR_AP_THREADS);
    sgr_actor_pose_forward_kernel<<<grid, SGR_AP_THREADS, 0, (hipStream_t)stream_>>>(
        K, records, n_cells, input_trans, input_rots, opt_trans, opt_rots, ego, poses, parts);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_actor_pose_backward(int K, const sgr_actor_pose_record* records, int n_cells, const float* input_trans,
                            const float* input_rots, const float* opt_trans, const float* opt_rots, const float* ego,
                            const float* dposes, float* contrib, float* d_opt_trans, float* d_opt_rots, void* stream_) {
    if (int rc = check_args("actor_pose_backward", K, records, n_cells, input_trans, input_rots, opt_trans, opt_rots, ego))
        return rc;
    if (!opt_trans) return sgr_set_error(SGR_E_INVALID, "actor_pose_backward: needs opt_trans and opt_rots");
    if (n_cells > 0 && (!d_opt_trans || !d_opt_rots)) return sgr_set_error(SGR_E_INVALID, "actor_pose_backward: no output");
    if (K > 0 && (!dposes || !contrib)) return sgr_set_error(SGR_E_INVALID, "actor_pose_backward: no dposes / contrib");
    if (n_cells == 0) return 0;
    const int64_t work = (int64_t)3 * n_cells > K ? (int64_t)3 * n_cells : K;
    int64_t blocks = (work + SGR_AP_THREADS - 1) / SGR_AP_THREADS;
    if (blocks > SGR_AP_MAX_BLOCKS) blocks = SGR_AP_MAX_BLOCKS;
    sgr_actor_pose_backward_kernel<<<(unsigned)blocks, SGR_AP_THREADS, 0, (hipStream_t)stream_>>>(
        K, records, n_cells, input_trans, input_rots, opt_trans, opt_rots, ego, dposes, contrib, d_opt_trans, d_opt_rots);
    SGR_HIP(hipGetLastError());
    if (K > 0) {
        sgr_actor_pose_apply_kernel<<<1, 64, 0, (hipStream_t)stream_>>>(K, records, n_cells, contrib, d_opt_trans, d_opt_rots);
        SGR_HIP(hipGetLastError());
    }
    return 0;
}
