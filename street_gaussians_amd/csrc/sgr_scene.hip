// sgr_scene.hip -- scene-graph rows next to the rasterizer (include/sgr_scene.h).
//
// n1  compose: background + posed actors -> the rasterizer's flat inputs, forward and backward.  The reference does
//     this with ~40 torch ops per iteration (per-attribute cat, clone, masked flips, einsum, quaternion products,
//     normalize; street_gaussian_model.py:287-449) that each stream the whole attribute through HBM.  Here every
//     parameter is read once and every output written once:
//       * one workgroup per CHUNK (<= 256 consecutive Gaussians of one model, table built on the host), one lane per
//         Gaussian for the small attributes;
//       * SH rows move with one lane per FLOAT (coalesced on both sides; a lane-per-Gaussian copy of 45-float rows is
//         issue-bound on CDNA4: 64 cache lines per load instruction);
//       * the pose gradient of an actor (rotation 4 + translation 3) is a reduction over its Gaussians: per-chunk
//         partial sums in a fixed order, then one small kernel per actor sums its chunks in order -> deterministic.
//     Per frame (include/sgr_scene_frame.h): the camera pose correction of the static segments, whose gradient is the
//     same 16-sum reduction over the background (thousands of chunks: two fixed-order levels instead of one wave), and
//     zero spans for the gradient blocks of the models absent from the frame.
// n12 the backward kernels in a second flavour (STEP = 1) whose sink is the optimiser (include/sgr_scene_step.h): where
//     the plain flavour stores g into a gradient array, it applies adam1(p, g, m, v) to that element.
// n2  densification statistics scattered back per model in one pass (street_gaussian_model.py:551-571).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sgr_scene.h"
#include "../../include/sgr_scene_frame.h"
#include "../../include/sgr_scene_step.h"
#include "sgr_adam_math.h"
#include "sgr_common.h"
#include "sgr_quat.h"

#define SGR_SC_THREADS 256
#define SGR_SC_NPART 16  // per-chunk partials of an actor: G[9] (sum dx' x^T), T[3] (sum dx'), Q[4] (rotation path)

struct SgrChunk {
    int32_t seg, start, n, out;  // segment, first Gaussian inside it, Gaussians, first output row
};
struct SgrSegDev {
    sgr_scene_segment s;
    sgr_scene_segment_grads g;
    int32_t first_chunk, nchunks;
    int32_t corr_first;  // static segment under a correction: ordinal of its first chunk among the corrected chunks
};

// ---- camera pose correction (include/sgr_scene_frame.h): the declared order, contraction off (sgr_quat.h: f<true>) ----
struct SgrCorr {
    Q4 raw, qc, qq;     // c[0:4], F.normalize(c[0:4]), qc / |qc|
    float nc, n2;       // max(|raw|, 1e-12), |qc|
    float R[9], t[3];
};
__device__ __forceinline__ SgrCorr corr_load(const float* __restrict__ c) {
    SgrCorr k;
    k.raw = qload(c);
    k.qc = qnormalize<true>(k.raw, k.nc);
    qtomat<true>(k.qc, k.R, k.qq, k.n2);
    k.t[0] = c[4]; k.t[1] = c[5]; k.t[2] = c[6];
    return k;
}

// ---- the fixed-order sums of a 256-thread workgroup's 16 values: wave butterfly, then waves 0..3 in order -------------
__device__ __forceinline__ void sum16_fixed(float (&v)[SGR_SC_NPART], float (&red)[SGR_SC_THREADS / 64][SGR_SC_NPART]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SGR_SC_NPART; k++) {
        float a = v[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
        if (lane == 0) red[wave][k] = a;
    }
    __syncthreads();
}
__device__ __forceinline__ float sum16_waves(const float (&red)[SGR_SC_THREADS / 64][SGR_SC_NPART], int k) {
    return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// ---- forward: small attributes, one lane per Gaussian ---------------------------------------------------------
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_fwd_kernel(const SgrChunk* __restrict__ chunks, const SgrSegDev* __restrict__ segs, int S,
                     float* __restrict__ means3D, float* __restrict__ rotations, float* __restrict__ scales,
                     float* __restrict__ opacities, float* __restrict__ semantics, const float* __restrict__ corr) {
    const SgrChunk c = chunks[blockIdx.x];
    const sgr_scene_segment& sg = segs[c.seg].s;
    if ((int)threadIdx.x >= c.n) return;
    const size_t i = (size_t)c.start + threadIdx.x, o = (size_t)c.out + threadIdx.x;
    float x[3] = {sg.xyz[3 * i], sg.xyz[3 * i + 1], sg.xyz[3 * i + 2]};
    const float4 qr = *reinterpret_cast<const float4*>(sg.rotation + 4 * i);
    float n;
    Q4 q = qnormalize({qr.x, qr.y, qr.z, qr.w}, n);  // gaussian_model.py:229-230
    if (sg.kind == SGR_SEG_ACTOR) {
        if (sg.flip_mask && sg.flip_mask[i]) {  // street_gaussian_model.py:324-327, 354-356
            x[sg.flip_axis] = -x[sg.flip_axis];
            q = qmul(qload(sg.flip_quat), q);
        }
        const Q4 po = qload(sg.pose);
        float R[9], pn;
        Q4 pq;
        qtomat(po, R, pq, pn);          // :357
        rot_apply(R, sg.pose + 4, x);   // :358
        float n2;
        q = qnormalize(qmul(po, q), n2);  // :328-329
    } else if (corr) {  // camera pose correction (camera_pose.py:89-114, street_gaussian_model.py:311-312, 340-341)
        const SgrCorr k = corr_load(corr);
        rot_apply<true>(k.R, k.t, x);
        q = qmul<true>(k.qc, q);
    }
    means3D[3 * o] = x[0]; means3D[3 * o + 1] = x[1]; means3D[3 * o + 2] = x[2];
    *reinterpret_cast<float4*>(rotations + 4 * o) = make_float4(q.w, q.x, q.y, q.z);
#pragma unroll
    for (int k = 0; k < 3; k++) scales[3 * o + k] = expf(sg.scaling[3 * i + k]);  // gaussian_model.py:225-226
    opacities[o] = sigmoidf_(sg.opacity[i]);                                        // :250-251
    if (S > 0) {
        float* out = semantics + o * (size_t)S;
        if (sg.semantic == nullptr) {
            for (int k = 0; k < S; k++) out[k] = 0.f;
        } else if (sg.kind == SGR_SEG_ACTOR) {  // gaussian_model_actor.py:62-69
            const float v = sg.semantic[i];
            for (int k = 0; k < S; k++) out[k] = 0.f;
            if (sg.class_label >= 0 && sg.class_label < S)
                out[sg.class_label] = sg.sem_mode == SGR_SEM_PROBABILITIES ? sigmoidf_(v) : v;
        } else if (sg.sem_mode == SGR_SEM_PROBABILITIES) {  // gaussian_model.py:247-248: softmax over the classes
            const float* in = sg.semantic + i * (size_t)S;
            float m = in[0];
            for (int k = 1; k < S; k++) m = fmaxf(m, in[k]);
            float sum = 0.f;
            for (int k = 0; k < S; k++) sum += expf(in[k] - m);
            for (int k = 0; k < S; k++) out[k] = expf(in[k] - m) / sum;
        }  // static logits: copied by the SH kernel, one lane per float
    }
}

// ---- forward: SH rows, one lane per float (get_features :366-381, get_features_fourier actor.py:71-80) ----------
// MC = M when it is known at compile time (16: divisions by the row length become multiplies), 0 = runtime M.
// Static models with logit semantics (a plain copy, gaussian_model.py:243-246) are also moved here, one lane per float.
template <int MC>
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_sh_fwd_kernel(const SgrChunk* __restrict__ chunks, const SgrSegDev* __restrict__ segs, int M_, int S,
                        float* __restrict__ shs, float* __restrict__ semantics) {
    const SgrChunk c = chunks[blockIdx.x];
    const sgr_scene_segment& sg = segs[c.seg].s;
    const int M = MC ? MC : M_;
    const int row = 3 * M, rest = 3 * (M - 1), C = sg.fourier_dim;
    if (S > 0 && sg.semantic && sg.kind == SGR_SEG_STATIC && sg.sem_mode == SGR_SEM_LOGITS) {
        const float* in = sg.semantic + (size_t)c.start * S;
        float* so = semantics + (size_t)c.out * S;
        for (int e = threadIdx.x; e < c.n * S; e += SGR_SC_THREADS) so[e] = in[e];
    }
    float* out = shs + (size_t)c.out * row;
    for (int e = threadIdx.x; e < c.n * row; e += SGR_SC_THREADS) {
        const int g = e / row, j = e - g * row;
        const size_t i = (size_t)c.start + g;
        float v;
        if (j < 3) {
            const float* dc = sg.features_dc + i * (size_t)C * 3 + j;
            if (sg.kind == SGR_SEG_ACTOR && sg.idft) {
                v = 0.f;
                for (int k = 0; k < C; k++) v += dc[3 * k] * sg.idft[k];
            } else {
                v = dc[0];
            }
        } else {
            v = sg.features_rest[i * (size_t)rest + (j - 3)];
        }
        out[e] = v;
    }
}

// ---- n12: the sink of a gradient value (include/sgr_scene_step.h) -------------------------------------------------
// SGR_SINK(grad, param, group, e, g).  STEP = 0: g is stored at grad[e].  STEP = 1: element e of the group's block takes
// one Adam step with g (adam1 keeps contraction off in its own body: a multiply that formed g stays a multiply and g
// enters rounded to f32 as the plain flavour stores it).  The lane's last read of param[e] comes before the sink.
struct SgrStepArgs {
    const sgr_scene_step* steps;  // parallel to the segment table
    AdamConsts k;
    float eps;
};
// the group's record, read once per use site (uniform: scalar loads); nothing is read in the plain flavour
template <int STEP>
__device__ __forceinline__ sgr_scene_step_group sink_group(const sgr_scene_step_group* sp, int group) {
    if constexpr (STEP) return sp[group];
    else return sgr_scene_step_group{nullptr, nullptr, 0.f, 0.f};
}
// the record of the block that starts b elements into the group's
template <int STEP>
__device__ __forceinline__ sgr_scene_step_group sink_at(sgr_scene_step_group sg, size_t b) {
    if constexpr (STEP) { sg.m += b; sg.v += b; }
    return sg;
}
template <int STEP>
__device__ __forceinline__ bool sink_wants(const float* grad, const sgr_scene_step_group& sg) {
    return STEP ? sg.m != nullptr : grad != nullptr;
}
__device__ __forceinline__ void sink_step(const float* param, const sgr_scene_step_group& sg, const SgrStepArgs& a, size_t e,
                                          float g) {
    float* pp = const_cast<float*>(param) + e;
    float p = *pp, m = sg.m[e], v = sg.v[e];
    adam1(p, g, m, v, a.k, sg.step_size, sg.bc2_sqrt, a.eps);
    *pp = p;
    sg.m[e] = m;
    sg.v[e] = v;
}
// one source text for the value in both flavours; the plain flavour's statement is the store it has always been
#define SGR_SINK(grad, param, group, e, value)                        \
    do {                                                              \
        if constexpr (STEP) sink_step(param, group, sa, e, value);    \
        else (grad)[e] = value;                                       \
    } while (0)

// ---- backward: small attributes + per-chunk pose partials ------------------------------------------------------
// One Gaussian's 16 partials of the rigid motion x' = R x + t, rot' = a (x) b, from dx (on x') and du (on the product):
// G = dx x^T, T = dx, Q = du b* (d(a b)/da . dO = dO b*).  dx becomes R^T dx; returns a* du (d(a b)/db . dO = a* dO).
__device__ __forceinline__ Q4 rigid_partials(const float (&R)[9], const float (&x)[3], const Q4 a, const Q4 b, const Q4 du,
                                             float (&dx)[3], float (&part)[SGR_SC_NPART]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) part[3 * r + c] = dx[r] * x[c];
        part[9 + r] = dx[r];
    }
    float dl[3];
    rot_pullback(R, dx, dl);
    dx[0] = dl[0]; dx[1] = dl[1]; dx[2] = dl[2];
    const Q4 da = qmul(du, qconj(b));
    part[12] = da.w; part[13] = da.x; part[14] = da.y; part[15] = da.z;
    return qmul(qconj(a), du);
}

template <int STEP>
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_bwd_kernel(const SgrChunk* __restrict__ chunks, const SgrSegDev* __restrict__ segs, int S,
                     const float* __restrict__ dmeans, const float* __restrict__ drot, const float* __restrict__ dscale,
                     const float* __restrict__ dopac, const float* __restrict__ dsem, float* __restrict__ partials,
                     const float* __restrict__ corr, float* __restrict__ cpart, const SgrStepArgs sa) {
    __shared__ float red[SGR_SC_THREADS / 64][SGR_SC_NPART];
    const SgrChunk c = chunks[blockIdx.x];
    const SgrSegDev& sd = segs[c.seg];
    const sgr_scene_segment& sg = sd.s;
    const sgr_scene_segment_grads& gr = sd.g;
    const sgr_scene_step_group* sp = STEP ? sa.steps[c.seg].group : nullptr;
    const sgr_scene_step_group kxyz = sink_group<STEP>(sp, SGR_STEP_XYZ), krot = sink_group<STEP>(sp, SGR_STEP_ROTATION),
                               kscl = sink_group<STEP>(sp, SGR_STEP_SCALING), kopa = sink_group<STEP>(sp, SGR_STEP_OPACITY),
                               ksem = sink_group<STEP>(sp, SGR_STEP_SEMANTIC);
    const bool live = (int)threadIdx.x < c.n;
    const size_t i = (size_t)c.start + (live ? threadIdx.x : 0), o = (size_t)c.out + (live ? threadIdx.x : 0);
    float part[SGR_SC_NPART];
#pragma unroll
    for (int k = 0; k < SGR_SC_NPART; k++) part[k] = 0.f;
    if (live) {
        float dx[3] = {dmeans ? dmeans[3 * o] : 0.f, dmeans ? dmeans[3 * o + 1] : 0.f, dmeans ? dmeans[3 * o + 2] : 0.f};
        Q4 dq = {0.f, 0.f, 0.f, 0.f};
        if (drot) {
            const float4 t = *reinterpret_cast<const float4*>(drot + 4 * o);
            dq = {t.x, t.y, t.z, t.w};
        }
        const float4 qr = *reinterpret_cast<const float4*>(sg.rotation + 4 * i);
        const Q4 qraw = {qr.x, qr.y, qr.z, qr.w};
        float n;
        const Q4 ql0 = qnormalize(qraw, n);
        const bool clamped = qlen(qraw) < SGR_Q_EPS;
        if (sg.kind == SGR_SEG_ACTOR) {  // x' = R(po) x + t, rot' = normalize(po (x) ql), after the flip of x and ql0
            const bool flip = sg.flip_mask && sg.flip_mask[i];
            const Q4 fq = qload(sg.flip_quat);
            float x[3] = {sg.xyz[3 * i], sg.xyz[3 * i + 1], sg.xyz[3 * i + 2]};
            if (flip) x[sg.flip_axis] = -x[sg.flip_axis];
            const Q4 ql = flip ? qmul(fq, ql0) : ql0;
            const Q4 po = qload(sg.pose);
            float R[9], pn, n2;
            Q4 pq;
            qtomat(po, R, pq, pn);
            const Q4 u = qmul(po, ql);
            const Q4 r = qnormalize(u, n2);
            const Q4 du = qnormalize_bwd(r, n2, dq, qlen(u) < SGR_Q_EPS);
            dq = rigid_partials(R, x, po, ql, du, dx, part);
            if (flip) {
                dx[sg.flip_axis] = -dx[sg.flip_axis];
                dq = qmul(qconj(fq), dq);
            }
        } else if (corr) {  // x' = R x + t, rot' = qc (x) ql0: the same partials as an actor's, over the background
            const SgrCorr k = corr_load(corr);
            const float x[3] = {sg.xyz[3 * i], sg.xyz[3 * i + 1], sg.xyz[3 * i + 2]};
            dq = rigid_partials(k.R, x, k.qc, ql0, dq, dx, part);
        }
        if (sink_wants<STEP>(gr.xyz, kxyz)) {
            SGR_SINK(gr.xyz, sg.xyz, kxyz, 3 * i, dx[0]);
            SGR_SINK(gr.xyz, sg.xyz, kxyz, 3 * i + 1, dx[1]);
            SGR_SINK(gr.xyz, sg.xyz, kxyz, 3 * i + 2, dx[2]);
        }
        if (sink_wants<STEP>(gr.rotation, krot)) {
            const Q4 d = qnormalize_bwd(ql0, n, dq, clamped);
            if constexpr (STEP) {  // the row as float4, like the plain store: p is the row read above
                const sgr_scene_step_group& sgp = krot;
                float4 p = qr, m = *reinterpret_cast<const float4*>(sgp.m + 4 * i), v = *reinterpret_cast<const float4*>(sgp.v + 4 * i);
                adam1(p.x, d.w, m.x, v.x, sa.k, sgp.step_size, sgp.bc2_sqrt, sa.eps);
                adam1(p.y, d.x, m.y, v.y, sa.k, sgp.step_size, sgp.bc2_sqrt, sa.eps);
                adam1(p.z, d.y, m.z, v.z, sa.k, sgp.step_size, sgp.bc2_sqrt, sa.eps);
                adam1(p.w, d.z, m.w, v.w, sa.k, sgp.step_size, sgp.bc2_sqrt, sa.eps);
                *reinterpret_cast<float4*>(const_cast<float*>(sg.rotation) + 4 * i) = p;
                *reinterpret_cast<float4*>(sgp.m + 4 * i) = m;
                *reinterpret_cast<float4*>(sgp.v + 4 * i) = v;
            } else {
                *reinterpret_cast<float4*>(gr.rotation + 4 * i) = make_float4(d.w, d.x, d.y, d.z);
            }
        }
        if (sink_wants<STEP>(gr.scaling, kscl)) {
#pragma unroll
            for (int k = 0; k < 3; k++)  // element k is read before it is written, and only by this lane
                SGR_SINK(gr.scaling, sg.scaling, kscl, 3 * i + k, (dscale ? dscale[3 * o + k] : 0.f) * expf(sg.scaling[3 * i + k]));
        }
        if (sink_wants<STEP>(gr.opacity, kopa)) {
            const float sgm = sigmoidf_(sg.opacity[i]);
            SGR_SINK(gr.opacity, sg.opacity, kopa, i, (dopac ? dopac[o] : 0.f) * sgm * (1.f - sgm));
        }
        if (sink_wants<STEP>(gr.semantic, ksem) && sg.semantic) {
            if (S <= 0 || !dsem) {
                const int cols = sg.kind == SGR_SEG_ACTOR ? 1 : S;
                for (int k = 0; k < cols; k++) SGR_SINK(gr.semantic, sg.semantic, ksem, i * (size_t)cols + k, 0.f);
            } else if (sg.kind == SGR_SEG_ACTOR) {
                float d = (sg.class_label >= 0 && sg.class_label < S) ? dsem[o * (size_t)S + sg.class_label] : 0.f;
                if (sg.sem_mode == SGR_SEM_PROBABILITIES) {
                    const float sgm = sigmoidf_(sg.semantic[i]);
                    d *= sgm * (1.f - sgm);
                }
                SGR_SINK(gr.semantic, sg.semantic, ksem, i, d);
            } else if (sg.sem_mode == SGR_SEM_PROBABILITIES) {
                const float* in = sg.semantic + i * (size_t)S;
                const float* d = dsem + o * (size_t)S;
                float m = in[0];
                for (int k = 1; k < S; k++) m = fmaxf(m, in[k]);
                float sum = 0.f, pd = 0.f;
                for (int k = 0; k < S; k++) sum += expf(in[k] - m);
                for (int k = 0; k < S; k++) pd += expf(in[k] - m) / sum * d[k];
                for (int k = 0; k < S; k++)  // in[k] is read for the last time in the iteration that writes element k
                    SGR_SINK(gr.semantic, sg.semantic, ksem, i * (size_t)S + k, expf(in[k] - m) / sum * (d[k] - pd));
            }  // static logits: copied by the SH kernel, one lane per float
        }
    }
    // uniform per workgroup: an actor's chunk sums go to its slot of `partials`, a corrected static chunk's to `cpart`
    float* dst = nullptr;
    if (sg.kind == SGR_SEG_ACTOR) dst = partials ? partials + (size_t)blockIdx.x * SGR_SC_NPART : nullptr;
    else if (corr && cpart) dst = cpart + (size_t)(sd.corr_first + (int)blockIdx.x - sd.first_chunk) * SGR_SC_NPART;
    if (dst == nullptr) return;
    sum16_fixed(part, red);
    if (threadIdx.x < SGR_SC_NPART) dst[threadIdx.x] = sum16_waves(red, threadIdx.x);
}

// one workgroup (one wave) per actor: sum its chunks in order, then chain into the 7 pose parameters
__global__ void __launch_bounds__(64)
sgr_scene_pose_bwd_kernel(const SgrSegDev* __restrict__ segs, const float* __restrict__ partials) {
    const SgrSegDev& sd = segs[blockIdx.x];
    if (sd.s.kind != SGR_SEG_ACTOR || sd.g.pose == nullptr) return;
    __shared__ float tot[SGR_SC_NPART];
    if (threadIdx.x < SGR_SC_NPART) {
        float a = 0.f;
        for (int c = 0; c < sd.nchunks; c++) a += partials[(size_t)(sd.first_chunk + c) * SGR_SC_NPART + threadIdx.x];
        tot[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float R[9], pn;
    Q4 q;
    qtomat(qload(sd.s.pose), R, q, pn);
    const Q4 dpo = qnormalize_bwd(q, pn, dquat_of_R(q, tot), false);  // tot[0:9] = G, through quaternion_to_matrix's own |q|
    sd.g.pose[0] = dpo.w + tot[12];
    sd.g.pose[1] = dpo.x + tot[13];
    sd.g.pose[2] = dpo.y + tot[14];
    sd.g.pose[3] = dpo.z + tot[15];
    sd.g.pose[4] = tot[9];
    sd.g.pose[5] = tot[10];
    sd.g.pose[6] = tot[11];
}

// correction, level 2: workgroup b sums the corrected chunks [256 b, 256 b + 256) (one per lane) in a fixed order
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_corr_sum_kernel(const float* __restrict__ cpart, int nc, float* __restrict__ gpart) {
    __shared__ float red[SGR_SC_THREADS / 64][SGR_SC_NPART];
    const int j = blockIdx.x * SGR_SC_THREADS + threadIdx.x;
    float v[SGR_SC_NPART];
#pragma unroll
    for (int k = 0; k < SGR_SC_NPART; k += 4) {
        const float4 t = j < nc ? *reinterpret_cast<const float4*>(cpart + (size_t)j * SGR_SC_NPART + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
    }
    sum16_fixed(v, red);
    if (threadIdx.x < SGR_SC_NPART) gpart[(size_t)blockIdx.x * SGR_SC_NPART + threadIdx.x] = sum16_waves(red, threadIdx.x);
}

// correction, level 3: one workgroup sums the ng groups (lane l: groups l, l + 256, ... in order), then one lane chains
// through R(qq), qq = qc / |qc| and qc = F.normalize(raw) into the 7 correction gradients
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_corr_final_kernel(const float* __restrict__ gpart, int ng, const float* __restrict__ corr, float* __restrict__ out) {
    __shared__ float red[SGR_SC_THREADS / 64][SGR_SC_NPART];
    float v[SGR_SC_NPART];
#pragma unroll
    for (int k = 0; k < SGR_SC_NPART; k++) v[k] = 0.f;
    for (int j = threadIdx.x; j < ng; j += SGR_SC_THREADS) {
#pragma unroll
        for (int k = 0; k < SGR_SC_NPART; k++) v[k] += gpart[(size_t)j * SGR_SC_NPART + k];
    }
    sum16_fixed(v, red);
    if (threadIdx.x != 0) return;
    float tot[SGR_SC_NPART];
#pragma unroll
    for (int k = 0; k < SGR_SC_NPART; k++) tot[k] = sum16_waves(red, k);
    const SgrCorr c = corr_load(corr);
    Q4 dqc = qnormalize_bwd(c.qq, c.n2, dquat_of_R(c.qq, tot), false);  // quaternion_to_matrix's own |q| (no eps)
    dqc = qadd(dqc, qload(tot + 12));
    const Q4 d = qnormalize_bwd(c.qc, c.nc, dqc, qlen<true>(c.raw) < SGR_Q_EPS);  // F.normalize
    out[0] = d.w; out[1] = d.x; out[2] = d.y; out[3] = d.z;
    out[4] = tot[9]; out[5] = tot[10]; out[6] = tot[11];
}

// zero spans: workgroup b clears SGR_SC_ZSPAN floats of the span whose block range holds b (binary search)
#define SGR_SC_ZSPAN 4096
struct SgrZeroDev {
    float* ptr;
    size_t count;
    uint32_t first_block;
};
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_zero_kernel(const SgrZeroDev* __restrict__ spans, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (spans[mid].first_block <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const SgrZeroDev s = spans[lo];
    const size_t base = (size_t)(blockIdx.x - s.first_block) * SGR_SC_ZSPAN;
#pragma unroll 4
    for (int k = 0; k < SGR_SC_ZSPAN / SGR_SC_THREADS; k++) {
        const size_t e = base + (size_t)k * SGR_SC_THREADS + threadIdx.x;
        if (e < s.count) s.ptr[e] = 0.f;
    }
}

// ---- backward: SH rows, one lane per float of each gradient array ----------------------------------------------
// STEP = 1 steps the element in place of the store (SGR_SINK); the SH rows' gradients read no parameter.
template <int MC, int STEP>
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_sh_bwd_kernel(const SgrChunk* __restrict__ chunks, const SgrSegDev* __restrict__ segs, int M_, int S,
                        const float* __restrict__ dshs, const float* __restrict__ dsem, const SgrStepArgs sa) {
    const SgrChunk c = chunks[blockIdx.x];
    const SgrSegDev& sd = segs[c.seg];
    const sgr_scene_step_group* sp = STEP ? sa.steps[c.seg].group : nullptr;
    const int M = MC ? MC : M_;
    const int row = 3 * M, rest = 3 * (M - 1), C = sd.s.fourier_dim;
    const sgr_scene_step_group ksem = sink_group<STEP>(sp, SGR_STEP_SEMANTIC), krest = sink_group<STEP>(sp, SGR_STEP_F_REST),
                               kdc = sink_group<STEP>(sp, SGR_STEP_F_DC);
    if (S > 0 && dsem && sink_wants<STEP>(sd.g.semantic, ksem) && sd.s.semantic && sd.s.kind == SGR_SEG_STATIC &&
        sd.s.sem_mode == SGR_SEM_LOGITS) {
        const float* in = dsem + (size_t)c.out * S;
        const size_t b = (size_t)c.start * S;  // the chunk's first element of the segment's block
        float* so = STEP ? nullptr : sd.g.semantic + b;
        const sgr_scene_step_group kb = sink_at<STEP>(ksem, b);
        for (int e = threadIdx.x; e < c.n * S; e += SGR_SC_THREADS) SGR_SINK(so, sd.s.semantic + b, kb, e, in[e]);
    }
    const float* in = dshs + (size_t)c.out * row;
    if (sink_wants<STEP>(sd.g.features_rest, krest)) {
        const size_t b = (size_t)c.start * rest;
        float* out = STEP ? nullptr : sd.g.features_rest + b;
        const sgr_scene_step_group kb = sink_at<STEP>(krest, b);
        for (int e = threadIdx.x; e < c.n * rest; e += SGR_SC_THREADS) {
            const int g = e / rest, j = e - g * rest;
            SGR_SINK(out, sd.s.features_rest + b, kb, e, dshs ? in[g * row + 3 + j] : 0.f);
        }
    }
    if (sink_wants<STEP>(sd.g.features_dc, kdc)) {
        const size_t b = (size_t)c.start * C * 3;
        float* out = STEP ? nullptr : sd.g.features_dc + b;
        const sgr_scene_step_group kb = sink_at<STEP>(kdc, b);
        const bool four = sd.s.kind == SGR_SEG_ACTOR && sd.s.idft;
        for (int e = threadIdx.x; e < c.n * C * 3; e += SGR_SC_THREADS) {
            const int g = e / (C * 3), j = e - g * (C * 3), k = j / 3, ch = j - 3 * k;
            const float d = dshs ? in[g * row + ch] : 0.f;
            SGR_SINK(out, sd.s.features_dc + b, kb, e, four ? d * sd.s.idft[k] : (k == 0 ? d : 0.f));
        }
    }
}

// ---- n2: densification statistics ---------------------------------------------------------------------------
struct SgrStatSegDev { sgr_scene_stats_segment s; };
__global__ void __launch_bounds__(SGR_SC_THREADS)
sgr_scene_stats_kernel(const SgrChunk* __restrict__ chunks, const SgrStatSegDev* __restrict__ segs,
                       const float* __restrict__ dmeans2D, const int* __restrict__ radii) {
    const SgrChunk c = chunks[blockIdx.x];
    if ((int)threadIdx.x >= c.n) return;
    const sgr_scene_stats_segment& sg = segs[c.seg].s;
    const size_t i = (size_t)c.start + threadIdx.x, o = (size_t)c.out + threadIdx.x;
    const int r = radii[o];
    if (r <= 0) return;  // visibility_filter = radii > 0 (street_gaussian_renderer.py)
    const float gx = dmeans2D[3 * o], gy = dmeans2D[3 * o + 1], gz = dmeans2D[3 * o + 2];
    if (sg.xyz_gradient_accum) {
        // op by op, as the rasterizer's statistics sink forms it (sgr_stat_sink_add<true>, sgr_pergauss.h): the two routes
        // to the statistics give the same bits
        float n2;
        { _Pragma("clang fp contract(off)") n2 = gx * gx + gy * gy; }
        sg.xyz_gradient_accum[2 * i] += sqrtf(n2);                  // street_gaussian_model.py:567
        sg.xyz_gradient_accum[2 * i + 1] += fabsf(gz);              // :568 (norm of one component)
    }
    if (sg.denom) sg.denom[i] += 1.0f;                               // :569
    if (sg.max_radii2D) sg.max_radii2D[i] = fmaxf(sg.max_radii2D[i], (float)r);  // :551-560
}

// ---- host side ----------------------------------------------------------------------------------------------------
template <typename Seg>
static size_t build_chunks(int K, const Seg* segs, std::vector<SgrChunk>& chunks, std::vector<int>& first,
                           std::vector<int>& count) {
    size_t out = 0;
    first.assign(K, 0);
    count.assign(K, 0);
    for (int k = 0; k < K; k++) {
        first[k] = (int)chunks.size();
        for (int s = 0; s < segs[k].count; s += SGR_SC_THREADS)
            chunks.push_back({k, s, std::min(SGR_SC_THREADS, segs[k].count - s), (int32_t)(out + s)});
        count[k] = (int)chunks.size() - first[k];
        out += (size_t)segs[k].count;
    }
    return out;
}

static int check_segments(int K, const sgr_scene_segment* segs, int M, int S) {
    if (K < 0 || (K > 0 && !segs)) return sgr_set_error(SGR_E_INVALID, "segs is required");
    if (M < 1 || S < 0) return sgr_set_error(SGR_E_INVALID, "need M >= 1 and S >= 0");
    for (int k = 0; k < K; k++) {
        const sgr_scene_segment& s = segs[k];
        if (s.count < 0 || s.fourier_dim < 1) return sgr_set_error(SGR_E_INVALID, "segment: count >= 0 and fourier_dim >= 1");
        if (s.count == 0) continue;
        if (!s.xyz || !s.rotation || !s.scaling || !s.opacity || !s.features_dc || (M > 1 && !s.features_rest))
            return sgr_set_error(SGR_E_INVALID, "segment: xyz, rotation, scaling, opacity, features_dc, features_rest are required");
        if (s.kind == SGR_SEG_ACTOR && !s.pose) return sgr_set_error(SGR_E_INVALID, "actor segment without a pose");
        if (s.kind == SGR_SEG_ACTOR && s.fourier_dim > 1 && !s.idft)
            return sgr_set_error(SGR_E_INVALID, "actor segment with fourier_dim > 1 needs idft");
        if (s.kind != SGR_SEG_ACTOR && s.fourier_dim != 1) return sgr_set_error(SGR_E_INVALID, "static segments have fourier_dim 1");
        if (s.flip_axis < 0 || s.flip_axis > 2) return sgr_set_error(SGR_E_INVALID, "flip_axis must be 0, 1 or 2");
    }
    return 0;
}

// Host tables travel through a per-thread, grow-only PINNED staging buffer so that the copy is really asynchronous
// (a pageable source makes hipMemcpyAsync stage or block); an event guards the buffer against reuse while the previous
// call's copy is still in flight.
struct SgrPinnedStage {
    char* p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
};
static int stage_get(size_t bytes, SgrPinnedStage** out) {
    static thread_local SgrPinnedStage stages[64];  // the guarding event belongs to a device: one stage per (thread, device)
    int dev = 0;
    SGR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return sgr_set_error(SGR_E_INVALID, "device index out of range");
    SgrPinnedStage& st = stages[dev];
    if (st.pending) {
        SGR_HIP(hipEventSynchronize(st.ev));
        st.pending = false;
    }
    if (bytes > st.cap) {
        if (st.p) (void)hipHostFree(st.p);
        st.p = nullptr;
        st.cap = 0;
        const size_t want = sgr_align_up(bytes + bytes / 2 + 4096, 4096);
        SGR_HIP(hipHostMalloc((void**)&st.p, want, hipHostMallocPortable));
        st.cap = want;
    }
    if (!st.ev) SGR_HIP(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    *out = &st;
    return 0;
}

// uploads [segments | chunks | zero spans | step table] (+ room for partials) into scratch; returns device pointers
template <typename SegDev>
static int upload(const std::vector<SegDev>& sd, const std::vector<SgrChunk>& chunks, size_t extra_floats,
                  sgr_alloc_fn scratch, void* scratch_user, hipStream_t stream, SegDev** dsegs, SgrChunk** dchunks,
                  float** dextra, const std::vector<SgrZeroDev>* spans = nullptr, SgrZeroDev** dspans = nullptr,
                  const sgr_scene_step* steps = nullptr, const sgr_scene_step** dsteps = nullptr) {
    const size_t b0 = sgr_align_up(sd.size() * sizeof(SegDev), 256), b1 = sgr_align_up(chunks.size() * sizeof(SgrChunk), 256);
    const size_t b2 = spans ? sgr_align_up(spans->size() * sizeof(SgrZeroDev), 256) : 0;
    const size_t b3 = steps ? sgr_align_up(sd.size() * sizeof(sgr_scene_step), 256) : 0;  // parallel to the segments
    char* base = scratch(b0 + b1 + b2 + b3 + extra_floats * sizeof(float) + 512, scratch_user);
    if (!base) return sgr_set_error(SGR_E_ALLOC, "scene scratch allocation failed");
    base = (char*)sgr_align_up((size_t)base, 256);
    SgrPinnedStage* st;
    int rc = stage_get(b0 + b1 + b2 + b3, &st);
    if (rc) return rc;
    memcpy(st->p, sd.data(), sd.size() * sizeof(SegDev));
    memcpy(st->p + b0, chunks.data(), chunks.size() * sizeof(SgrChunk));
    if (spans) memcpy(st->p + b0 + b1, spans->data(), spans->size() * sizeof(SgrZeroDev));
    if (steps) memcpy(st->p + b0 + b1 + b2, steps, sd.size() * sizeof(sgr_scene_step));
    SGR_HIP(hipMemcpyAsync(base, st->p, b0 + b1 + b2 + b3, hipMemcpyHostToDevice, stream));
    SGR_HIP(hipEventRecord(st->ev, stream));
    st->pending = true;
    *dsegs = (SegDev*)base;
    *dchunks = (SgrChunk*)(base + b0);
    if (dspans) *dspans = (SgrZeroDev*)(base + b0 + b1);
    if (dsteps) *dsteps = (const sgr_scene_step*)(base + b0 + b1 + b2);
    if (dextra) *dextra = (float*)(base + b0 + b1 + b2 + b3);
    return 0;
}

// the frame's zero spans as the zero kernel's table (empty spans dropped); returns the number of workgroups
static int zero_table(const sgr_scene_frame* frame, std::vector<SgrZeroDev>& spans, uint32_t* blocks) {
    *blocks = 0;
    if (!frame || frame->n_zero <= 0) return 0;
    if (!frame->zero) return sgr_set_error(SGR_E_INVALID, "frame: n_zero > 0 without a span array");
    size_t total = 0;
    for (int k = 0; k < frame->n_zero; k++) {
        const sgr_zero_span& z = frame->zero[k];
        if (z.count == 0) continue;
        if (!z.ptr) return sgr_set_error(SGR_E_INVALID, "frame: zero span without a pointer");
        spans.push_back({z.ptr, z.count, (uint32_t)total});
        total += (z.count + SGR_SC_ZSPAN - 1) / SGR_SC_ZSPAN;
        if (total > 0x7fffffffu) return sgr_set_error(SGR_E_INVALID, "frame: zero spans too large");
    }
    *blocks = (uint32_t)total;
    return 0;
}

static int compose_forward(int K, const sgr_scene_segment* segs, int M, int S, float* means3D, float* rotations,
                           float* scales, float* opacities, float* shs, float* semantics, const sgr_scene_frame* frame,
                           sgr_alloc_fn scratch, void* scratch_user, hipStream_t stream) {
    int rc = check_segments(K, segs, M, S);
    if (rc) return rc;
    if (!scratch) return sgr_set_error(SGR_E_INVALID, "scratch callback is required");
    std::vector<SgrChunk> chunks;
    std::vector<int> first, count;
    const size_t N = build_chunks(K, segs, chunks, first, count);
    if (N == 0) return 0;
    if (!means3D || !rotations || !scales || !opacities || !shs || (S > 0 && !semantics))
        return sgr_set_error(SGR_E_INVALID, "all output arrays are required");
    std::vector<SgrSegDev> sd(K);
    for (int k = 0; k < K; k++) { sd[k].s = segs[k]; sd[k].g = sgr_scene_segment_grads{}; sd[k].first_chunk = first[k]; sd[k].nchunks = count[k]; sd[k].corr_first = -1; }
    SgrSegDev* dsegs; SgrChunk* dchunks;
    if ((rc = upload(sd, chunks, 0, scratch, scratch_user, stream, &dsegs, &dchunks, nullptr))) return rc;
    const unsigned nb = (unsigned)chunks.size();
    const float* corr = frame ? frame->correction : nullptr;
    sgr_scene_fwd_kernel<<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, S, means3D, rotations, scales, opacities, semantics, corr);
    if (M == 16) sgr_scene_sh_fwd_kernel<16><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, M, S, shs, semantics);
    else sgr_scene_sh_fwd_kernel<0><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, M, S, shs, semantics);
    SGR_HIP(hipGetLastError());
    return 0;
}

// what sgr_scene_compose_backward_step refuses on top of the plain backward (include/sgr_scene_step.h)
static int check_steps(int K, const sgr_scene_segment* segs, const sgr_scene_step* steps, const sgr_scene_segment_grads* grads,
                       double beta1, double beta2) {
    if (K > 0 && !steps) return sgr_set_error(SGR_E_INVALID, "steps is required");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return sgr_set_error(SGR_E_INVALID, "betas must lie in [0, 1)");
    for (int k = 0; k < K; k++) {
        if (grads) {
            const sgr_scene_segment_grads& g = grads[k];
            if (g.xyz || g.rotation || g.scaling || g.opacity || g.features_dc || g.features_rest || g.semantic)
                return sgr_set_error(SGR_E_INVALID, "step sink: grads may carry only .pose (a group is stepped, not written)");
        }
        if (segs[k].count == 0) continue;
        const sgr_scene_segment& s = segs[k];
        const float* param[SGR_SCENE_STEP_GROUPS] = {s.xyz, s.features_dc, s.features_rest, s.opacity, s.scaling, s.rotation, s.semantic};
        for (int g = 0; g < SGR_SCENE_STEP_GROUPS; g++) {
            const sgr_scene_step_group& sg = steps[k].group[g];
            if (sg.m && (!sg.v || !param[g]))
                return sgr_set_error(SGR_E_INVALID, "step sink: a stepped group needs exp_avg_sq and its parameter pointer");
        }
    }
    return 0;
}

// steps == NULL: the plain backward (gradients into `grads`); else the step sink, `grads` NULL or .pose only
static int compose_backward(int K, const sgr_scene_segment* segs, const sgr_scene_segment_grads* grads, int M, int S,
                            const float* dL_dmeans3D, const float* dL_drotations, const float* dL_dscales,
                            const float* dL_dopacities, const float* dL_dshs, const float* dL_dsemantics,
                            const sgr_scene_frame* frame, sgr_alloc_fn scratch, void* scratch_user, hipStream_t stream,
                            const sgr_scene_step* steps = nullptr, double beta1 = 0.0, double beta2 = 0.0, float eps = 0.f) {
    int rc = check_segments(K, segs, M, S);
    if (rc) return rc;
    if ((!grads && !steps) || !scratch) return sgr_set_error(SGR_E_INVALID, "grads and scratch are required");
    if (steps && (rc = check_steps(K, segs, steps, grads, beta1, beta2))) return rc;
    std::vector<SgrZeroDev> spans;
    uint32_t zblocks = 0;
    if ((rc = zero_table(frame, spans, &zblocks))) return rc;
    const float* corr = frame ? frame->correction : nullptr;
    float* corr_grad = corr ? frame->correction_grad : nullptr;
    std::vector<SgrChunk> chunks;
    std::vector<int> first, count;
    const size_t N = build_chunks(K, segs, chunks, first, count);
    if (N == 0 && zblocks == 0 && !corr_grad) return 0;
    std::vector<SgrSegDev> sd(K);
    int nc = 0;  // corrected chunks
    for (int k = 0; k < K; k++) {
        sd[k].s = segs[k]; sd[k].g = grads ? grads[k] : sgr_scene_segment_grads{}; sd[k].first_chunk = first[k]; sd[k].nchunks = count[k]; sd[k].corr_first = -1;
        if (corr && segs[k].kind == SGR_SEG_STATIC) { sd[k].corr_first = nc; nc += count[k]; }
    }
    const int ng = (nc + SGR_SC_THREADS - 1) / SGR_SC_THREADS;  // groups of 256 corrected chunks
    const size_t np = chunks.size() * SGR_SC_NPART, ncp = corr_grad ? (size_t)nc * SGR_SC_NPART : 0;
    const size_t ngp = corr_grad ? (size_t)ng * SGR_SC_NPART : 0;
    SgrSegDev* dsegs; SgrChunk* dchunks; float* partials; SgrZeroDev* dspans;
    SgrStepArgs sa{nullptr, AdamConsts{0.f, 0.f, 0.f}, eps};
    if (steps) sa.k = adam_consts(beta1, beta2);
    if ((rc = upload(sd, chunks, np + ncp + ngp, scratch, scratch_user, stream, &dsegs, &dchunks, &partials, &spans, &dspans,
                     steps, &sa.steps)))
        return rc;
    float* cpart = corr_grad ? partials + np : nullptr;
    float* gpart = corr_grad ? partials + np + ncp : nullptr;
    if (zblocks) sgr_scene_zero_kernel<<<zblocks, SGR_SC_THREADS, 0, stream>>>(dspans, (int)spans.size());
    const unsigned nb = (unsigned)chunks.size();
    if (nb && !steps) {
        sgr_scene_bwd_kernel<0><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, S, dL_dmeans3D, dL_drotations, dL_dscales,
                                                                   dL_dopacities, dL_dsemantics, partials, corr, cpart, sa);
        sgr_scene_pose_bwd_kernel<<<(unsigned)K, 64, 0, stream>>>(dsegs, partials);
        if (M == 16) sgr_scene_sh_bwd_kernel<16, 0><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, M, S, dL_dshs, dL_dsemantics, sa);
        else sgr_scene_sh_bwd_kernel<0, 0><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, M, S, dL_dshs, dL_dsemantics, sa);
    } else if (nb) {  // the step sink: the same launches, the other flavour
        sgr_scene_bwd_kernel<1><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, S, dL_dmeans3D, dL_drotations, dL_dscales,
                                                                   dL_dopacities, dL_dsemantics, partials, corr, cpart, sa);
        sgr_scene_pose_bwd_kernel<<<(unsigned)K, 64, 0, stream>>>(dsegs, partials);
        if (M == 16) sgr_scene_sh_bwd_kernel<16, 1><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, M, S, dL_dshs, dL_dsemantics, sa);
        else sgr_scene_sh_bwd_kernel<0, 1><<<nb, SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, M, S, dL_dshs, dL_dsemantics, sa);
    }
    if (corr_grad) {
        if (ng) sgr_scene_corr_sum_kernel<<<(unsigned)ng, SGR_SC_THREADS, 0, stream>>>(cpart, nc, gpart);
        sgr_scene_corr_final_kernel<<<1, SGR_SC_THREADS, 0, stream>>>(gpart, ng, corr, corr_grad);
    }
    SGR_HIP(hipGetLastError());
    return 0;
}

extern "C" {

int sgr_scene_compose_forward(int K, const sgr_scene_segment* segs, int M, int S, float* means3D, float* rotations,
                              float* scales, float* opacities, float* shs, float* semantics, sgr_alloc_fn scratch,
                              void* scratch_user, void* stream_) {
    return compose_forward(K, segs, M, S, means3D, rotations, scales, opacities, shs, semantics, nullptr, scratch,
                           scratch_user, (hipStream_t)stream_);
}

int sgr_scene_compose_forward_ex(int K, const sgr_scene_segment* segs, int M, int S, float* means3D, float* rotations,
                                 float* scales, float* opacities, float* shs, float* semantics,
                                 const sgr_scene_frame* frame, sgr_alloc_fn scratch, void* scratch_user, void* stream_) {
    return compose_forward(K, segs, M, S, means3D, rotations, scales, opacities, shs, semantics, frame, scratch,
                           scratch_user, (hipStream_t)stream_);
}

int sgr_scene_compose_backward(int K, const sgr_scene_segment* segs, const sgr_scene_segment_grads* grads, int M, int S,
                               const float* dL_dmeans3D, const float* dL_drotations, const float* dL_dscales,
                               const float* dL_dopacities, const float* dL_dshs, const float* dL_dsemantics,
                               sgr_alloc_fn scratch, void* scratch_user, void* stream_) {
    return compose_backward(K, segs, grads, M, S, dL_dmeans3D, dL_drotations, dL_dscales, dL_dopacities, dL_dshs,
                            dL_dsemantics, nullptr, scratch, scratch_user, (hipStream_t)stream_);
}

int sgr_scene_compose_backward_ex(int K, const sgr_scene_segment* segs, const sgr_scene_segment_grads* grads, int M,
                                  int S, const float* dL_dmeans3D, const float* dL_drotations, const float* dL_dscales,
                                  const float* dL_dopacities, const float* dL_dshs, const float* dL_dsemantics,
                                  const sgr_scene_frame* frame, sgr_alloc_fn scratch, void* scratch_user, void* stream_) {
    return compose_backward(K, segs, grads, M, S, dL_dmeans3D, dL_drotations, dL_dscales, dL_dopacities, dL_dshs,
                            dL_dsemantics, frame, scratch, scratch_user, (hipStream_t)stream_);
}

int sgr_scene_compose_backward_step(int K, const sgr_scene_segment* segs, const sgr_scene_step* steps,
                                    const sgr_scene_segment_grads* grads, int M, int S, const float* dL_dmeans3D,
                                    const float* dL_drotations, const float* dL_dscales, const float* dL_dopacities,
                                    const float* dL_dshs, const float* dL_dsemantics, const sgr_scene_frame* frame,
                                    double beta1, double beta2, float eps, sgr_alloc_fn scratch, void* scratch_user,
                                    void* stream_) {
    if (K < 0 || (K > 0 && !steps)) return sgr_set_error(SGR_E_INVALID, "steps is required");
    static const sgr_scene_step none{};  // K == 0: a frame without a segment still writes its zero spans
    return compose_backward(K, segs, grads, M, S, dL_dmeans3D, dL_drotations, dL_dscales, dL_dopacities, dL_dshs,
                            dL_dsemantics, frame, scratch, scratch_user, (hipStream_t)stream_, steps ? steps : &none, beta1,
                            beta2, eps);
}

int sgr_scene_densification_stats(int K, const sgr_scene_stats_segment* segs, const float* dL_dmeans2D, const int* radii,
                                  sgr_alloc_fn scratch, void* scratch_user, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (K < 0 || (K > 0 && !segs) || !scratch) return sgr_set_error(SGR_E_INVALID, "segs and scratch are required");
    for (int k = 0; k < K; k++)
        if (segs[k].count < 0) return sgr_set_error(SGR_E_INVALID, "segment count must be >= 0");
    std::vector<SgrChunk> chunks;
    std::vector<int> first, count;
    const size_t N = build_chunks(K, segs, chunks, first, count);
    if (N == 0) return 0;
    if (!dL_dmeans2D || !radii) return sgr_set_error(SGR_E_INVALID, "dL_dmeans2D and radii are required");
    std::vector<SgrStatSegDev> sd(K);
    for (int k = 0; k < K; k++) sd[k].s = segs[k];
    SgrStatSegDev* dsegs; SgrChunk* dchunks;
    int rc = upload(sd, chunks, 0, scratch, scratch_user, stream, &dsegs, &dchunks, nullptr);
    if (rc) return rc;
    sgr_scene_stats_kernel<<<(unsigned)chunks.size(), SGR_SC_THREADS, 0, stream>>>(dchunks, dsegs, dL_dmeans2D, radii);
    SGR_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
