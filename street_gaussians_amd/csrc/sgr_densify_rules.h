// sgr_densify_rules.h -- what sgr_densify.hip (one model per call) and sgr_densify_scene.hip (a whole FlatScene per call)
// share: the work-area layout, the flag bits and the per-row DECISIONS (what happens to a point, where its rows go, which
// candidates are pruned).  Each is one __device__ function that
// both files' kernels call, built with the same flags (build.py gives neither file flags of its own), so the per-model
// path and the scene path cannot drift apart: the scene path's contract is bit-identity with the per-model loop.
#pragma once
#include <cstdint>

#include "../../include/sgr_densify.h"
#include "sgr_common.h"
#include "sgr_quat.h"

struct DnWork {
    uint32_t *flags, *offA, *offB, *offS, *offC, *tmp, *totals;  // totals: nA nB nS nC nClone nPrunedCand
};
static inline DnWork dn_carve(char* base, size_t N, char** end = nullptr) {
    DnWork w;
    char* p = base;
    const size_t n = N ? N : 1;
    sgr_carve(p, w.flags, n);
    sgr_carve(p, w.offA, n);
    sgr_carve(p, w.offB, n);
    sgr_carve(p, w.offS, n);
    sgr_carve(p, w.offC, n);
    sgr_carve(p, w.tmp, sgr_scan_tmp_count(n));
    sgr_carve(p, w.totals, 16);
    if (end) *end = p;
    return w;
}

#define DN_CLONE 1u
#define DN_SPLIT 2u
#define DN_PRUNE_SELF 4u
#define DN_PRUNE_CHILD 8u

#define SGR_DN_ROWS 128  // result rows one workgroup of a gather builds

struct DnSphere { float cx, cy, cz, r; };
struct DnBox { float lo[3], hi[3]; };

#ifdef __HIPCC__
// clone / split / prune-self / prune-child of original point i (gaussian_model.py:522-543), as DN_* bits
__device__ __forceinline__ uint32_t dn_decide_flags(const sgr_densify_params& p, const float* __restrict__ accum,
                                                    const float* __restrict__ denom, const float* __restrict__ scaling,
                                                    const float* __restrict__ opacity, size_t i) {
    float g = accum[2 * i + p.grad_column] / denom[i];  // :523
    if (g != g) g = 0.0f;                                // grads[grads.isnan()] = 0.0 (:524)
    const float s0 = expf(scaling[3 * i]), s1 = expf(scaling[3 * i + 1]), s2 = expf(scaling[3 * i + 2]);
    const float smax = fmaxf(s0, fmaxf(s1, s2));
    const float dense = p.percent_dense * p.extent;
    const bool clone = (fabsf(g) >= p.max_grad) && (smax <= dense);  // :497-499 (norm of a 1-vector)
    const bool split = (g >= p.max_grad) && (smax > dense);          // :462-464
    const float op = sigmoidf_(opacity[i]);
    const bool low = op < p.min_opacity;                              // :533
    const float big = p.extent * p.percent_big_ws;
    const bool prune_self = !p.defer_prune && (low || (p.prune_big && smax > big));  // :536-540
    // children: log(scale / (0.8 N)) -> exp gives scale / (0.8 N) again (up to rounding, like the reference's log/exp)
    const float child = expf(logf(smax / (0.8f * (float)p.n_split)));
    const bool prune_child = !p.defer_prune && (low || (p.prune_big && child > big));
    return (clone ? DN_CLONE : 0u) | (split ? DN_SPLIT : 0u) | (prune_self ? DN_PRUNE_SELF : 0u) |
           (prune_child ? DN_PRUNE_CHILD : 0u);
}
// the four masks the scans rank (sgr_densify.hip, head comment)
__device__ __forceinline__ void dn_store_masks(const DnWork& w, size_t i, uint32_t f) {
    const bool split = f & DN_SPLIT;
    w.flags[i] = f;
    w.offA[i] = (!split && !(f & DN_PRUNE_SELF)) ? 1u : 0u;
    w.offB[i] = ((f & DN_CLONE) && !(f & DN_PRUNE_SELF)) ? 1u : 0u;
    w.offS[i] = split ? 1u : 0u;
    w.offC[i] = (split && !(f & DN_PRUNE_CHILD)) ? 1u : 0u;
}

// Where original point i's rows go in a result block that starts at row `base`: kept originals (nA of them, this one at
// rank rA), then clones (nB, rank rB), then split children copy-major (nC parents with surviving children, rank rC; :468-476).
// src = i, kind = SGR_KIND_*, sample_row = sample_base + copy * nS + rS for children (rS = rank among the nS split points,
// the reference's repeat(N, 1) order), else -1.
__device__ __forceinline__ void dn_map_row(uint32_t f, int32_t i, uint32_t base, uint32_t nA, uint32_t nB, uint32_t nS,
                                           uint32_t nC, uint32_t rA, uint32_t rB, uint32_t rS, uint32_t rC, int n_split,
                                           uint32_t sample_base, int32_t* __restrict__ src, uint8_t* __restrict__ kind,
                                           int32_t* __restrict__ sample_row) {
    const bool split = f & DN_SPLIT;
    if (!split && !(f & DN_PRUNE_SELF)) {
        const uint32_t o = base + rA;
        src[o] = i; kind[o] = SGR_KIND_KEEP; sample_row[o] = -1;
    }
    if ((f & DN_CLONE) && !(f & DN_PRUNE_SELF)) {
        const uint32_t o = base + nA + rB;
        src[o] = i; kind[o] = SGR_KIND_CLONE; sample_row[o] = -1;
    }
    if (split && !(f & DN_PRUNE_CHILD)) {
        for (int n = 0; n < n_split; n++) {  // repeat(N, 1): copy-major
            const uint32_t o = base + nA + nB + (uint32_t)n * nC + rC;
            src[o] = i; kind[o] = SGR_KIND_SPLIT_CHILD; sample_row[o] = (int32_t)(sample_base + (uint32_t)n * nS + rS);
        }
    }
}

#define DN_LOW 1u
#define DN_BIG 2u
#define DN_OUTSIDE 4u
// low opacity / big in world space (after the background's exemption) / outside the tracking box of candidate row i, as
// DN_LOW | DN_BIG | DN_OUTSIDE (include/sgr_densify.h: the three prune variants); zn = the candidate's two box samples
// ([2,3] standard normals), read by the actor rule with prune_big only
__device__ __forceinline__ uint32_t dn_decide_prune(const sgr_densify_params& p, int variant, const float* __restrict__ xyz,
                                                    const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                    const float* __restrict__ opacity, const DnSphere& sph, const DnBox& box,
                                                    const float* __restrict__ zn, size_t i) {
#pragma clang fp contract(off)
    bool big = false, outside = false;
    const float op = sigmoidf_(opacity[i]);
    const bool low = op < p.min_opacity;
    const float s[3] = {expf(scaling[3 * i]), expf(scaling[3 * i + 1]), expf(scaling[3 * i + 2])};
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (p.prune_big) {
        big = fmaxf(s[0], fmaxf(s[1], s[2])) > p.extent * p.percent_big_ws;
        if (variant == SGR_PRUNE_BKGD) {  // gaussian_model_bkgd.py:95-97
            const float dx = x - sph.cx, dy = y - sph.cy, dz = z - sph.cz;
            const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
            if (dist > 2.0f * sph.r) big = false;
        }
        if (variant == SGR_PRUNE_ACTOR) {  // gaussian_model_actor.py:231-249
            float R[9], nrm;
            Q4 qn;
            qtomat<true>(qload(rotation + 4 * i), R, qn, nrm);
            const float c[3] = {x, y, z};
            bool inside = true;
            for (int m = 0; m < 2; m++) {
                const float v[3] = {zn[3 * m] * s[0], zn[3 * m + 1] * s[1], zn[3 * m + 2] * s[2]};
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const float w = rot_row<true>(R + 3 * a, v, c[a]);
                    inside = inside && (w >= box.lo[a]) && (w <= box.hi[a]);
                }
            }
            outside = !inside;
        }
    }
    return (low ? DN_LOW : 0u) | (big ? DN_BIG : 0u) | (outside ? DN_OUTSIDE : 0u);
}
#endif
