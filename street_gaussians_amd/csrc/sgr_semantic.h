// sgr_semantic.h -- the per-pixel arithmetic of the semantic cross-entropy (include/sgr_semantic_loss.h), one text for the
// gfx950 kernels of sgr_semantic_loss.hip and for the host build of tests/host_math/semantic_host.hip.  __host__ __device__;
// a pixel's S channel values live in a register array of NC >= S floats that every loop walks fully unrolled (no dynamic
// index into it: the label's channel is picked with a select, so the array never goes to scratch).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SGR_SEM_HD __host__ __device__ __forceinline__
#define SGR_SEM_EPS 1e-8f  // street_gaussian_renderer.py:261-262, in float32
#define SGR_SEM_MODE_LOGITS 0         // == SGR_SEM_LOGITS
#define SGR_SEM_MODE_PROBABILITIES 1  // == SGR_SEM_PROBABILITIES
// the kernels use the hardware exponential and logarithm (v_exp_f32 / v_log_f32), the host build the C library's
#if defined(__HIP_DEVICE_COMPILE__)
#define SGR_SEM_EXP(x) __expf(x)
#define SGR_SEM_LOG(x) __logf(x)
#else
#define SGR_SEM_EXP(x) expf(x)
#define SGR_SEM_LOG(x) logf(x)
#endif

enum { SGR_SEM_PIX_IGNORED = 0, SGR_SEM_PIX_VALID = 1, SGR_SEM_PIX_OUT_OF_RANGE = 2 };

// label p of a map of dtype SGR_SEM_LABEL_U8 (0) / I32 (1) / I64 (2); the 64-bit label is read as two 32-bit words, so a
// map that is only 4-byte aligned is fine
SGR_SEM_HD int64_t sem_label(const void* labels, int dtype, size_t p) {
    if (dtype == 0) return ((const uint8_t*)labels)[p];
    if (dtype == 1) return ((const int32_t*)labels)[p];
    const uint32_t* w = (const uint32_t*)labels + 2 * p;
    return (int64_t)(((uint64_t)w[1] << 32) | w[0]);
}
// valid: in [0, S) and not ignore_index; out of range: >= S and not ignore_index (counted, no gradient); else ignored
SGR_SEM_HD int sem_classify(int64_t l, int S, int ignore_index) {
    if (l < 0 || l == (int64_t)ignore_index) return SGR_SEM_PIX_IGNORED;
    return l < S ? SGR_SEM_PIX_VALID : SGR_SEM_PIX_OUT_OF_RANGE;
}

// channel values of pixel p of the planar [S][plane] image, consecutive lanes on consecutive pixels of a plane
template <int NC>
SGR_SEM_HD void sem_load(float (&x)[NC], const float* __restrict__ sem, size_t plane, size_t p, int S) {
#pragma unroll
    for (int c = 0; c < NC; c++) x[c] = c < S ? sem[c * plane + p] : 0.f;
}

// best <- the first channel holding the maximum (np.argmax's tie rule); loss <- loss_p for label l (anything when l is
// not in [0, S): the caller drops it).
//   logits:         m = max_c x_c,  loss_p = (m - x_l) + log(sum_c exp(x_c - m))       [= lse - x_l, without forming lse:
//                   the sum is exact 0 + log(sum) where the label is the arg-max, and exactly 0 for S = 1]
//   probabilities:  s = sum_c r_c (c ascending),  q_l = r_l / (s + eps),  loss_p = -log(q_l + eps)
template <int NC>
SGR_SEM_HD void sem_forward_point(const float (&x)[NC], int S, int mode, int l, float& loss, int& best) {
    float m = x[0], xl = x[0];
    best = 0;
#pragma unroll
    for (int c = 1; c < NC; c++) {
        if (c < S) {
            if (x[c] > m) {
                m = x[c];
                best = c;
            }
            if (c == l) xl = x[c];
        }
    }
    float s = 0.f;
    if (mode == SGR_SEM_MODE_LOGITS) {
#pragma unroll
        for (int c = 0; c < NC; c++)
            if (c < S) s += SGR_SEM_EXP(x[c] - m);
        loss = (m - xl) + SGR_SEM_LOG(s);
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++)
            if (c < S) s += x[c];
        loss = -SGR_SEM_LOG(xl / (s + SGR_SEM_EPS) + SGR_SEM_EPS);
    }
}

// x[c] <- scale * d loss_p / d x_c of a VALID pixel with label l, in place.
//   logits:         exp(x_c - m) / sum_k exp(x_k - m) - [c == l]      [= exp(x_c - lse) - [c == l]; m and the sum are
//                   recomputed from the registers: lse rounded to float32 would cost ulp(lse) / 2 of every probability]
//   probabilities:  -([c == l] / (s + eps) - r_l / (s + eps)^2) / (q_l + eps)
template <int NC>
SGR_SEM_HD void sem_backward_point(float (&x)[NC], int S, int mode, int l, float scale) {
    float m = x[0], xl = x[0];
#pragma unroll
    for (int c = 1; c < NC; c++) {
        if (c < S) {
            m = x[c] > m ? x[c] : m;
            if (c == l) xl = x[c];
        }
    }
    float s = 0.f;
    if (mode == SGR_SEM_MODE_LOGITS) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < S) {
                x[c] = SGR_SEM_EXP(x[c] - m);
                s += x[c];
            }
        }
        const float inv = 1.0f / s;
#pragma unroll
        for (int c = 0; c < NC; c++)
            if (c < S) x[c] = (x[c] * inv - (c == l ? 1.0f : 0.f)) * scale;
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++)
            if (c < S) s += x[c];
        const float d = s + SGR_SEM_EPS, q = xl / d;
        const float w = scale / (q + SGR_SEM_EPS), a = 1.0f / d, b = xl / (d * d);
#pragma unroll
        for (int c = 0; c < NC; c++)
            if (c < S) x[c] = -((c == l ? a : 0.f) - b) * w;
    }
}
