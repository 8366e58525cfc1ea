// sgr_optim.hip -- the fused per-segment Adam step (include/sgr_optim.h) on gfx950.
//
// A pure stream: per element it reads p, g, m, v and writes p, m, v (28 bytes), so the kernel is built to keep HBM
// busy and nothing else.  One launch per step over a list of records (one per chunk stepped now):
//   - the grid is capped at a few workgroups per CU (256 CUs) and walks the spans grid-stride; a span is
//     SGR_ADAM_SPAN consecutive elements of one chunk, 4 float4 per lane of a 256-lane workgroup;
//   - each workgroup copies the records' span_start column into LDS once and finds the record of a span by a binary
//     search there (all lanes read the same word: a broadcast);
//   - inside a span the body moves as float4 when p, g, m and v share their alignment modulo 16 bytes (chunks start at
//     any 4-byte offset: an odd count x width 3 gives unaligned blocks), the at most 3 elements before the first aligned
//     one and after the last one go element by element; otherwise the whole span goes element by element.
// The arithmetic is the header's contract, with contraction off for this file (pragma below, and -ffp-contract=off in
// build.py's PER_FILE_FLAGS); hipcc's defaults give correctly rounded f32 division and square root and keep denormals.
#include <string>

#include "../../include/sgr_optim.h"
#include "sgr_adam_math.h"  // AdamConsts, adam1: the per-element arithmetic
#include "sgr_common.h"

#pragma clang fp contract(off)

static constexpr int SGR_ADAM_THREADS = 256;
static constexpr int SGR_ADAM_VEC = 4;                                       // float4 per lane per span
static constexpr int64_t SGR_ADAM_SPAN = SGR_ADAM_THREADS * SGR_ADAM_VEC * 4; // 4096 elements
static constexpr int SGR_ADAM_MAX_RECORDS = 4096;                            // LDS: 16 KiB of span starts
static constexpr int SGR_ADAM_BLOCKS_PER_CU = 4;
static constexpr int SGR_ADAM_CUS = 256;

static_assert(sizeof(sgr_adam_chunk) == 32 && sizeof(sgr_adam_record) == 32, "table layout of include/sgr_optim.h");

__global__ void __launch_bounds__(SGR_ADAM_THREADS)
sgr_adam_step_kernel(const sgr_adam_chunk* __restrict__ chunks, const sgr_adam_record* __restrict__ records,
                     int n_chunks, int n_records, int64_t n_spans, AdamConsts k) {
    extern __shared__ int32_t s_start[];
    for (int i = threadIdx.x; i < n_records; i += SGR_ADAM_THREADS) s_start[i] = records[i].span_start;
    __syncthreads();
    const int t = threadIdx.x;
    for (int64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
        // record r = the last one with span_start <= span
        int lo = 0, hi = n_records - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((int64_t)s_start[mid] <= span) lo = mid;
            else hi = mid - 1;
        }
        const sgr_adam_record rec = records[lo];
        if (rec.chunk < 0 || rec.chunk >= n_chunks) continue;
        const sgr_adam_chunk ch = chunks[rec.chunk];
        const int64_t e0 = (span - rec.span_start) * SGR_ADAM_SPAN;
        if (e0 < 0 || e0 >= ch.count) continue;
        const int64_t e1 = min(e0 + SGR_ADAM_SPAN, ch.count);
        float* __restrict__ p = ch.p;
        float* __restrict__ m = ch.m;
        float* __restrict__ v = ch.v;
        const float* __restrict__ g = rec.g;
        const float ss = rec.step_size, bc2s = rec.bc2_sqrt, eps = rec.eps;
        const uintptr_t ap = (uintptr_t)p;
        const bool vec = (((ap ^ (uintptr_t)g) | (ap ^ (uintptr_t)m) | (ap ^ (uintptr_t)v)) & 15) == 0;
        if (vec) {
            // first element whose address is 16-byte aligned: e0 is a multiple of 4, so it is e0 + h
            const int64_t h = (int64_t)(((16 - (ap & 15)) & 15) >> 2);
            const int64_t a0 = min(e0 + h, e1);
            const int nv = (int)((e1 - a0) >> 2);
            const int64_t a1 = a0 + 4 * (int64_t)nv;
            if (t < a0 - e0) {
                const int64_t i = e0 + t;
                float pp = p[i], mm = m[i], vv = v[i];
                adam1(pp, g[i], mm, vv, k, ss, bc2s, eps);
                p[i] = pp; m[i] = mm; v[i] = vv;
            }
            if (t < e1 - a1) {
                const int64_t i = a1 + t;
                float pp = p[i], mm = m[i], vv = v[i];
                adam1(pp, g[i], mm, vv, k, ss, bc2s, eps);
                p[i] = pp; m[i] = mm; v[i] = vv;
            }
            float4* __restrict__ p4 = reinterpret_cast<float4*>(p + a0);
            float4* __restrict__ m4 = reinterpret_cast<float4*>(m + a0);
            float4* __restrict__ v4 = reinterpret_cast<float4*>(v + a0);
            const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + a0);
            float4 P[SGR_ADAM_VEC], G[SGR_ADAM_VEC], M[SGR_ADAM_VEC], V[SGR_ADAM_VEC];
#pragma unroll
            for (int j = 0; j < SGR_ADAM_VEC; ++j) {
                const int q = t + j * SGR_ADAM_THREADS;
                if (q < nv) {
                    P[j] = p4[q]; G[j] = g4[q]; M[j] = m4[q]; V[j] = v4[q];
                }
            }
#pragma unroll
            for (int j = 0; j < SGR_ADAM_VEC; ++j) {
                const int q = t + j * SGR_ADAM_THREADS;
                if (q < nv) {
                    adam1(P[j].x, G[j].x, M[j].x, V[j].x, k, ss, bc2s, eps);
                    adam1(P[j].y, G[j].y, M[j].y, V[j].y, k, ss, bc2s, eps);
                    adam1(P[j].z, G[j].z, M[j].z, V[j].z, k, ss, bc2s, eps);
                    adam1(P[j].w, G[j].w, M[j].w, V[j].w, k, ss, bc2s, eps);
                    p4[q] = P[j]; m4[q] = M[j]; v4[q] = V[j];
                }
            }
        } else {
            for (int64_t i = e0 + t; i < e1; i += SGR_ADAM_THREADS) {
                float pp = p[i], mm = m[i], vv = v[i];
                adam1(pp, g[i], mm, vv, k, ss, bc2s, eps);
                p[i] = pp; m[i] = mm; v[i] = vv;
            }
        }
    }
}

int sgr_adam_span_elems(void) { return (int)SGR_ADAM_SPAN; }
int sgr_adam_max_blocks(void) { return SGR_ADAM_CUS * SGR_ADAM_BLOCKS_PER_CU; }
int sgr_adam_max_records(void) { return SGR_ADAM_MAX_RECORDS; }

int sgr_adam_step(const sgr_adam_chunk* chunks, int n_chunks, const sgr_adam_record* records, int n_records,
                  int64_t n_spans, double beta1, double beta2, void* stream_) {
    if (n_chunks < 0 || n_records < 0 || n_spans < 0)
        return sgr_set_error(SGR_E_INVALID, "adam: negative table size");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return sgr_set_error(SGR_E_INVALID, "adam: betas must lie in [0, 1)");
    if (n_records > SGR_ADAM_MAX_RECORDS)
        return sgr_set_error(SGR_E_INVALID, "adam: more than " + std::to_string(SGR_ADAM_MAX_RECORDS) + " records in one step");
    if (n_spans == 0) return 0;
    if (!chunks || !records || n_chunks == 0 || n_records == 0)
        return sgr_set_error(SGR_E_INVALID, "adam: n_spans > 0 needs the chunk and record tables");
    if (n_spans > (int64_t)INT32_MAX) return sgr_set_error(SGR_E_INVALID, "adam: more than 2^31 - 1 spans");
    const AdamConsts k = adam_consts(beta1, beta2);
    const int64_t cap = sgr_adam_max_blocks();
    const unsigned grid = (unsigned)(n_spans < cap ? n_spans : cap);
    sgr_adam_step_kernel<<<grid, SGR_ADAM_THREADS, (size_t)n_records * sizeof(int32_t), (hipStream_t)stream_>>>(
        chunks, records, n_chunks, n_records, n_spans, k);
    SGR_HIP(hipGetLastError());
    return 0;
}
