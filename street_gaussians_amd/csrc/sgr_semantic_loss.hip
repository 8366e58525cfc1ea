// sgr_semantic_loss.hip -- cross-entropy on the rendered semantic head in one op (include/sgr_semantic_loss.h) on gfx950.
//
// Forward: ONE map kernel, a lane per pixel (consecutive lanes on consecutive pixels of every channel plane: a wave's load
// is 256 contiguous bytes).  A pixel's S values are loaded into registers back to back -- S independent loads in flight per
// lane -- and the arithmetic of sgr_semantic.h runs on them: each element of `semantic` is read once.  Four block partials
// (loss sum; valid, out-of-range and correct counts, the counts as integers from wave ballots) go to the workspace in block
// order; one finishing workgroup adds them in a fixed order and evaluates the four scalars.
// Backward: ONE kernel of the same shape reads a valid pixel's values once and writes its S gradient elements once; every
// other pixel gets S zeros without a load.
// No access is wider than 4 bytes, so nothing here depends on the alignment or the parity of H * W.
#include "../../include/sgr_semantic_loss.h"
#include "sgr_common.h"
#include "sgr_reduce.h"
#include "sgr_semantic.h"

#define SGR_SEM_BLOCK 256         // pixels per block of the map kernel (sgr_semantic_loss_block_pixels)
#define SGR_SEM_FINISH_SPAN 1024  // block partials per quantity one trip of the finishing loop covers
#define SGR_SEM_SUMS 4            // block partials per block: loss sum (float), valid, out of range, correct (uint32 bits)

template <int NC>
__global__ void __launch_bounds__(SGR_SEM_BLOCK)
sgr_semantic_loss_map_kernel(int S, size_t plane, const float* __restrict__ sem, const void* __restrict__ labels, int dtype,
                             int ignore_index, int mode, uint8_t* __restrict__ pred, float* __restrict__ block_sums) {
    __shared__ float lsum[4];
    __shared__ uint32_t lcnt[3][4];
    const size_t p = (size_t)blockIdx.x * SGR_SEM_BLOCK + threadIdx.x;
    int cls = SGR_SEM_PIX_IGNORED, best = 0, l = -1;
    float loss = 0.f;
    if (p < plane) {
        const int64_t lab = sem_label(labels, dtype, p);
        cls = sem_classify(lab, S, ignore_index);
        if (cls == SGR_SEM_PIX_VALID) l = (int)lab;
        if (cls == SGR_SEM_PIX_VALID || pred) {
            float x[NC];
            sem_load<NC>(x, sem, plane, p, S);
            sem_forward_point<NC>(x, S, mode, l, loss, best);
            if (pred) pred[p] = (uint8_t)best;
        }
    }
    const bool valid = cls == SGR_SEM_PIX_VALID;
    // (every lane of the block is here: the DPP sum and the ballots see full waves)
    const float wsum = sgr_wave_sum_dpp(valid ? loss : 0.f);  // valid in lane 63
    const uint32_t nv = __popcll(__ballot(valid)), no = __popcll(__ballot(cls == SGR_SEM_PIX_OUT_OF_RANGE)),
                   nc = __popcll(__ballot(valid && best == l));
    if ((threadIdx.x & 63) == 63) {
        const int w = threadIdx.x >> 6;
        lsum[w] = wsum;
        lcnt[0][w] = nv;
        lcnt[1][w] = no;
        lcnt[2][w] = nc;
    }
    __syncthreads();
    if (threadIdx.x < SGR_SEM_SUMS) {
        const int q = threadIdx.x;
        float out;
        if (q == 0) out = ((lsum[0] + lsum[1]) + lsum[2]) + lsum[3];
        else out = __uint_as_float(((lcnt[q - 1][0] + lcnt[q - 1][1]) + lcnt[q - 1][2]) + lcnt[q - 1][3]);
        block_sums[(size_t)q * gridDim.x + blockIdx.x] = out;
    }
}

// one workgroup: row 0 of block_sums summed as floats, rows 1..3 as integers, lanes striding over the blocks in a fixed
// order.  A trip covers SGR_SEM_FINISH_SPAN blocks of all four rows with unconditional loads (index clamped, value dropped
// past the end): 16 loads in flight per lane, the single workgroup is latency-bound.
__global__ void __launch_bounds__(256)
sgr_semantic_loss_finish_kernel(const float* __restrict__ block_sums, size_t nblocks, float* __restrict__ terms) {
    __shared__ float lsum[4];
    __shared__ uint32_t lcnt[3][4];
    float a = 0.f;
    uint32_t n[3] = {0u, 0u, 0u};
    for (size_t i0 = threadIdx.x; i0 < nblocks; i0 += SGR_SEM_FINISH_SPAN) {
        float v[4][SGR_SEM_SUMS];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t i = i0 + 256 * u, ic = i < nblocks ? i : nblocks - 1;
#pragma unroll
            for (int q = 0; q < SGR_SEM_SUMS; q++) v[u][q] = block_sums[q * nblocks + ic];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool in = i0 + 256 * u < nblocks;
            a += in ? v[u][0] : 0.f;
#pragma unroll
            for (int q = 0; q < 3; q++) n[q] += in ? __float_as_uint(v[u][q + 1]) : 0u;
        }
    }
    a = sgr_wave_sum_dpp(a);  // valid in lane 63
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) n[q] += __shfl_xor(n[q], o, 64);
    if ((threadIdx.x & 63) == 63) {
        const int w = threadIdx.x >> 6;
        lsum[w] = a;
#pragma unroll
        for (int q = 0; q < 3; q++) lcnt[q][w] = n[q];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float tot = ((lsum[0] + lsum[1]) + lsum[2]) + lsum[3];
    uint32_t c[3];
#pragma unroll
    for (int q = 0; q < 3; q++) c[q] = ((lcnt[q][0] + lcnt[q][1]) + lcnt[q][2]) + lcnt[q][3];
    const float n_valid = (float)c[0];
    terms[SGR_SEM_LOSS] = tot / n_valid;  // no valid pixel: 0 / 0 = NaN like torch's mean over an empty selection
    terms[SGR_SEM_N_VALID] = n_valid;
    terms[SGR_SEM_N_OUT_OF_RANGE] = (float)c[1];
    terms[SGR_SEM_ACCURACY] = (float)c[2] / n_valid;
}

template <int NC>
__global__ void __launch_bounds__(SGR_SEM_BLOCK)
sgr_semantic_loss_bwd_kernel(int S, size_t plane, const float* __restrict__ sem, const void* __restrict__ labels, int dtype,
                             int ignore_index, int mode, const float* __restrict__ terms, const float* __restrict__ upstream,
                             float* __restrict__ grad) {
    const size_t p = (size_t)blockIdx.x * SGR_SEM_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const int64_t lab = sem_label(labels, dtype, p);
    float x[NC];
    if (sem_classify(lab, S, ignore_index) == SGR_SEM_PIX_VALID) {
        // (a valid pixel exists, so n_valid >= 1; with none the quotient is never formed)
        const float scale = upstream[0] / terms[SGR_SEM_N_VALID];
        sem_load<NC>(x, sem, plane, p, S);
        sem_backward_point<NC>(x, S, mode, (int)lab, scale);
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++) x[c] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < NC; c++)
        if (c < S) grad[c * plane + p] = x[c];
}

static int sem_check(int S, int H, int W, const float* semantic, const void* labels, int label_dtype, int mode) {
    if (S < 1 || S > SGR_SEM_MAX_CHANNELS) return sgr_set_error(SGR_E_INVALID, "S must be in [1, 32]");
    if (H <= 0 || W <= 0 || (size_t)H * W >= ((size_t)1 << 31)) return sgr_set_error(SGR_E_INVALID, "H, W must be positive, H * W < 2^31");
    if (!semantic || !labels) return sgr_set_error(SGR_E_INVALID, "semantic and labels are required");
    if (label_dtype < SGR_SEM_LABEL_U8 || label_dtype > SGR_SEM_LABEL_I64) return sgr_set_error(SGR_E_INVALID, "unknown label dtype");
    if (mode != SGR_SEM_LOGITS && mode != SGR_SEM_PROBABILITIES) return sgr_set_error(SGR_E_INVALID, "unknown mode");
    return 0;
}
static inline size_t sem_blocks(int H, int W) { return ((size_t)H * W + SGR_SEM_BLOCK - 1) / SGR_SEM_BLOCK; }

// the instantiation that holds S channels: 8, 16, 24 or 32 registers
#define SGR_SEM_DISPATCH(KERNEL, ...)                                          \
    do {                                                                       \
        if (S <= 8) KERNEL<8><<<grid, SGR_SEM_BLOCK, 0, stream>>>(__VA_ARGS__);       \
        else if (S <= 16) KERNEL<16><<<grid, SGR_SEM_BLOCK, 0, stream>>>(__VA_ARGS__); \
        else if (S <= 24) KERNEL<24><<<grid, SGR_SEM_BLOCK, 0, stream>>>(__VA_ARGS__); \
        else KERNEL<32><<<grid, SGR_SEM_BLOCK, 0, stream>>>(__VA_ARGS__);             \
    } while (0)

extern "C" {

size_t sgr_semantic_loss_workspace_floats(int S, int H, int W) {
    if (S <= 0 || H <= 0 || W <= 0) return 0;
    return SGR_SEM_SUMS * sem_blocks(H, W);
}
int sgr_semantic_loss_block_pixels(void) { return SGR_SEM_BLOCK; }
int sgr_semantic_loss_finish_span(void) { return SGR_SEM_FINISH_SPAN; }

int sgr_semantic_loss_forward(int S, int H, int W, const float* semantic, const void* labels, int label_dtype,
                              int ignore_index, int mode, float* terms, uint8_t* pred, float* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = sem_check(S, H, W, semantic, labels, label_dtype, mode)) return rc;
    if (!terms || !workspace) return sgr_set_error(SGR_E_INVALID, "terms and workspace are required");
    const size_t plane = (size_t)H * W, nblocks = sem_blocks(H, W);
    const unsigned grid = (unsigned)nblocks;
    SGR_SEM_DISPATCH(sgr_semantic_loss_map_kernel, S, plane, semantic, labels, label_dtype, ignore_index, mode, pred, workspace);
    sgr_semantic_loss_finish_kernel<<<1, 256, 0, stream>>>(workspace, nblocks, terms);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_semantic_loss_backward(int S, int H, int W, const float* semantic, const void* labels, int label_dtype,
                               int ignore_index, int mode, const float* terms, const float* upstream, float* dL_dsemantic,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = sem_check(S, H, W, semantic, labels, label_dtype, mode)) return rc;
    if (!terms || !upstream || !dL_dsemantic) return sgr_set_error(SGR_E_INVALID, "terms, upstream and dL_dsemantic are required");
    const size_t plane = (size_t)H * W;
    const unsigned grid = (unsigned)sem_blocks(H, W);
    SGR_SEM_DISPATCH(sgr_semantic_loss_bwd_kernel, S, plane, semantic, labels, label_dtype, ignore_index, mode, terms, upstream,
                     dL_dsemantic);
    SGR_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
