/* sgr_optim.h -- C ABI of the fused per-segment Adam step over flat parameter tensors (street_gaussians_amd/optim.py).
 *
 * The reference trains one torch.optim.Adam(eps=1e-15) per sub-model, with seven named groups each (xyz, f_dc, f_rest,
 * opacity, scaling, rotation, semantic; lib/models/gaussian_model.py:292-304, gaussian_model_actor.py:170-192).  A
 * CHUNK is the block of one (segment, attribute) inside a flat tensor: its parameter, first and second moment live at
 * p / m / v, count floats each.  One call updates every chunk listed in this step's records, in one launch.
 *
 * Per element, f32, no contraction, correctly rounded division and square root, denormals preserved -- the op order of
 * torch/optim/adam.py: _multi_tensor_adam (c1 = (float)(1 - beta1), c2 = (float)(1 - beta2)):
 *   1. m = m + c1 * (g - m)                 (_foreach_lerp_, weight < 0.5 branch)
 *   2. v = v * beta2                        (_foreach_mul_)
 *   3. v = v + c2 * (g * g)                 (_foreach_addcmul_)
 *   4. d = sqrtf(v) / bc2_sqrt + eps        (_foreach_sqrt, _foreach_div_, _foreach_add_)
 *   5. p = p + step_size * (m / d)          (_foreach_addcdiv_)
 * with, per chunk, computed by the caller in double exactly as torch's Python does and then rounded to f32:
 *   bc1 = 1 - beta1 ** step,  bc2_sqrt = (1 - beta2 ** step) ** 0.5,  step_size = -(lr / bc1)
 * (step = the chunk's step count after this step's increment).  NaN and inf propagate through the sequence.
 *
 * Tables (DEVICE arrays):
 *   chunks   [n_chunks]   sgr_adam_chunk: p, m, v, count; built once per layout
 *   records  [n_records]  sgr_adam_record, one per chunk stepped now, in increasing span_start with records[0].span_start
 *                         = 0: the gradient g of that chunk (count floats), the index of its chunk, its first span and
 *                         its f32 scalars.  A chunk without a record is not touched.  One step takes at most
 *                         sgr_adam_max_records() records (the span starts of all of them sit in LDS); a longer table
 *                         is refused and nothing is launched: the caller splits the step.
 * A span is sgr_adam_span_elems() consecutive elements of one chunk; a chunk of count elements has
 * ceil(count / span) spans, record i owns spans [span_start_i, span_start_{i+1}) and n_spans is the total.  Chunks
 * may start at any 4-byte offset: where p, g, m and v are equally aligned modulo 16 bytes the body moves as float4,
 * the rest element by element.  Chunks must not overlap.  Nothing synchronises with the host; the tables are read by
 * the launch on `stream`, so the caller keeps them alive and unchanged until it completes. */
#ifndef SGR_OPTIM_H
#define SGR_OPTIM_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgr_adam_chunk {
    float* p;
    float* m;        /* exp_avg    */
    float* v;        /* exp_avg_sq */
    int64_t count;   /* floats */
} sgr_adam_chunk;    /* 32 bytes */

typedef struct sgr_adam_record {
    const float* g;
    int32_t chunk;
    int32_t span_start;
    float step_size;  /* -(lr / bc1) */
    float bc2_sqrt;
    float eps;
    int32_t pad;
} sgr_adam_record;   /* 32 bytes */

/* elements per span (a power of two, a multiple of 4) */
int sgr_adam_span_elems(void);
/* workgroups of the largest grid: a step of more spans walks them grid-stride, span += the grid */
int sgr_adam_max_blocks(void);
/* records one step takes at most (4096) */
int sgr_adam_max_records(void);

/* One Adam step of every chunk named by a record.  beta1 / beta2 are the optimiser's betas (c1 = 1 - beta1 and
 * c2 = 1 - beta2 are formed in double, then rounded).  SGR_E_INVALID: negative sizes, n_spans > 0 without tables,
 * betas outside [0, 1), n_records > sgr_adam_max_records(), n_spans > 2^31 - 1. */
int sgr_adam_step(const sgr_adam_chunk* chunks, int n_chunks, const sgr_adam_record* records, int n_records,
                  int64_t n_spans, double beta1, double beta2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
