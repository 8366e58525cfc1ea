/* sgr_sky_step.h -- C ABI of the sky cube map's optimiser: the texture backward's gather and the Adam step of
 * include/sgr_optim.h in one kernel, over the part of the map that has ever received a gradient
 * (street_gaussians_amd/sky.py: SkyAdam).
 *
 * The reference steps its sky model with a dense torch.optim.Adam(eps=1e-15) over all 6 R R 3 elements every iteration
 * (lib/models/sky_cubemap.py:53-75), R = 1024 by default: 18.9 M elements, of which a frame's sky pixels touch a few per
 * cent.  Two facts make the dense passes avoidable without changing a bit of the result:
 *   - an element with g = 0, m = 0 and v = 0 is left bitwise unchanged by the five operations of include/sgr_optim.h:
 *     m and v stay +0, d = 0 / bc2_sqrt + eps = eps, p + step_size * (0 / eps) = p + (-0) = p, for every p and step --
 *     given eps > 0 in f32 (eps = 0 makes 0 / 0) and a learning rate >= 0 (step_size <= 0: a positive one would turn a
 *     p of -0 into +0); the caller refuses anything else;
 *   - an element that has once received a gradient keeps moving while its moments decay, so the set that has to be
 *     stepped is "ever touched", and it only grows.
 * The map is cut into BLOCKS of sgr_sky_step_block_texels() (256) consecutive texels of the flat [6, R, R] index -- one
 * workgroup, one lane per texel; the last block of a map may be partial.  `active` holds one byte per block,
 * ceil(6 R R / block) bytes, 0 or 1; the caller zeroes it once and keeps it with the moments.  The invariant the caller
 * maintains: active[b] = 1 for every block with a non-zero exp_avg or exp_avg_sq element (after loading a checkpoint,
 * rebuild it from the moments).
 *
 * One training step:
 *   sgr_sky_forward                as before
 *   sgr_sky_backward_deferred      sgr_sky_backward without the texture backward's gather: dL/drgb, dL/dacc and
 *                                  dL/daffine are bit-identical to sgr_sky_backward's; the key, sort, records and starts
 *                                  stages of the texture backward (include/sgr_texture.h) run on the compacted sky pixels
 *                                  with the device-side count and stay in `cube_work`; active[b] is set to 1 for every
 *                                  block that holds a tap texel of one of this backward's samples (the four taps of the
 *                                  sample's cell: a seam tap on the neighbouring face included, a missing corner tap
 *                                  not).  Plain byte stores of the same value from many lanes: no atomics.  Sentinel keys
 *                                  and positions past the device count mark nothing.  No dL/dcube exists.
 *   sgr_sky_adam_step              one launch over all blocks.  A block whose byte is 0 exits after reading it.  In an
 *                                  active block each lane (1) sums its texel's gradient exactly as the texture backward's
 *                                  gather does -- its four own cells, then the border cells of the neighbouring faces, in
 *                                  double in that fixed order, rounded to f32 once (the contract of include/sgr_texture.h)
 *                                  -- and (2) applies the five operations of include/sgr_optim.h to the texel's three
 *                                  elements of cube / exp_avg / exp_avg_sq: f32, no contraction, correctly rounded
 *                                  division and square root, denormals kept.  Every element is written by exactly one
 *                                  lane.  The result is bitwise that of sgr_sky_backward followed by sgr_adam_step (or
 *                                  torch.optim.Adam) over the whole map.
 * step_size = -(lr / bc1) and bc2_sqrt are computed by the caller in double as include/sgr_optim.h states and rounded to
 * f32; they, eps and the betas are kernel arguments: nothing is uploaded.
 *
 * All arrays are DEVICE arrays, float32 unless stated; cube, exp_avg and exp_avg_sq are [6, R, R, 3] and need only their
 * natural 4-byte alignment.  Nothing allocates and nothing synchronises with the host.  cube_work is read by
 * sgr_sky_adam_step: keep it untouched between the deferred backward and the step, on one stream. */
#ifndef SGR_SKY_STEP_H
#define SGR_SKY_STEP_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"
#include "sgr_sky.h"

#ifdef __cplusplus
extern "C" {
#endif

/* texels per activity block */
int sgr_sky_step_block_texels(void);

/* bytes of the deferred-gradient workspace `cube_work` for an H x W frame: a header, the texture backward's sort
 * buffers, starts, rec and gs; 0 when the arguments are invalid. */
size_t sgr_sky_step_workspace_bytes(int H, int W, int R);

/* sgr_sky_backward's arguments with dL_dcube replaced by cube_work (sgr_sky_step_workspace_bytes) and active;
 * scratch: sgr_sky_workspace_bytes(.., SGR_SKY_SCRATCH_DEFERRED) (a SGR_SKY_SCRATCH block is large enough too). */
int sgr_sky_backward_deferred(int H, int W, int R, int C, const float* dL_dout, const float* rgb, const float* acc,
                              const float* affine, int flags, const void* saved, float* dL_drgb, float* dL_dacc,
                              void* cube_work, uint8_t* active, float* dL_daffine, void* scratch, void* stream);

/* One Adam step of the active blocks of cube with the gradient held in cube_work.  cube_work == NULL: no samples, a
 * step with g = 0 (the touched texels still move).  SGR_E_INVALID: R < 1, a missing pointer, betas outside [0, 1). */
int sgr_sky_adam_step(int R, float* cube, float* exp_avg, float* exp_avg_sq, const void* cube_work, const uint8_t* active,
                      float step_size, float bc2_sqrt, float eps, double beta1, double beta2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
