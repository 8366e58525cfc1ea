/* sgr_sky.h -- C ABI of the fused sky composite and colour correction: Step 2 of the reference's
 * StreetGaussianRenderer.render (lib/models/street_gaussian_renderer.py:107-117) as a few HIP kernels that never
 * synchronise with the host:
 *
 *   sky_color = pc.sky_cubemap(camera, acc.detach())        SkyCubeMap.forward, lib/models/sky_cubemap.py:77-123
 *   rgb = rgb + sky_color * (1 - acc)
 *   rgb = pc.color_correction(camera, rgb)                  ColorCorrection.forward, lib/models/color_correction.py:129-132
 *   rgb = clamp(rgb, 0, 1)                                  when cfg.mode != 'train'
 *
 * Layouts (DEVICE arrays, float32 unless stated, contiguous):
 *   rgb, out [3, H, W]   acc [1, H, W]   cube [6, R, R, 3] (include/sgr_texture.h)   K [3, 3]   w2c [4, 4] (world to
 *   camera, row-major: R = w2c[:3, :3], T = w2c[:3, 3])   sky_mask [H, W] uint8 (bool) or NULL   perturb_x, perturb_y
 *   [H, W] or NULL   affine [3, 4] or NULL (no colour correction)
 *
 * The contract, per pixel (x, y), in float32 with contraction off:
 *   mask  TRAIN and sky_mask given: sky_mask[y, x] or y < 50 (the caller's mask is not written);
 *         otherwise (1 - acc) > 1e-3f
 *   ray   xy1 = (x + px, y + py, 1), (px, py) = (perturb_x, perturb_y)[y, x] when TRAIN, else (0.5, 0.5);
 *         Ki = K^-1 in closed form (adjugate / det, per element);
 *         pc_i = (xy1_0 Ki_i0 + xy1_1 Ki_i1) + xy1_2 Ki_i2;  pw_j = ((pc_0 - T_0) R_0j + (pc_1 - T_1) R_1j) + (pc_2 - T_2) R_2j;
 *         o_j = -((R_0j T_0 + R_1j T_1) + R_2j T_2);  d = pw - o;  d = d / sqrt((d_0^2 + d_1^2) + d_2^2)
 *         (get_rays_torch's order, lib/utils/graphics_utils.py:186-207, with its subtract-then-add-back of T)
 *   sky   mask pixel: clamp(lookup(cube, d), 0, 1), the lookup being the device function of texture()'s forward;
 *         other pixels: the fill, 1 (WHITE) or 0
 *   c     c = rgb + sky (1 - acc)
 *   cc    out_i = ((A_i0 c_0 + A_i1 c_1) + A_i2 c_2) + A_i3 when affine is given, else out = c
 *   clamp out = clamp(out, 0, 1) when CLAMP
 * Clamps keep NaN; their backward passes 0 <= x <= 1 inclusive, as torch.clamp's.
 *
 * The forward compacts the mask pixels in row-major order (the order of the reference's rays_d[mask]) with a device-wide
 * scan; their count stays on the device.  The backward writes dL/drgb, dL/dacc, dL/daffine (per-block partials, then a
 * fixed-order sum: no float atomics) and dL/dcube, which is texture()'s backward (key, sort, starts, records, gather) on
 * the compacted sky pixels with upstream (1 - acc) dL/dsky, zeroed where the sky clamp stopped it: every element written
 * once, bit-reproducible.  Nothing synchronises with the host and nothing allocates: the saved state and the scratch come
 * from the caller. */
#ifndef SGR_SKY_H
#define SGR_SKY_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SGR_SKY_TRAIN = 1, /* cfg.mode == 'train': the sky-mask rule and the perturbed rays */
    SGR_SKY_WHITE = 2, /* cfg.model.sky.white_background: fill 1 instead of 0 */
    SGR_SKY_CLAMP = 4, /* clamp the output to [0, 1] (cfg.mode != 'train') */
};
enum { SGR_SKY_SAVED = 0, SGR_SKY_SCRATCH = 1, SGR_SKY_SCRATCH_DEFERRED = 2 };

/* bytes of the state the forward saves for the backward (part SGR_SKY_SAVED), of the backward's scratch
 * (SGR_SKY_SCRATCH) or of the deferred backward's (SGR_SKY_SCRATCH_DEFERRED, include/sgr_sky_step.h: without the
 * texture stages' buffers); 0 when the arguments are invalid.  C = 3 only. */
size_t sgr_sky_workspace_bytes(int H, int W, int R, int C, int part);

/* out [3, H, W]; saved: sgr_sky_workspace_bytes(.., SGR_SKY_SAVED), kept untouched until the backward. */
int sgr_sky_forward(int H, int W, int R, int C, const float* rgb, const float* acc, const float* cube, const float* K,
                    const float* w2c, const uint8_t* sky_mask, const float* perturb_x, const float* perturb_y,
                    const float* affine, int flags, float* out, void* saved, void* stream);

/* dL_drgb [3, H, W], dL_dacc [1, H, W], dL_dcube [6, R, R, 3] (every element written), dL_daffine [3, 4] (written when
 * affine is given); the arguments are the forward's.  scratch: sgr_sky_workspace_bytes(.., SGR_SKY_SCRATCH). */
int sgr_sky_backward(int H, int W, int R, int C, const float* dL_dout, const float* rgb, const float* acc,
                     const float* affine, int flags, const void* saved, float* dL_drgb, float* dL_dacc, float* dL_dcube,
                     float* dL_daffine, void* scratch, void* stream);

/* Test entry: the forward's ray of every pixel, rays [H, W, 3], and its K^-1, kinv [3, 3] (row-major). */
int sgr_sky_test_rays(int H, int W, const float* K, const float* w2c, const float* perturb_x, const float* perturb_y,
                      int flags, float* rays, float* kinv, void* stream);

/* Test entry: the stable radix sort of the first *dev_n of n (key, value) pairs, the count read on the device (the sky
 * backward's sort); same arguments and result as sgr_test_sort32 otherwise. */
int sgr_test_sort32_count(uint32_t* keys0, uint32_t* keys1, uint32_t* vals0, uint32_t* vals1, uint32_t n, int end_bit,
                          int max_bits, const uint32_t* dev_n, uint32_t* hist, uint32_t* scan_tmp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
