/* sgr_object_alpha.h -- C ABI of the OBJECT-ALPHA head of the training render: the alpha image of Gaussians [split, P) of a
 * frame blended alone, and its gradient, from the finished tile lists of the frame's sgr_forward.
 *
 * The reference's training loop regularises the objects' accumulated alpha (train.py:114-122): once the densification has
 * ended it calls render_object every iteration (lib/models/street_gaussian_renderer.py:58-72) -- a second compose, a second
 * preprocess, a second binning with its host wait, a second blend and a second whole backward -- to obtain ONE image,
 * acc_obj, and its gradient.  A tile's (depth, index)-sorted list of a contiguous subset is the frame's list with the other
 * Gaussians taken out (include/sgr_layers.h), and the per-Gaussian stage of sgr_backward does not care which kernel wrote
 * the partial rows it sums.  So the head is two kernels (csrc/sgr_object_alpha.hip) beside the shipped path: an alpha-only
 * walk forward, an alpha-only walk backward that writes partial rows in the shipped format, then the unchanged row sum and
 * per-Gaussian backward.
 *
 * FORWARD, per pixel, in float32, the entries i of the pixel's tile list with Gaussian index g_i >= split that are not
 * marked dead, in list order (the arithmetic of sgr_forward in the same mode, forward.cu:394-445, the expressions of
 * csrc/sgr_blend_layers.hip in their order):
 *   T = 1, A = 0, last = 0
 *   for each i (at list position p_i, counted from 1 inside the tile's range):
 *       alpha_i = min(0.99, opacity_i * G_i(pixel));  skip when power_i > 0 or alpha_i < 1/255
 *       test_T = T * (1 - alpha_i);  stop this pixel when test_T < 0.0001
 *       A = A + alpha_i * T;  T = test_T;  last = p_i
 *   out_alpha = A;  out_last = last
 * out_alpha is bit for bit the out_alpha of sgr_forward over Gaussians [split, P) alone (= alpha[1] of sgr_forward_layers),
 * in every switch combination and in lazy mode.  out_last is the layer's n_contrib (forward.cu:431-445): private state of
 * the backward below.
 *
 * BACKWARD, per pixel, the alpha part of backward.cu:505-640 (dL_dpixel = dL_ddepth = 0, no background term):
 *   T = 1 - layer_alpha;  last_alpha = 0;  accum = 0
 *   for the entries with g_i >= split at positions p_i <= layer_last, back to front:
 *       skip when power_i > 0 or alpha_i < 1/255      (the forward's decision: same expressions, same guard)
 *       T = T / (1 - alpha_i)
 *       accum = last_alpha + (1 - last_alpha) * accum
 *       dL_dopa = (1 - accum) * dL_dlayer_alpha * T;  last_alpha = alpha_i
 *       dL_dopacity_i += G_i * dL_dopa;  dL_dG = opacity_i * dL_dopa
 *       dL_dmean2D_i (x, y, |x| + |y|) and dL_dconic_i (x, y, w) from dL_dG as backward.cu:616-635
 * with power, G, the reciprocal of 1 - alpha and the parity mode's guard at the 1/255 threshold written as the shipped blend
 * backward writes them in that mode.  The seven sums of a (tile, Gaussian) pair over the tile's 256 pixels are reduced on
 * chip in a fixed order and written once, as a partial row of the layout sgr_backward's S = 0 kernel writes (positions 7..10
 * zero); sgr_backward's row sum and per-Gaussian stage (cov2D, projection, cov3D backward) follow unchanged.  Gradients are
 * bit-reproducible from call to call.  Rows [0, split) of every output are zero.
 *
 * The head never touches dL/dmeans2D, a statistics sink, colours or SH: the reference's object pass has its own
 * screen-space tensor that nobody reads, and nothing in train.py reads an object colour gradient.
 *
 * The "touched" bytes of the binning buffer belong to sgr_backward: sgr_layer_alpha_backward clears them before its walk
 * and again after its per-Gaussian stage, so an sgr_backward over the same forward is correct before it, after it, or
 * again after it. */
#ifndef SGR_OBJECT_ALPHA_H
#define SGR_OBJECT_ALPHA_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* After an sgr_forward of the same frame (same P, width, height, same switches; R = its return value), on its three
 * buffers, which are only read.  out_alpha [H*W] float, out_last [H*W] uint32.  One launch; split == P, P == 0 or R == 0
 * fill zeros without a walk.  -SGR_E_INVALID, before any HIP call, when split lies outside [0, P], a size is not positive
 * or a pointer that is needed is NULL. */
int sgr_layer_alpha_forward(int P, int R, int width, int height, int split, const char* geom_buffer,
                            const char* binning_buffer, const char* image_buffer, float* out_alpha, uint32_t* out_last,
                            void* stream);

/* The gradient of sum(dL_dlayer_alpha * out_alpha) with respect to the Gaussians' means3D, opacities and scales /
 * rotations (or cov3D_precomp).  layer_alpha / layer_last: the forward's two images.  means3D, scales, rotations,
 * cov3D_precomp, radii (may be NULL: the forward's own) as given to sgr_forward.  Outputs of full length P, every element
 * written: dL_dmean3D [P,3], dL_dopacity [P], dL_dscale [P,3], dL_drot [P,4], dL_dcov3D [P,6] (NULL: not wanted).
 * `scale_modifier` is IGNORED: the backward reads the value the forward left in the geometry buffer's camera block, and
 * dL_dscale lacks the chain factor scale_modifier exactly as sgr_backward's does (include/sgr.h).
 * `scratch` is called once.  The binning buffer is written (the "touched" bytes, left cleared).  -SGR_E_INVALID, before any
 * HIP call and before the allocation callback, for the argument errors of the forward or a NULL input / output. */
int sgr_layer_alpha_backward(int P, int R, int width, int height, int split, const float* means3D, const float* scales,
                             float scale_modifier, const float* rotations, const float* cov3D_precomp, const int* radii,
                             char* geom_buffer, char* binning_buffer, char* image_buffer, const float* layer_alpha,
                             const uint32_t* layer_last, const float* dL_dlayer_alpha, float* dL_dmean3D,
                             float* dL_dopacity, float* dL_dscale, float* dL_drot, float* dL_dcov3D, sgr_alloc_fn scratch,
                             void* scratch_user, int debug, void* stream);

#ifdef __cplusplus
}
#endif
#endif
