/* sgr_layers.h -- C ABI of the layered forward: the composite of sgr_forward plus the images of two LAYERS of the same
 * frame, Gaussians [0, split) and [split, P), from ONE front end and one binning.
 *
 * The reference's trajectory renderer asks for three images per frame (StreetGaussianRenderer.render_all,
 * lib/models/street_gaussian_renderer.py:13-40): the composite, the background alone (render_background, :42-56) and the
 * objects alone (render_object, :58-72), each a whole rasterizer forward over its own Gaussian set on a white background.
 * The three share everything up to the blend: the preprocess is per Gaussian, and every tile's (depth, index)-sorted list of
 * a contiguous subset is the frame's list with the other Gaussians taken out.  sgr_forward_layers therefore runs the
 * launches of sgr_forward unchanged and then ONE more kernel (csrc/sgr_blend_layers.hip) that walks the same tile ranges,
 * the same final instance list and the same per-Gaussian records.
 *
 * The contract, per pixel and per layer l, in float32, the list entries i of the pixel's tile that belong to layer l taken
 * in list order (the arithmetic of sgr_forward in the same mode, forward.cu:394-445):
 *   T = 1, C = (0, 0, 0), A = 0
 *   for each i:  alpha_i = min(0.99, opacity_i * G_i(pixel));  skip when power_i > 0 or alpha_i < 1/255
 *                test_T = T * (1 - alpha_i);  stop this layer of this pixel when test_T < 0.0001
 *                w = alpha_i * T;  C_c = fma(rgb_i_c, w, C_c);  A = A + w;  T = test_T
 *   color[l]_c = C_c + T * background_c   (multiply and add rounded separately);  alpha[l] = A
 *   clamp: color[l]_c = clamp(color[l]_c, 0, 1), NaN kept (render_kernel outside training,
 *   street_gaussian_renderer.py:242-243)
 * Each layer has its own T and its own stop: the composite's transmittance plays no part, so an opaque layer 0 in front does
 * not end layer 1.  With the same expressions on the same list order, color[l] / alpha[l] are bit for bit what sgr_forward
 * returns as out_color / out_alpha for Gaussians of layer l alone with `background` as its background, in every switch
 * combination and in lazy mode.  A layer without Gaussians (split == 0, split == P, or P == 0 -- the reference's empty
 * model, street_gaussian_renderer.py:138-151) is the background colour with alpha 0.
 *
 * Inference only: there is no backward for the layer images.  The composite's outputs and buffers are those of sgr_forward
 * (the extra kernel writes none of them), so sgr_backward may follow as after sgr_forward. */
#ifndef SGR_LAYERS_H
#define SGR_LAYERS_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgr_layer_images {
    int split;                /* Gaussians [0, split) = layer 0, [split, P) = layer 1; 0 <= split <= P */
    const float* background;  /* 3 floats, device: the colour behind both layer images */
    int clamp;                /* 1: layer colours clamped to [0, 1] on store */
    float* color[2];          /* [3, H, W] each */
    float* alpha[2];          /* [1, H, W] each */
} sgr_layer_images;

/* sgr_forward (same parameters, same order, same launches, same return value) followed by the layer kernel.
 * layers == NULL is sgr_forward.  -SGR_E_INVALID, before any HIP call and any allocation callback, when split lies
 * outside [0, P], background is NULL or one of the four output pointers is NULL. */
int sgr_forward_layers(sgr_alloc_fn geometry_buffer, void* geometry_user, sgr_alloc_fn binning_buffer, void* binning_user,
                       sgr_alloc_fn image_buffer, void* image_user, int P, int D, int M, int S, const float* background,
                       int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                       const float* semantics, const float* opacities, const float* scales, float scale_modifier,
                       const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                       const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                       float* out_depth, float* out_alpha, float* out_semantic, int* radii, int debug, void* stream,
                       const sgr_layer_images* layers);

#ifdef __cplusplus
}
#endif
#endif
