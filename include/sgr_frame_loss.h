/* sgr_frame_loss.h -- C ABI of the fused frame loss: every image-space term of a training step in one op (SURVEY.md 8f,
 * row n3: "a fused loss + dL_dout_* producer would feed the blend backward without materialising intermediates").
 *
 * train.py:100-133 of the reference, with loss_utils.py:21-37 (l1_loss), :61-78 (psnr) and :80-125 (ssim):
 *     Ll1   = l1_loss(image, gt, mask)                                                              train.py:101
 *     loss  = (1 - lambda_dssim) * lambda_l1 * Ll1 + lambda_dssim * (1 - ssim(image, gt, mask=mask))         :103
 *     sky   = where(sky_mask, -log(1 - a), -log(a)).mean() [* lambda_sky_scale[cam]],  a = clamp(acc)    :107-110
 *     loss += lambda_sky * sky                                                                               :112
 *     obj   = where(obj_bound, -(b log b + (1 - b) log(1 - b)), -log(1 - b)).mean(),  b = clamp(acc_obj) :117-120
 *     loss += lambda_reg * obj                                                                               :122
 *     lidar = mean of the int(keep * n) smallest |depth / (acc + 1e-10) - lidar_depth|                   :126-130
 *             over the n pixels with lidar_depth > 0 and mask; acc is the UNCLAMPED render_pkg['acc']
 *     loss += lambda_depth_lidar * lidar                                                                     :132
 * and, for the progress bar (train.py:173), psnr = 20 log10(1 / sqrt(mse)), mse = mean (image - gt)^2 over the masked
 * pixels' C values (loss_utils.py:76-77).
 *
 * Per pixel, one map kernel over 16x16 tiles: for every channel the SSIM map value M and dM/dmu1, dM/dsigma1^2,
 * dM/dsigma12 (kept for the backward), |a - b| and (a - b)^2 on masked pixels; once per pixel the sky and the object term on
 * the clamped accumulations (clamp bounds 1e-6f and 1.0f - 1e-6f in float32) and the LiDAR error.  Block partial sums go
 * to the workspace in block order; one finishing workgroup adds them in a fixed order and evaluates the scalars, so every
 * result is bit-reproducible (the only atomic is the integer count of LiDAR pixels).  Each term keeps what sgr_loss.h
 * states for its stand-alone op: NaN for an empty mask or no LiDAR pixel, int(keep * n) in double, ties at the threshold
 * share the remaining slots.
 *
 * All arrays are DEVICE float32 ([C,H,W] planar images, [H,W] maps) or bytes (0/1 masks); nothing is allocated and
 * nothing waits on the host. */
#ifndef SGR_FRAME_LOSS_H
#define SGR_FRAME_LOSS_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into `terms` (eight device floats) */
enum {
    SGR_FL_L1 = 0,    /* l1_loss(image, gt, mask)                                  scalar_dict['l1_loss'] */
    SGR_FL_SSIM = 1,  /* ssim(image, gt, mask=mask) */
    SGR_FL_SKY = 2,   /* mean * f32(sky_scale), as train.py:110 logs it            scalar_dict['sky_loss'] */
    SGR_FL_OBJ = 3,   /*                                                           scalar_dict['obj_acc_loss'] */
    SGR_FL_LIDAR = 4, /*                                                           scalar_dict['lidar_depth_loss'] */
    SGR_FL_MSE = 5,   /* mean (image - gt)^2 over the masked pixels' C values */
    SGR_FL_PSNR = 6,  /* 20 log10(1 / sqrt(mse)) */
    SGR_FL_LOSS = 7,  /* float32, in train.py's order, every weight rounded to float32 first:
                       *   w_l1 * l1 + lambda_dssim * (1 - ssim), then + lambda_sky * sky, + lambda_reg * obj,
                       *   + lambda_depth_lidar * lidar.  A term that is off is written as 0 and is NOT added (no 0 * x). */
    SGR_FL_TERMS = 8
};

/* HOST memory, read during the call.  A term is on exactly when both pointers of its pair are non-NULL; one pointer of a
 * pair alone is an error (SGR_E_INVALID).  The colour term is always on. */
typedef struct sgr_frame_loss_args {
    const float* image;        /* [C,H,W] rendered colour */
    const float* gt;           /* [C,H,W] */
    const uint8_t* mask;       /* [H,W] or NULL: the pixels that count (colour and LiDAR terms) */
    const float* acc;          /* [H,W] accumulated opacity: sky term (with sky_mask) and LiDAR term (with depth) */
    const uint8_t* sky_mask;   /* [H,W] */
    const float* acc_obj;      /* [H,W] accumulated opacity of the object layer (with obj_bound) */
    const uint8_t* obj_bound;  /* [H,W] */
    const float* depth;        /* [H,W] accumulated depth (with lidar_depth; needs acc) */
    const float* lidar_depth;  /* [H,W], <= 0 where there is no return */
    float w_l1;                /* (1 - lambda_dssim) * lambda_l1, evaluated in double by the caller, rounded here */
    float lambda_dssim;
    float lambda_sky;
    float sky_scale;           /* lambda_sky_scale[cam], 1 when the list is empty */
    float lambda_reg;
    float lambda_depth_lidar;
    double keep;               /* 0.95 in train.py:128 -- a double, like the Python float */
} sgr_frame_loss_args;

/* bytes of `saved` (what the forward leaves for the backward: the SSIM partials, the LiDAR keys and selection, counts)
 * and floats of `workspace` (block partial sums; free again after the call that used it) */
size_t sgr_frame_loss_saved_bytes(int C, int H, int W);
size_t sgr_frame_loss_workspace_floats(int C, int H, int W);
/* Block sums per quantity that one trip of the finishing workgroups' loop covers: an image of more 16x16 tiles (frame
 * loss; workspace floats / 6) or more 256-pixel blocks (mse; workspace floats / 2) gives the loop a second trip. */
int sgr_frame_loss_finish_span(void);

/* terms[SGR_FL_TERMS] <- the scalars above.  Launches: one clear of the selection's counters, the map kernel, the LiDAR
 * term's radix select when that term is on (sgr_loss.h), one finishing workgroup. */
int sgr_frame_loss_forward(int C, int H, int W, const sgr_frame_loss_args* args, float* terms, char* saved,
                           float* workspace, void* stream);

/* ONE launch: every non-NULL gradient image is written once, = upstream[0] * d terms[SGR_FL_LOSS] / d input.
 *   dL_dimage  [C,H,W]  the 11x11 convolution of the saved partials (weight -lambda_dssim / (C*H*W)) plus
 *                       w_l1 * sign(image - gt) / count; exactly 0 on masked-out pixels
 *   dL_dacc    [H,W]    sky term (0 where the clamp is active) + LiDAR term, added in registers
 *   dL_ddepth  [H,W]    LiDAR term
 *   dL_dacc_obj [H,W]   object term
 * A NULL output is not written and its loads are skipped; an output whose terms are all off is an error.  args, saved and
 * terms are the forward's (the kernel reads the counts and the selection from `saved`); workspace is not used today. */
int sgr_frame_loss_backward(int C, int H, int W, const sgr_frame_loss_args* args, const float* terms, const char* saved,
                            float* workspace, const float* upstream, float* dL_dimage, float* dL_dacc, float* dL_ddepth,
                            float* dL_dacc_obj, void* stream);

/* psnr(img1, img2, mask) of loss_utils.py:61-78 without the host wait of img[mask]:
 * out[0] = mse over the masked pixels' C values, out[1] = 20 log10(1 / sqrt(mse)), out[2] = number of values averaged.
 * An empty mask gives NaN.  workspace: sgr_mse_workspace_floats floats. */
size_t sgr_mse_workspace_floats(int C, int H, int W);
int sgr_mse_forward(int C, int H, int W, const float* a, const float* b, const uint8_t* mask, float* out, float* workspace,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
