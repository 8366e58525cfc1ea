/* sgr_semantic_loss.h -- C ABI of the fused cross-entropy on the rendered semantic head: the one image-space consumer of
 * the rasterizer's outputs that sgr_frame_loss.h does not cover.  It produces the dL/dsemantics image [S,H,W] that the
 * rasterizer's backward reads.
 *
 * The reference renders the head (street_gaussian_renderer.py:254-264, semantic_mode 'logits' / 'probabilities' of
 * gaussian_model.py:243-247), carries cfg.optim.lambda_semantic and the ground-truth convention "label < 0 is invalid"
 * (lib/utils/sem_utils.py:35), and leaves the loss to the trainer.  This op is that loss:
 *     logits:         F.cross_entropy(semantic.permute(1, 2, 0).reshape(-1, S), labels.reshape(-1), ignore_index=...)
 *     probabilities:  street_gaussian_renderer.py:261-262 ("normalize to probabilities", "change for cross entropy loss")
 *                     followed by F.nll_loss
 *
 * A pixel is VALID when its label is in [0, S) and differs from ignore_index.  Every other pixel contributes nothing and
 * gets a zero gradient; labels >= S that are not ignore_index are counted as well (terms[SGR_SEM_N_OUT_OF_RANGE]), so a
 * caller can notice a bad label map without a device assert.  Per valid pixel with label l, all in float32:
 *     logits         m = max_c x_c
 *                    loss_p = (m - x_l) + log(sum_c exp(x_c - m))                        [= lse - x_l]
 *                    d loss_p / d x_c = exp(x_c - m) / sum_k exp(x_k - m) - [c == l]     [= exp(x_c - lse) - [c == l]]
 *     probabilities  eps = 1e-8f,  s = sum_c r_c (c ascending),  q_l = r_l / (s + eps)
 *                    loss_p = -log(q_l + eps)
 *                    d loss_p / d r_c = -([c == l] / (s + eps) - r_l / (s + eps)^2) / (q_l + eps)
 * exp and log are the hardware's (v_exp_f32, v_log_f32).
 *
 * Forward: ONE map kernel (a lane per pixel, consecutive lanes on consecutive pixels of a channel plane, the pixel's S
 * values held in registers: every element of `semantic` is read once) and ONE finishing workgroup that adds the block
 * partials in a fixed order.  No float atomics: every result is bit-reproducible from run to run.  The counts are summed as
 * integers and are exact; they are stored as floats (exact up to 2^24 pixels).
 * Backward: ONE kernel, every element of dL_dsemantic written exactly once.  It recomputes m and the sum from the values
 * it reads anyway, so the forward saves NOTHING per pixel for it: lse rounded to float32 would put ulp(lse) / 2 into every
 * probability, and the recomputation costs no memory traffic.  The backward reads the forward's `terms` on the device.
 *
 * All arrays are DEVICE memory; nothing is allocated and nothing waits on the host.  No access is wider than 4 bytes
 * (int64 labels are read as two words), so 4-byte-aligned views are fine. */
#ifndef SGR_SEMANTIC_LOSS_H
#define SGR_SEMANTIC_LOSS_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGR_SEM_MAX_CHANNELS 32 /* the rasterizer's own limit on S */

/* indices into `terms` (four device floats) */
enum {
    SGR_SEM_LOSS = 0,           /* sum of loss_p / n_valid; NaN when n_valid == 0, like F.cross_entropy */
    SGR_SEM_N_VALID = 1,        /* number of valid pixels */
    SGR_SEM_N_OUT_OF_RANGE = 2, /* number of labels >= S that are not ignore_index */
    SGR_SEM_ACCURACY = 3,       /* share of the valid pixels whose first-maximum channel (np.argmax's tie rule, as
                                 * vis_semantic_label of lib/utils/sem_utils.py:22 uses) equals the label; NaN when none */
    SGR_SEM_TERMS = 4
};
enum { SGR_SEM_LOGITS = 0, SGR_SEM_PROBABILITIES = 1 };                          /* mode */
enum { SGR_SEM_LABEL_U8 = 0, SGR_SEM_LABEL_I32 = 1, SGR_SEM_LABEL_I64 = 2 }; /* label_dtype */

/* floats of `workspace` (four block partials per block of the map kernel; free again after the forward) */
size_t sgr_semantic_loss_workspace_floats(int S, int H, int W);
/* Pixels per block of the map kernel, and block partials per quantity that one trip of the finishing workgroup's loop
 * covers: an image of more than finish_span * block_pixels pixels gives that loop a second trip. */
int sgr_semantic_loss_block_pixels(void);
int sgr_semantic_loss_finish_span(void);

/* terms[SGR_SEM_TERMS] <- the scalars above; pred (uint8 [H,W], or NULL) <- the first-maximum channel of every pixel, what
 * lib/utils/sem_utils.py:22 computes on the host.  semantic: float32 planar [S,H,W], 1 <= S <= SGR_SEM_MAX_CHANNELS and
 * H * W < 2^31 (else SGR_E_INVALID); labels: [H,W] of label_dtype.  Two launches. */
int sgr_semantic_loss_forward(int S, int H, int W, const float* semantic, const void* labels, int label_dtype,
                              int ignore_index, int mode, float* terms, uint8_t* pred, float* workspace, void* stream);

/* ONE launch: dL_dsemantic [S,H,W] <- upstream[0] / n_valid * d loss_p / d x_c on valid pixels and exactly 0 on every other
 * pixel, n_valid read from the forward's terms on the device.  With n_valid == 0 every element is exactly 0, not NaN. */
int sgr_semantic_loss_backward(int S, int H, int W, const float* semantic, const void* labels, int label_dtype,
                               int ignore_index, int mode, const float* terms, const float* upstream, float* dL_dsemantic,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif
