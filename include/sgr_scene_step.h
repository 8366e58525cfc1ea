/* sgr_scene_step.h -- the scene-graph compose backward of include/sgr_scene_frame.h with the optimiser as its sink:
 * every value the plain backward would store into a Gaussian-group gradient is instead applied to that element as one
 * Adam step (street_gaussians_amd/optim.py: SegmentedAdam.sink, scene.py: FlatScene.compose(grad_sink=)).
 *
 * The plain hand-over writes one f32 gradient per raw parameter of the frame's models (sgr_scene_compose_backward_ex),
 * and sgr_adam_step (include/sgr_optim.h) then reads each of them exactly once next to p, m and v.  Nothing else
 * consumes the gradient, so the backward kernels can step the element they have just formed the gradient of: the
 * gradient's store and load, the step's launch and tables, the zero spans of the absent models and the gradient
 * tensors themselves go away.  The result is bitwise that of the two calls.
 *
 * The rule: an element is stepped with the value g if and only if sgr_scene_compose_backward_ex, given a gradient
 * array for that element's group, would have written g to its gradient.  That is literal: the zeros written for
 * features_dc rows k > 0 of an actor without idft, for a semantic block with S <= 0 or without dL_dsemantics, and for
 * a group whose upstream gradient is NULL (dL_dshs, dL_dscales, ...) are steps with g = 0 (the moments decay and the
 * element moves); the static-logits semantic copy and the Fourier product d * idft[k] are stepped by the SH kernel.  A
 * model that is not in `segs` is not touched: its bytes and its step counts stay, as torch's Adam skips a parameter
 * without a gradient.
 *
 * Per element the arithmetic is that of include/sgr_optim.h (the five operations, f32, no contraction, correctly
 * rounded division and square root, denormals kept; csrc/sgr_adam_math.h is the one definition both kernels inline).
 * g enters it rounded to f32 exactly as the plain backward stores it: both flavours of a kernel form g with the same
 * device code, and no multiply that forms g is contracted into the step's first subtraction.  step_size = -(lr / bc1)
 * and bc2_sqrt are computed by the caller in double as include/sgr_optim.h states, for the group's step count AFTER
 * this step's increment, and rounded to f32.
 *
 * Reads before writes: the parameters are read and written by the same launch.  Every lane owns its row (one Gaussian
 * for xyz, rotation, scaling, opacity and semantic; one float for the SH rows) and reads every element of a leaf it
 * needs for a gradient -- xyz for the pose and correction partials, rotation, scaling, opacity, the semantic row's
 * maximum and sum for the softmax, idft -- before it writes that element; no lane reads another lane's row.  The
 * reductions that follow (pose, correction: two levels) read only the partials, the poses and the correction, none
 * of which is stepped here.  The forward of the frame must have completed on the same stream.
 *
 * The actor pose gradient (grads[k].pose) and the correction gradient (frame->correction_grad) are gradients as
 * before: the same bits, the same fixed-order reductions.
 *
 * All pointers are DEVICE pointers unless noted; `segs`, `steps` and `grads` are HOST arrays.  Plain C. */
#ifndef SGR_SCENE_STEP_H
#define SGR_SCENE_STEP_H
#include <stddef.h>
#include <stdint.h>
#include "sgr_scene.h"
#include "sgr_scene_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGR_SCENE_STEP_GROUPS 7
/* the groups in the order of optim.GROUPS: the segment's xyz, features_dc, features_rest, opacity, scaling, rotation,
 * semantic */
#define SGR_STEP_XYZ 0
#define SGR_STEP_F_DC 1
#define SGR_STEP_F_REST 2
#define SGR_STEP_OPACITY 3
#define SGR_STEP_SCALING 4
#define SGR_STEP_ROTATION 5
#define SGR_STEP_SEMANTIC 6

/* One group of one segment: the moments of the block the segment's parameter pointer addresses (same element offsets,
 * same alignment: rotation's are read as float4) and the step's two scalars.  m == NULL: the group is neither stepped
 * nor written. */
typedef struct sgr_scene_step_group {
    float* m;        /* exp_avg    */
    float* v;        /* exp_avg_sq */
    float step_size; /* -(lr / bc1) */
    float bc2_sqrt;
} sgr_scene_step_group;

/* Runs parallel to `segs`: steps[k] belongs to segs[k]. */
typedef struct sgr_scene_step {
    sgr_scene_step_group group[SGR_SCENE_STEP_GROUPS];
} sgr_scene_step;

/* sgr_scene_compose_backward_ex with the Adam step as the sink of the Gaussian groups.  The parameters segs[k].xyz ...
 * segs[k].semantic of every stepped group are WRITTEN (the const of sgr_scene_segment's pointers is the forward's).
 * grads: NULL, or per segment only .pose (the other seven must be NULL); frame as in sgr_scene_compose_backward_ex
 * (its zero spans now name the pose rows of absent actors at most).  beta1 / beta2 / eps are the optimiser's: c1 and
 * c2 are formed in double and rounded once, as sgr_adam_step does.
 * SGR_E_INVALID: what sgr_scene_compose_backward_ex refuses; steps missing; a Gaussian-group gradient pointer; betas
 * outside [0, 1); a stepped group of a non-empty segment without v or without its parameter pointer.
 * Nothing synchronises with the host and nothing is allocated beyond the scratch callback (tables and partials). */
int sgr_scene_compose_backward_step(int K, const sgr_scene_segment* segs, const sgr_scene_step* steps,
                                    const sgr_scene_segment_grads* grads, int M, int S, const float* dL_dmeans3D,
                                    const float* dL_drotations, const float* dL_dscales, const float* dL_dopacities,
                                    const float* dL_dshs, const float* dL_dsemantics, const sgr_scene_frame* frame,
                                    double beta1, double beta2, float eps, sgr_alloc_fn scratch, void* scratch_user,
                                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
