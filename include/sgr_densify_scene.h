/* sgr_densify_scene.h -- C ABI of density control for a whole flat scene in one pass.
 *
 * StreetGaussianModel.densify_and_prune of the reference (lib/models/street_gaussian_model.py:573-586) loops over its
 * models and calls each model's own densify_and_prune: GaussianModel's (gaussian_model.py:522-553, SGR_PRUNE_BASE),
 * GaussianModelBkgd's (gaussian_model_bkgd.py:74-114, SGR_PRUNE_BKGD) or GaussianModelActor's
 * (gaussian_model_actor.py:204-261, SGR_PRUNE_ACTOR).  include/sgr_densify.h is one such call.  Every decision is per
 * row and depends on the row's own model's thresholds only, so here the models' rows are ONE flat array (the layout of
 * scene.FlatScene: the models' blocks behind each other) and the whole scene is planned, laid out and gathered once:
 * two host waits and a number of launches that does not depend on the number of models.
 *
 * LAYOUT CONTRACT.  Segment s covers the flat rows [start, start + count); the segments are sorted, do not overlap and
 * cover [0, N); count == 0 is legal.  Block s of the result is bit for bit what the per-model calls of
 * include/sgr_densify.h return for segment s with its own parameters (the kernels of both paths call the same device
 * functions, csrc/sgr_densify_rules.h):
 *   - rows inside a block in the reference's order: kept originals ascending, then clones ascending, then split
 *     children copy-major; blocks follow each other in segment order;
 *   - the candidates (every kept original, clone and split child, BEFORE pruning: the plan always defers the prune, whose
 *     predicate on a candidate's own row is the one the undeferred plan applies to its source row) are laid out the
 *     same way, block s at row cand_base[s];
 *   - `normals` [sum_s n_split * points_split_s, 3] is the concatenation of the segments' blocks, segment s at row
 *     normals_base[s]; sample_row of a split child already includes normals_base[s];
 *   - `box_normals` [sum n_cand_s, 2, 3] is the concatenation, over the segments with SGR_PRUNE_ACTOR and prune_big, of
 *     one [n_cand_s, 2, 3] block each, segment s at candidate row box_base[s];
 *   - moments of new rows are zero (sgr_densify_gather's zero_new).
 * The bases follow from the per-segment totals of the first read-back: sgr_densify_scene_layout, host only.
 * n_split is one value for the whole scene (sgr_densify_split_children takes one).
 *
 * SEQUENCE.  sgr_densify_scene_plan (read-back 1) -> sgr_densify_scene_layout -> sgr_densify_scene_map ->
 * sgr_densify_gather of xyz / scaling / rotation / opacity + sgr_densify_split_children (src indexes flat rows, so
 * they work as they are) -> sgr_densify_scene_prune (read-back 2) -> sgr_densify_gather per uniform-width array and
 * sgr_densify_scene_gather_ragged for features_dc / semantic, whose row width differs per segment.
 * All pointers are DEVICE pointers unless marked host. */
#ifndef SGR_DENSIFY_SCENE_H
#define SGR_DENSIFY_SCENE_H
#include <stddef.h>
#include <stdint.h>
#include "sgr_densify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGR_DENSIFY_SCENE_MAX_SEGMENTS 1024 /* the kernels stage the segments' row starts in LDS */

/* One model of the scene.  The table is passed twice: a host copy (argument checks, before any HIP call) and a device
 * copy the launches read. */
typedef struct sgr_densify_scene_segment {
    int32_t start, count;          /* first flat row, rows */
    int32_t dc_width, sem_width;   /* floats per row of features_dc (3 * fourier_dim) and of semantic (0 allowed) */
    int64_t dc_offset, sem_offset; /* element offset of the segment's block in the flat features_dc / semantic array */
    sgr_densify_params params;     /* defer_prune is ignored */
    int32_t variant;               /* SGR_PRUNE_* */
    float sphere[4];               /* SGR_PRUNE_BKGD: {cx, cy, cz, radius}; a NaN radius = missing */
    float box[6];                  /* SGR_PRUNE_ACTOR with prune_big: {min xyz, max xyz}; NaN = missing */
} sgr_densify_scene_segment;

size_t sgr_densify_scene_work_bytes(int n, int nseg);

/* Flags of all N rows with each row's own segment's parameters, the four mask scans over the whole scene; a segment's
 * totals are differences of the scans at its ends.  totals (host, [nseg, 4], written before the call returns; the call
 * synchronises the stream): per segment {kept originals, clones, split points, split points with children} -- with the
 * prune deferred the first is count - split points and the last equals the third.
 * work: sgr_densify_scene_work_bytes(N, nseg) bytes, kept until the last call of the sequence. */
int sgr_densify_scene_plan(int N, int nseg, const sgr_densify_scene_segment* segs_host,
                           const sgr_densify_scene_segment* segs, const float* xyz_gradient_accum, const float* denom,
                           const float* scaling, const float* opacity, char* work, int64_t* totals, void* stream);

/* Host only, no HIP call.  layout (host, [nseg + 1, 3]): per segment {cand_base, normals_base, box_base} as rows of the
 * candidate arrays, of `normals` and of `box_normals`; row nseg holds the three sizes.  n_cand_s = totals[s][0] +
 * totals[s][1] + n_split * totals[s][3].  SGR_E_INVALID when the candidates exceed 2^31 - 1 rows. */
int sgr_densify_scene_layout(int nseg, const sgr_densify_scene_segment* segs_host, const int64_t* totals, int64_t* layout);

/* src / kind / sample_row of every candidate row (n_cand = layout[nseg][0] entries each), as sgr_densify_map writes
 * them for one model: src = the FLAT source row. */
int sgr_densify_scene_map(int N, int nseg, const sgr_densify_scene_segment* segs_host, const sgr_densify_scene_segment* segs,
                          const char* work, int32_t* src, uint8_t* kind, int32_t* sample_row, void* stream);

/* Every candidate against its own segment's prune rule, then the compaction of the survivors:
 * sel[0 .. n_out) = ascending candidate rows that stay, src_out / kind_out = src / kind of those rows (arrays of n_cand
 * entries; n_out = the sum of the segments' survivors).  counts (host, [nseg, 5], written before the call returns; the call
 * synchronises the stream): per segment {below min opacity, big in world space, outside the tracking box, pruned,
 * survivors = rows of the segment's block of the result}.
 * cand_work: sgr_densify_scene_work_bytes(n_cand, nseg) bytes; work: the plan's. */
int sgr_densify_scene_prune(int n_cand, int nseg, const sgr_densify_scene_segment* segs_host,
                            const sgr_densify_scene_segment* segs, const float* xyz, const float* scaling,
                            const float* rotation, const float* opacity, const float* box_normals, const int32_t* src,
                            const uint8_t* kind, char* work, char* cand_work, int32_t* sel, int32_t* src_out,
                            uint8_t* kind_out, int64_t* counts, void* stream);

/* Row gather of features_dc (which = 0) or semantic (which = 1): result block s holds rows of the segment's own width,
 * the blocks packed behind each other.  out row r of block s = in row src[r] of block s; with zero_new, rows whose
 * kind != KEEP are zero-filled (src / kind = src_out / kind_out of sgr_densify_scene_prune).  One launch for all
 * segments.  new_counts (host, [nseg]) = the survivors per segment that call returned. */
int sgr_densify_scene_gather_ragged(int nseg, const sgr_densify_scene_segment* segs_host,
                                    const sgr_densify_scene_segment* segs, const int64_t* new_counts, const char* work,
                                    int which, const float* in, const int32_t* src, const uint8_t* kind, int zero_new,
                                    float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
