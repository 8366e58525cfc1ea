// sgr_launch.h -- every launcher that one translation unit defines and sgr_api.hip calls, declared HERE only and included by
// the defining file too: a definition that drifts from its declaration is another overload, the declared one stays undefined,
// and the link (-Wl,-z,defs) fails -- not the first call on a GPU.  (The scan and sort primitives: sgr_common.h, same rule.)
// Arguments that come in groups travel as host structs filled by name; the launchers unpack them -- no kernel takes one.
#pragma once
#include "../../include/sgr.h"
#include "sgr_math.h"

// The tile lists of a frame, as every tile kernel walks them.
struct SgrTileLists {
    int gx = 0, gy = 0;  // tile grid.  gy < 0: |gy| rows, walked in the FRAME's order (the flag word behind the ranges, sgr_wg_tile)
    int W = 0, H = 0;
    const uint2* ranges = nullptr;
    const uint32_t* point_list = nullptr;  // the final instance list
    const float4* rec = nullptr;
    // workgroups of a tile kernel: the supertile-ordered grid incl. padding blocks; 0 = nothing to launch
    unsigned blocks() const { return (gx <= 0 || gy == 0) ? 0u : sgr_xcd_grid_blocks(gx, gy < 0 ? -gy : gy); }
};
// f(std::true_type{}) or f(std::false_type{}): the kernel instantiation of a run-time flag
template <typename F> static inline void sgr_with_flag(bool on, F&& f) { if (on) f(std::true_type{}); else f(std::false_type{}); }

// sgr_preprocess.hip
void sgr_launch_mark_visible(int P, const float* means3D, const float* viewmatrix, uint8_t* present, hipStream_t s);
void sgr_launch_preprocess(int P, int D, int M, const float* means3D, const float* scales, const float* rotations,
                           const float* opacities, const float* shs, const float* cov3D_precomp, const float* colors_precomp,
                           const SgrCam* cam, const SgrGeomView& gv, int* radii, int prefiltered, bool stage_sh, int tight,
                           bool want_jac, hipStream_t s);
void sgr_launch_filter(int P, const float* means3D, const float* scales, const float* rotations, const float* cov3D_precomp,
                       const SgrCamArgs& ca, const SgrGeomView& gv, int* radii, float* means2D, int prefiltered, hipStream_t s);
void sgr_launch_duplicate(int P, const SgrGeomView& gv, const uint32_t* order, const uint32_t* bsum, const uint32_t* sub, void* keys,
                          int key16, uint32_t* vals, int gx, uint32_t cap, int marks, hipStream_t s);
void sgr_launch_tile_ranges(int L, const void* keys, int key16, uint2* ranges, uint8_t* touched, uint32_t T, hipStream_t s);
void sgr_launch_tile_order(const uint2* ranges, int T, int force, hipStream_t s);
void sgr_launch_compose_keys(int L, const void* tile_keys, int key16, const uint32_t* point_list, const float4* rec, uint64_t* out,
                             hipStream_t s);
// sgr_blend_fwd.hip, sgr_blend_layers.hip, sgr_object_alpha.hip.  S must be <= SGR_SEM_MAX (checked by the caller).
void sgr_launch_blend_fwd(bool cull, bool exact, const SgrTileLists& tl, int S, const float* semantics, const float* bg,
                          float* out_color, float* out_depth, float* out_alpha, float* out_semantic, uint32_t* n_contrib,
                          uint8_t* hit4, uint32_t* hlist, uint32_t* n_contrib_k, hipStream_t s);
void sgr_launch_blend_layers(bool exact, const SgrTileLists& tl, int split, int P, const float* bg, int clamp,
                             float* const color[2], float* const alpha[2], hipStream_t s);
void sgr_launch_layers_fill(int W, int H, const float* bg, int clamp, float* const color[2], float* const alpha[2], hipStream_t s);
void sgr_launch_object_alpha_fwd(bool exact, const SgrTileLists& tl, int split, float* out_alpha, uint32_t* out_last, hipStream_t s);
// row_stride: sgr_partial_row_stride(0) = 12 floats (three float4 stores per row)
void sgr_launch_object_alpha_bwd(bool exact, const SgrTileLists& tl, const uint32_t* u0, const uint64_t* tmask, int split,
                                 const float* layer_alpha, const uint32_t* layer_last, const float* dL_dlayer_alpha,
                                 float* partials, int row_stride, uint8_t* touched, uint32_t row_limit, hipStream_t s);

// sgr_blend_bwd.hip (and variants/sgr_blend_bwd_sw.hip, which reads the fields its S = 0 kernel has a parameter for)
int sgr_partial_row_stride(int S);
struct SgrBlendBwdArgs {
    bool cull = true, dpp = true, det = true;  // quadrant cull, DPP wave reduction, deterministic LDS combine
    bool v2 = false, exact = false;            // variant builds: transposed S = 0 accumulation; parity mode
    int S = 0;
    const float *bg = nullptr, *semantics = nullptr, *alphas = nullptr;
    const uint64_t* tmask = nullptr;
    const uint32_t *u0 = nullptr, *n_contrib = nullptr, *n_contrib_k = nullptr;
    const uint8_t* hit4 = nullptr;    // nullptr: the kernel redoes the geometric cull
    const uint32_t* hlist = nullptr;  // nullptr: the positional walk
    const uint32_t* hl_flag = nullptr;  // the frame's "hit list written" header word
    const float *dL_dpix = nullptr, *dL_ddepth = nullptr, *dL_dalpha = nullptr, *dL_dsem = nullptr;
    float* partials = nullptr;
    uint8_t* touched = nullptr;  // one byte per row: written by this backward
    uint32_t row_limit = 0;
};
void sgr_launch_blend_bwd(const SgrTileLists& tl, const SgrBlendBwdArgs& a, hipStream_t s);
void sgr_launch_blend_bwd_sw(const SgrTileLists& tl, const SgrBlendBwdArgs& a, int row_stride, hipStream_t s);

// sgr_gauss_bwd.hip: the row sum + the per-Gaussian stage.  A default means "not asked for".
struct SgrGaussBwdArgs {
    int P = 0, D = 0, M = 0, S = 0;
    const float *means3D = nullptr, *shs = nullptr, *scales = nullptr, *rotations = nullptr, *cov3D_precomp = nullptr;
    const int* radii = nullptr;
    const SgrCam* cam = nullptr;
    SgrGeomView gv = {};
    const float* partials = nullptr;
    int row_stride = 0, W = 0, H = 0;
    const uint8_t* touched = nullptr;
    float4* cd = nullptr;
    float *dL_dmean2D = nullptr, *dL_dopacity = nullptr, *dL_dcolor = nullptr, *dL_dmean3D = nullptr, *dL_dcov3D = nullptr,
          *dL_dsh = nullptr, *dL_dscale = nullptr, *dL_drot = nullptr, *dL_dsemantic = nullptr;
    SgrStatSink sink;                 // the statistics sink (empty: none)
    int quad = 0;                     // variant builds: the rows are the scalar walk's four per instance
    int exact = 0, rs_wave = 0;       // parity mode; variant builds: the wave-cooperative row sum
    hipEvent_t after_rows = nullptr;  // recorded once dL/dmean2D, dL/dopacity and dL/dcolour are final
    uint32_t row_limit = 0;
    float* masked_color_out = nullptr;
    int skip_sh = 0, skip_cov = 0;    // nobody receives dL/dSH / dL/dcov3D
};
// Returns non-zero when `after_rows` could not be recorded (everything is launched regardless).  _strict: the same source with
// FP contraction off (sgr_gauss_bwd_strict.hip renames the launcher with a #define: this then declares the strict one twice).
typedef int SgrGaussBwdLauncher(const SgrGaussBwdArgs& a, hipStream_t s);
SgrGaussBwdLauncher sgr_launch_gauss_bwd, sgr_launch_gauss_bwd_strict;
// sgr_multiview.hip
void sgr_launch_masked_color_grad(int P, const uint32_t* clamped, const float* dL_dcolor, float* out, hipStream_t s);
void sgr_launch_sh_grad_from_views(int P, int D, int M, int V, const float* means3D, size_t means_stride, const float* campos,
                                   size_t campos_stride, const float* drgb, size_t drgb_stride, float* dL_dsh, hipStream_t s);
// self-tests (sgr_blend_bwd.hip, sgr_tile_sort.hip); sgr_knn.hip
void sgr_launch_wave_sum_test(const float* in, float* out_dpp, float* out_shfl, int nwaves, hipStream_t s);
void sgr_launch_lds_atomic_order_test(const uint32_t* pattern, uint32_t* out, int trials, hipStream_t s);
int sgr_knn_impl(int P, const float* points, float* meanDists, sgr_alloc_fn scratch, void* scratch_user, hipStream_t s,
                 std::string& err);
