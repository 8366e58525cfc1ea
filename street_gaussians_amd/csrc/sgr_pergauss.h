// sgr_pergauss.h -- the steps the per-Gaussian kernels share (preprocess + duplicate: sgr_preprocess.hip, per-Gaussian
// backward: sgr_gauss_bwd.hip and its strict twin, view-sharded exchange: sgr_multiview.hip), one text per step: the view
// direction, the SH row -> RGB fold with its bias / clamp, the clamp-masked colour gradient, the packed tile rect word and
// the decisions made on it, the densification-statistics sink, the scale + rotation load and the copy of a wave's SH rows
// through LDS.  __host__ __device__ inline functions like sgr_math.h and sgr_quat.h, so tests/host_math runs the same
// text on the CPU (tests/test_host_math.py, tests/test_pergauss_host_cpu.py); the LDS copies at the end are device-only.
//
// Contraction: f<true> evaluates operation by operation, f<> takes the state of the including translation unit
// (SGR_FP_FLAVOURS, sgr_common.h) -- contracted in sgr_gauss_bwd.hip and sgr_multiview.hip, op by op in
// sgr_gauss_bwd_strict.hip through its file pragma.  The colour fold is part of the preprocess's op-by-op contract
// (strict mode promises the reference's colour bits) and has that one flavour only.
#pragma once
#include "sgr_math.h"

// ---- view direction: dir_orig = mean - campos, dir = dir_orig / |dir_orig| (forward.cu:28-29, backward.cu:50-53) ----
template <bool NC = false>
SGR_HD void sgr_view_dir(const float* p, const float* campos, float* dir_orig, float* dir) {
    SGR_FP_FLAVOURS(
        _Pragma("unroll") for (int i = 0; i < 3; i++) dir_orig[i] = p[i] - campos[i];
        const float len = sqrtf(dir_orig[0] * dir_orig[0] + dir_orig[1] * dir_orig[1] + dir_orig[2] * dir_orig[2]);
        _Pragma("unroll") for (int i = 0; i < 3; i++) dir[i] = dir_orig[i] / len;)
}

// ---- SH row -> RGB (forward.cu:20-71), op by op ----
// One step of the fold: channel ch of coefficient k (element 3 k + ch of the row); coefficient 0 assigns.
SGR_HD void sgr_sh_fold1(int k, int ch, float v, const float* Y, float* rgb) {
#pragma clang fp contract(off)
    rgb[ch] = (k == 0) ? Y[0] * v : rgb[ch] + Y[k] * v;
}
// float4 number i of a row (e4 = its four floats): the elements below coefficient ncoef, in ascending order
SGR_HD void sgr_sh_fold4(int i, const float* e4, const float* Y, int ncoef, float* rgb) {
#pragma unroll
    for (int j = 0; j < 4; j++)
        if ((4 * i + j) / 3 < ncoef) sgr_sh_fold1((4 * i + j) / 3, (4 * i + j) % 3, e4[j], Y, rgb);
}
// a whole row, coefficient by coefficient (rows that are not 16-byte aligned; the host harness)
SGR_HD void sgr_sh_fold_row(const float* sh, const float* Y, int ncoef, float* rgb) {
    for (int k = 0; k < ncoef; k++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) sgr_sh_fold1(k, ch, sh[3 * k + ch], Y, rgb);
}
// + 0.5, clamp at zero; clamped = 3-bit mask of the channels the clamp held (forward.cu:64-70)
SGR_HD void sgr_sh_finish(float* rgb, uint32_t& clamped) {
    clamped = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        rgb[ch] += 0.5f;
        clamped |= rgb[ch] < 0 ? 1u << ch : 0u;
        rgb[ch] = fmaxf(rgb[ch], 0.0f);
    }
}
// the colour gradient that reaches the SH coefficients: none for a channel the forward clamped (backward.cu:40-44)
SGR_HD float sgr_mask_clamped1(uint32_t cl, int ch, float g) { return ((cl >> ch) & 1u) ? 0.f : g; }
SGR_HD void sgr_mask_clamped(uint32_t cl, const float* g, float* out) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) out[ch] = sgr_mask_clamped1(cl, ch, g[ch]);
}

// ---- scale + rotation of one Gaussian (the rotation as one 16-byte load) ----
SGR_HD void sgr_load_scale_rot(const float* __restrict__ scales, const float* __restrict__ rotations, int idx, float* sc,
                               float* rot) {
    sc[0] = scales[3 * idx]; sc[1] = scales[3 * idx + 1]; sc[2] = scales[3 * idx + 2];
    const float4 q = *reinterpret_cast<const float4*>(rotations + 4 * (size_t)idx);
    rot[0] = q.x; rot[1] = q.y; rot[2] = q.z; rot[3] = q.w;
}

// ---- packed tile rect word: x0 | y0 << 10 | w << 20, bit 31 = SGR_RECT_MASKED (SgrGeomView::aux) ----
struct SgrRect { uint32_t x0, y0, w; bool masked; };
SGR_HD uint32_t sgr_pack_rect(uint32_t x0, uint32_t y0, uint32_t w) { return x0 | (y0 << 10) | (w << 20); }
SGR_HD SgrRect sgr_unpack_rect(uint32_t r) {
    return SgrRect{r & 1023u, (r >> 10) & 1023u, (r >> 20) & 1023u, (r & SGR_RECT_MASKED) != 0u};
}
// tile of the centre coordinate c (pixels) along one axis, clamped into the tiles [lo, hi) of the rect
static_assert(SGR_BLOCK_X == SGR_BLOCK_Y, "square tiles");
SGR_HD float sgr_centre_tile(float c, uint32_t lo, uint32_t hi) {
    return fminf(fmaxf(floorf(c * (1.0f / SGR_BLOCK_X)), (float)lo), (float)(hi - 1));
}

// Tile rect of a Gaussian.  The reference takes the square of ceil(3 sigma_max) pixels around the centre
// (auxiliary.h:46-57 getRect) and so emits a (tile, Gaussian) instance for many tiles in which the Gaussian cannot pass
// the alpha >= 1/255 test of the blend (forward.cu:428-430): low opacity, anisotropy.  Those instances change nothing in
// any output (the blend skips them) but are duplicated, sorted, staged and given a partial-gradient row.  `tight`
// intersects the reference rect with the tiles of the box [px -+ hx] x [py -+ hy] outside of which alpha < 1/255
// (sgr_extent: conservative, the box the quadrant cull of the blend kernels has used since round 1): 0.72 of the
// reference's instances on the benchmark scene; every image bit-identical, the gradients equal up to the grouping of the
// row sum's additions (tests).  A Gaussian keeps at least one tile, so that "radius > 0" still implies "owns a row".
// tight > 1: inside that rect only the tiles the alpha >= 1/255 ellipse reaches (the rect is its bounding box: the
// corners go): a 64-bit tile mask for rects of up to 64 tiles (sgr_math.h: sgr_tile_mask), bit 31 of the rect word says
// "masked".  duplicate emits the set tiles, the backward numbers a Gaussian's rows by the rank of the tile in the mask.
// 0.61 instead of 0.72 of the reference's instances on the benchmark scene.
// Returns the rect word, the number of tiles emitted for it and the mask (as computed: it is the Gaussian's tmask only when
// the word says "masked"; 0 where no mask was looked at).
struct SgrTightRect { uint32_t rect, nemit; uint64_t tmask; };
SGR_HD SgrTightRect sgr_tight_rect(const SgrProj& pr, float hx, float hy, float opacity, int tight) {
    uint32_t x0 = pr.rx0, x1 = pr.rx1, y0 = pr.ry0, y1 = pr.ry1;
    if (tight) {
        // pixel x of tile t: 16 t .. 16 t + 15; pixels that can pass lie in [px - hx, px + hx]  (NaN extents: fmaxf / fminf
        // return the other operand = the reference rect)
        const float inv = 1.0f / SGR_BLOCK_X;
        float fx0 = fmaxf(floorf((pr.px - hx) * inv), (float)x0), fx1 = fminf(floorf((pr.px + hx) * inv) + 1.0f, (float)x1);
        float fy0 = fmaxf(floorf((pr.py - hy) * inv), (float)y0), fy1 = fminf(floorf((pr.py + hy) * inv) + 1.0f, (float)y1);
        if (!(fx0 < fx1)) { fx0 = sgr_centre_tile(pr.px, x0, x1); fx1 = fx0 + 1.0f; }
        if (!(fy0 < fy1)) { fy0 = sgr_centre_tile(pr.py, y0, y1); fy1 = fy0 + 1.0f; }
        x0 = (uint32_t)fx0; x1 = (uint32_t)fx1; y0 = (uint32_t)fy0; y1 = (uint32_t)fy1;
    }
    const uint32_t w = x1 - x0, h = y1 - y0;
    SgrTightRect t{sgr_pack_rect(x0, y0, w), w * h, 0ull};
    if (tight > 1 && w >= 2u && h >= 2u && t.nemit <= 64u) {  // (a single row or column of tiles IS its bounding box)
        t.tmask = sgr_tile_mask(pr.px, pr.py, pr.con_x, pr.con_y, pr.con_z, opacity, x0, y0, x1, y1);
        if (t.tmask == 0) {  // reaches no tile (opacity below 1/255 ...): the centre's tile, so that the Gaussian owns a row
            const uint32_t cx = (uint32_t)sgr_centre_tile(pr.px, x0, x1), cy = (uint32_t)sgr_centre_tile(pr.py, y0, y1);
            t.tmask = 1ull << ((cy - y0) * w + (cx - x0));
        }
        const uint32_t cnt = (uint32_t)__builtin_popcountll(t.tmask);
        if (cnt != t.nemit) { t.rect |= SGR_RECT_MASKED; t.nemit = cnt; }
    }
    return t;
}

// The k-th tile emitted for a rect word (k < nemit), row-major over the rect or over the set bits of its mask: what the
// duplicate kernel writes into slot k of the Gaussian's range.  k / w with ONE reciprocal and an exact fix-up (k < 2^20), so
// rcp_w may be off by an ulp either way (the device passes v_rcp_f32).  `mask` is read for a masked word only.
SGR_HD uint2 sgr_slot_tile(uint32_t rect, const uint64_t& mask, uint32_t k, float rcp_w) {
    const SgrRect r = sgr_unpack_rect(rect);
    if (r.masked) k = sgr_select_bit(mask, k);  // the k-th tile of the mask, as an index into the rect
    uint32_t q = (uint32_t)((float)k * rcp_w);
    int rem = (int)k - (int)(q * r.w);
    if (rem < 0) { q--; rem += (int)r.w; }
    if (rem >= (int)r.w) { q++; rem -= (int)r.w; }
    return make_uint2(r.x0 + (uint32_t)rem, r.y0 + q);
}
// Its inverse: the partial-gradient row of instance (Gaussian g, tile (tx, ty)) = the Gaussian's first row + the rank of
// the tile among the tiles it is emitted for (its index inside the rect when there is no mask).
SGR_HD uint32_t sgr_row_of(uint32_t rect, uint32_t tx, uint32_t ty, const uint32_t* __restrict__ u0,
                           const uint64_t* __restrict__ tmask, uint32_t g) {
    const SgrRect r = sgr_unpack_rect(rect);
    uint32_t j = (ty - r.y0) * r.w + (tx - r.x0);
    if (r.masked) j = (uint32_t)__builtin_popcountll(tmask[g] & ((1ull << j) - 1ull));
    return u0[g] + j;
}
// Marked-list mode: is tile (tx, ty) of the reference's rect one of the live_n tiles emitted for the cut-down rect word?
// Inside the cut-down rect and, with a mask, one of its set tiles (index j inside that rect: below the number of its tiles
// without a mask -- which bounds the row -- or a set bit with one).
SGR_HD bool sgr_mark_live(uint32_t live_rect, const uint32_t& live_n, const uint64_t& mask, uint32_t tx, uint32_t ty) {
    const SgrRect l = sgr_unpack_rect(live_rect);
    const uint32_t dxl = tx - l.x0, dyl = ty - l.y0;  // (wrap around for tiles left of / above the rect: >= w / huge)
    const uint32_t j = dyl * l.w + dxl;
    const bool live = dxl < l.w && ty >= l.y0;
    if (l.masked) return live && j < 64u && ((mask >> (j & 63u)) & 1ull);
    return live && j < live_n;
}

// ---- densification statistics of one view (set_max_radii2D + add_densification_stats, street_gaussian_model.py:551-571) ----
// Persistent row of Gaussian idx: identity, or through the frame's segment map (binary search over the segment starts;
// kernel arguments -> scalar loads); -1: in no segment.
SGR_HD long sgr_stat_sink_row(const SgrStatSink& sink, int idx) {
    if (sink.nseg <= 0) return idx;
    int lo = 0, hi = sink.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sink.start[mid] <= idx) lo = mid; else hi = mid - 1;
    }
    return (idx >= sink.start[lo] && idx < sink.start[lo] + sink.count[lo]) ? (long)idx + sink.shift[lo] : -1;
}
// (gx, gy, gz) = dL/dmean2D of a Gaussian with radius r > 0
template <bool NC = false>
SGR_HD void sgr_stat_sink_add(const SgrStatSink& sink, long row, float gx, float gy, float gz, int r) {
    SGR_FP_FLAVOURS(sink.accum[2 * (size_t)row] += sqrtf(gx * gx + gy * gy);)  // norm of grad[:, :2]
    sink.accum[2 * (size_t)row + 1] += fabsf(gz);                               // norm of grad[:, 2:]
    sink.denom[row] += 1.0f;
    sink.max_radii[row] = fmaxf(sink.max_radii[row], (float)r);
}

// ---- a wave's 64 SH rows (M = 16: 12 float4 each) as ONE contiguous 12 KB block, through LDS with coalesced 1 KB transfers ----
// float4s of the rows of the wave whose first Gaussian is g0
__device__ __forceinline__ int sgr_wave_row4s(int P, int g0) { return max(0, min(64, P - g0)) * 12; }
// Half h of the block (rows 32 h .. 32 h + 31) into lds, the rows of the Gaussians in `vis` only; STRIDE = float4s between
// consecutive rows in LDS (12: packed; 13: the per-lane float4 reads of 16 consecutive rows fall on 16 disjoint 4-bank groups)
template <int STRIDE>
__device__ __forceinline__ void sgr_rows_to_lds(float4* lds, const float* __restrict__ rows, int P, int g0, int h, int lane,
                                                uint64_t vis) {
    const float4* src = reinterpret_cast<const float4*>(rows) + (size_t)g0 * 12;
    const int nrow4 = sgr_wave_row4s(P, g0);
#pragma unroll
    for (int it = 0; it < 6; it++) {
        const int f = h * 384 + it * 64 + lane, row = f / 12;
        if (f < nrow4 && ((vis >> row) & 1ull)) lds[f - h * 384 + (STRIDE - 12) * (row - 32 * h)] = src[f];
    }
}
// Block number h of ROWS packed rows (32: a half, 64: the whole wave) from lds back to the rows
template <int ROWS>
__device__ __forceinline__ void sgr_rows_from_lds(float* __restrict__ rows, const float4* lds, int P, int g0, int h, int lane) {
    float4* dst = reinterpret_cast<float4*>(rows) + (size_t)g0 * 12;
    const int nrow4 = sgr_wave_row4s(P, g0);
#pragma unroll
    for (int it = 0; it < ROWS * 12 / 64; it++) {
        const int f = h * ROWS * 12 + it * 64 + lane;
        if (f < nrow4) dst[f] = lds[f - h * ROWS * 12];
    }
}
