// sgr_loss_internal.h -- what sgr_loss.hip (the stand-alone image-space losses) and sgr_frame_loss.hip (all of them in one
// op) share: the SSIM steps (sgr_ssim.h), the tile grid, the block reduction, the per-pixel arithmetic of the accumulation
// and LiDAR terms, and the LiDAR term's radix select, whose kernels live in sgr_loss.hip behind sgr_lidar_select_launch.
#pragma once
#include <math.h>

#include "../../include/sgr.h"
#include "sgr_common.h"
#include "sgr_ssim.h"

static inline dim3 tile_grid(int C, int H, int W) {
    return dim3((W + SGR_LS_T - 1) / SGR_LS_T, (H + SGR_LS_T - 1) / SGR_LS_T, C);
}

// ---- LiDAR depth term: work area of the selection (train.py:124-131) ------------------------------------------------
struct LdWork {
    uint32_t* key;    // [n] float bits of the error (>= 0, so unsigned order == float order); 0xffffffff = not selected
    uint32_t* hist;   // [4][256]
    uint32_t* state;  // [0] count  [1] k  [2] prefix  [3] k remaining  [4] count below threshold  [5] ties
    float* sums;      // [SGR_L1_BLOCKS]
};
#define SGR_L1_BLOCKS 1024  // workgroups of every grid-stride reduction of the family
static inline LdWork ld_carve(char* base, size_t n) {
    LdWork w;
    char* p = base;
    sgr_carve(p, w.key, n ? n : 1);
    sgr_carve(p, w.hist, 4 * 256);
    sgr_carve(p, w.state, 16);
    sgr_carve(p, w.sums, SGR_L1_BLOCKS);
    return w;
}
static inline size_t ld_work_bytes(size_t n) {
    char* base = (char*)4096;
    LdWork w = ld_carve(base, n ? n : 1);
    return (size_t)((char*)(w.sums + SGR_L1_BLOCKS) - base) + 512;
}

#ifdef __HIPCC__
// The selection over n keys that are already in w.key, with their count in w.state[0] and w.hist zeroed: k = int(keep *
// count) in double, a 4-pass radix select of the k-th smallest key, the sum of the keys below it, then out[0] = loss,
// out[1] = k, out[2] = threshold, out[3] = weight of the errors equal to the threshold (sgr_loss.h).  Defined in sgr_loss.hip.
void sgr_lidar_select_launch(int n, const LdWork& w, double keep, float* out, hipStream_t stream);

static inline int ls_check_dims(int C, int H, int W) {
    return (C <= 0 || H <= 0 || W <= 0) ? sgr_set_error(SGR_E_INVALID, "C, H, W must be positive") : 0;
}
// sum of a 256-lane workgroup (float, or a count): each wave's sum to lds4[wave]; after a barrier, the four in a fixed order
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {  // own function: inside wave_sums_to_lds it moves the reducers' instructions
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ void wave_sums_to_lds(T v, T* lds4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
}
template <typename T>
__device__ __forceinline__ T lds4_total(const T* lds4) { return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3]; }
__device__ __forceinline__ float block_sum_256(float v, float* lds4) {
    wave_sums_to_lds(v, lds4);
    __syncthreads();
    return lds4_total(lds4);
}

// ---- accumulation terms (train.py:106-121); mode: SGR_BCE_SKY 0, SGR_BCE_OBJECT 1 -------------------------------------
__device__ __forceinline__ float bce_clamp(float acc) {  // torch.clamp(acc, min=1e-6, max=1.-1e-6)
    return fminf(fmaxf(acc, 1e-6f), 1.0f - 1e-6f);
}
__device__ __forceinline__ float bce_term(int mode, float a, bool m) {
    if (mode == 0) return m ? -logf(1.0f - a) : -logf(a);
    return m ? -(a * logf(a) + (1.0f - a) * logf(1.0f - a)) : -logf(1.0f - a);
}
// torch.clamp's backward passes the gradient on [min, max]: elsewhere d(term)/dacc is zero
__device__ __forceinline__ bool bce_clamp_passes(float x) { return x >= 1e-6f && x <= 1.0f - 1e-6f; }
// d(term)/dacc at an acc x that the clamp passes
__device__ __forceinline__ float bce_grad(int mode, float x, bool m) {
    if (mode == 0) return m ? 1.0f / (1.0f - x) : -1.0f / x;
    return m ? (logf(1.0f - x) - logf(x)) : 1.0f / (1.0f - x);
}

// ---- LiDAR depth term, per pixel ---------------------------------------------------------------------------------------
// key of a pixel of depth_mask = (lidar_depth > 0) & mask: the bits of |depth / (acc + 1e-10) - lidar|
__device__ __forceinline__ uint32_t lidar_key(float depth, float acc, float l) {
    const float e = fabsf(depth / (acc + 1e-10f) - l);
    return (e == e) ? __float_as_uint(e) : 0x7fc00000u;  // NaN sorts last among the selected, like topk
}
// gradient of the term to one pixel's depth and acc; out = {loss, k, threshold, tie weight}, up = the term's upstream
__device__ __forceinline__ void lidar_grad(uint32_t key, const float* __restrict__ out, float depth, float acc, float l,
                                           float up, float& gd, float& ga) {
    const uint32_t t = __float_as_uint(out[2]);
    float wgt = 0.f;
    if (out[1] > 0.f && key != 0xffffffffu) wgt = key < t ? 1.0f : (key == t ? out[3] : 0.f);
    gd = 0.f;
    ga = 0.f;
    if (wgt > 0.f) {
        const float den = acc + 1e-10f, diff = depth / den - l;
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);  // not l1_sign(): the call moves the up * wgt multiply
        const float g = up * wgt * sgn / out[1];
        gd = g / den;
        ga = -g * depth / (den * den);
    }
}
#endif
