// sgr_sky.hip -- the fused sky composite and colour correction (include/sgr_sky.h) on gfx950.
//
// Forward, four launches and no host round trip:
//   1. flag    one lane per pixel: the mask rule, 0 / 1 per pixel
//   2. scan    sgr_launch_scan, inclusive and in place: flag[p] becomes the number of mask pixels up to p, and the total
//              (the count) is written to the device -- a mask pixel's compacted position is flag[p] - 1, the row-major
//              order of the reference's rays_d[mask]
//   3. fused   one lane per pixel: ray, lookup (mask pixels only), fill, composite, colour correction, clamp; writes
//              [3, H, W] directly.  A mask pixel also writes its ray and its unclamped sky value at its compacted position.
// Saved for the backward: the scanned flags (4 B / pixel), the count, and per MASK pixel the ray and the raw sky value
// (24 B).  Recomputing the sky in the backward instead would read the ray (12 B) plus the four texel taps (>= 48 B of
// gathers) per mask pixel, against 12 B to read the saved value; the ray is needed anyway, by the texture backward's key
// and record stages.
// Backward:
//   4. pixel   one lane per pixel: dL/drgb, dL/dacc, the texture upstream of the mask pixels at their compacted
//              positions, and per-block partials of the 12 sums of dL/daffine (fixed shuffle tree)
//   5. affine  one block: the partials summed in double in a fixed order
//   6. cube    the texture backward (sgr_texture_cube_backward_impl) on the compacted rays and upstreams, with the count
//              read on the device: the sort never touches the non-sky pixels.
// With the cube map's own optimiser (include/sgr_sky_step.h) stage 6 stops before its gather and leaves the sorted
// records in a workspace (sgr_sky_backward_deferred); the gather then happens inside the Adam step, per texel of the
// blocks that have ever been touched (sgr_sky_adam_step; the kernel is sgr_texture.hip's).
#include <string>

#include "../../include/sgr_sky.h"
#include "../../include/sgr_sky_step.h"
#include "../../include/sgr_texture.h"
#include "sgr_common.h"
#include "sgr_cube.h"

namespace {

// the camera of the ray contract: K^-1 (closed form in double, rounded once), R, T, and the origin o = -R^T T
struct SkyCam {
    float ki[9], r[9], t[3], o[3];
};

__device__ __forceinline__ void sky_camera(const float* __restrict__ K, const float* __restrict__ w2c, SkyCam& c) {
#pragma clang fp contract(off)
    double a[9];
#pragma unroll
    for (int i = 0; i < 9; i++) a[i] = (double)K[i];
    const double c0 = a[4] * a[8] - a[5] * a[7], c3 = a[5] * a[6] - a[3] * a[8], c6 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c3 + a[2] * c6;
    const double adj[9] = {c0, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                           c3, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                           c6, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
#pragma unroll
    for (int i = 0; i < 9; i++) c.ki[i] = (float)(adj[i] / det);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) c.r[3 * i + j] = w2c[4 * i + j];
        c.t[i] = w2c[4 * i + 3];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) c.o[j] = -((c.r[j] * c.t[0] + c.r[3 + j] * c.t[1]) + c.r[6 + j] * c.t[2]);
}

// the unit ray through (x + px, y + py): get_rays_torch's operation order (include/sgr_sky.h)
__device__ __forceinline__ void sky_ray(const SkyCam& c, float X, float Y, float d[3]) {
#pragma clang fp contract(off)
    float pc[3], pw[3];
#pragma unroll
    for (int i = 0; i < 3; i++) pc[i] = (X * c.ki[3 * i] + Y * c.ki[3 * i + 1]) + 1.f * c.ki[3 * i + 2];
    const float q0 = pc[0] - c.t[0], q1 = pc[1] - c.t[1], q2 = pc[2] - c.t[2];
#pragma unroll
    for (int j = 0; j < 3; j++) pw[j] = (q0 * c.r[j] + q1 * c.r[3 + j]) + q2 * c.r[6 + j];
#pragma unroll
    for (int j = 0; j < 3; j++) d[j] = pw[j] - c.o[j];
    const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int j = 0; j < 3; j++) d[j] = d[j] / nrm;
}

__device__ __forceinline__ void sky_pixel_xy(int64_t p, int W, const float* __restrict__ px, const float* __restrict__ py,
                                             bool train, float& X, float& Y) {
#pragma clang fp contract(off)
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    X = (float)x + (train ? px[p] : 0.5f);
    Y = (float)y + (train ? py[p] : 0.5f);
}

// torch.clamp(v, 0, 1): NaN stays NaN
__device__ __forceinline__ float sky_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
__device__ __forceinline__ bool sky_passes(float v) { return v >= 0.f && v <= 1.f; }

struct SkyArgs {
    int H, W, R;
    int64_t HW;
    int flags;
    const float *rgb, *acc, *cube, *K, *w2c, *px, *py, *affine;
    const uint8_t* sky_mask;
};

struct SkySaved {
    uint32_t *flag, *count, *scan_tmp;
    float *rays, *sky;  // compacted: [count, 3]
};

SkySaved carve_saved(char* base, int64_t HW, char** end = nullptr) {
    SkySaved v;
    char* p = base;
    const size_t n = (size_t)HW;
    sgr_carve(p, v.flag, n);
    sgr_carve(p, v.count, 64);
    sgr_carve(p, v.scan_tmp, sgr_scan_tmp_count(n));
    sgr_carve(p, v.rays, 3 * n);
    sgr_carve(p, v.sky, 3 * n);
    if (end) *end = p;
    return v;
}

constexpr int kBlock = 256;

struct SkyScratch {
    float *up, *part;
    void* tex_work;
};

SkyScratch carve_scratch(char* base, int64_t HW, size_t tex_bytes, char** end = nullptr) {
    SkyScratch v;
    char* p = base;
    const size_t n = (size_t)HW;
    sgr_carve(p, v.up, 3 * n);
    sgr_carve(p, v.part, 12 * ((n + kBlock - 1) / kBlock));
    char* tw;
    sgr_carve(p, tw, tex_bytes);
    v.tex_work = tw;
    if (end) *end = p;
    return v;
}

unsigned blocks(uint64_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

}  // namespace

// ---- forward --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sgr_sky_flag_kernel(SkyArgs a, uint32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.HW) return;
    bool m;
    if ((a.flags & SGR_SKY_TRAIN) && a.sky_mask) m = p < 50 * (int64_t)a.W || a.sky_mask[p] != 0;
    else m = (1.f - a.acc[p]) > 1e-3f;
    flag[p] = m ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
sgr_sky_fwd_kernel(SkyArgs a, SgrCubeSeam sm, const uint32_t* __restrict__ incl, float* __restrict__ rays,
                   float* __restrict__ skyc, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.HW) return;
    const uint32_t hi = incl[p], lo = p ? incl[p - 1] : 0u;
    const float fill = (a.flags & SGR_SKY_WHITE) ? 1.f : 0.f;
    float s[3] = {fill, fill, fill};
    if (hi != lo) {  // a mask pixel, compacted position lo
        SkyCam cam;
        sky_camera(a.K, a.w2c, cam);
        float X, Y, d[3], raw[3];
        sky_pixel_xy(p, a.W, a.px, a.py, (a.flags & SGR_SKY_TRAIN) != 0, X, Y);
        sky_ray(cam, X, Y, d);
        tx_lookup<3>(a.cube, a.R, 3, sm, d[0], d[1], d[2], raw);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            rays[3 * (size_t)lo + ch] = d[ch];
            skyc[3 * (size_t)lo + ch] = raw[ch];
            s[ch] = sky_clamp01(raw[ch]);
        }
    }
    const float oma = 1.f - a.acc[p];
    float c[3], o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) c[ch] = a.rgb[ch * a.HW + p] + s[ch] * oma;
    if (a.affine) {
        const float* A = a.affine;
#pragma unroll
        for (int i = 0; i < 3; i++) o[i] = ((A[4 * i] * c[0] + A[4 * i + 1] * c[1]) + A[4 * i + 2] * c[2]) + A[4 * i + 3];
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) o[i] = c[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) out[i * a.HW + p] = (a.flags & SGR_SKY_CLAMP) ? sky_clamp01(o[i]) : o[i];
}

__global__ void __launch_bounds__(256) sgr_sky_rays_kernel(SkyArgs a, float* __restrict__ rays, float* __restrict__ kinv) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.HW) return;
    SkyCam cam;
    sky_camera(a.K, a.w2c, cam);
    if (p == 0)
        for (int i = 0; i < 9; i++) kinv[i] = cam.ki[i];
    float X, Y, d[3];
    sky_pixel_xy(p, a.W, a.px, a.py, (a.flags & SGR_SKY_TRAIN) != 0, X, Y);
    sky_ray(cam, X, Y, d);
    for (int ch = 0; ch < 3; ch++) rays[3 * p + ch] = d[ch];
}

// ---- backward -------------------------------------------------------------------------------------------------------
template <bool AFF>
__global__ void __launch_bounds__(256)
sgr_sky_bwd_kernel(SkyArgs a, const float* __restrict__ g, const uint32_t* __restrict__ incl, const float* __restrict__ skyc,
                   float* __restrict__ drgb, float* __restrict__ dacc, float* __restrict__ up, float* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ float red[4][12];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    float sums[12];
#pragma unroll
    for (int k = 0; k < 12; k++) sums[k] = 0.f;
    if (p < a.HW) {
        const uint32_t hi = incl[p], lo = p ? incl[p - 1] : 0u;
        const bool m = hi != lo;
        const float fill = (a.flags & SGR_SKY_WHITE) ? 1.f : 0.f;
        float raw[3], s[3], c[3], gp[3], dc[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            raw[ch] = m ? skyc[3 * (size_t)lo + ch] : fill;
            s[ch] = m ? sky_clamp01(raw[ch]) : fill;
        }
        const float oma = 1.f - a.acc[p];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) c[ch] = a.rgb[ch * a.HW + p] + s[ch] * oma;
        const float* A = a.affine;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float gi = g[i * a.HW + p];
            if (a.flags & SGR_SKY_CLAMP) {
                const float o = AFF ? ((A[4 * i] * c[0] + A[4 * i + 1] * c[1]) + A[4 * i + 2] * c[2]) + A[4 * i + 3] : c[i];
                gp[i] = sky_passes(o) ? gi : 0.f;
            } else {
                gp[i] = gi;
            }
        }
        if constexpr (AFF) {
#pragma unroll
            for (int j = 0; j < 3; j++) dc[j] = (A[j] * gp[0] + A[4 + j] * gp[1]) + A[8 + j] * gp[2];
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) sums[4 * i + j] = gp[i] * c[j];
                sums[4 * i + 3] = gp[i];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++) dc[j] = gp[j];
        }
#pragma unroll
        for (int j = 0; j < 3; j++) drgb[j * a.HW + p] = dc[j];
        dacc[p] = -((dc[0] * s[0] + dc[1] * s[1]) + dc[2] * s[2]);
        if (m) {
#pragma unroll
            for (int j = 0; j < 3; j++) up[3 * (size_t)lo + j] = sky_passes(raw[j]) ? dc[j] * oma : 0.f;
        }
    }
    if constexpr (AFF) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            float v = sums[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            sums[k] = v;
        }
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < 12; k++) red[wave][k] = sums[k];
        __syncthreads();
        if (threadIdx.x < 12)
            part[(size_t)blockIdx.x * 12 + threadIdx.x] =
                (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// one block: dL/daffine[k] = the nb partials of sum k, in double, lane t taking blocks t, t + 256, ... and the 256 lane
// sums added in lane order
__global__ void __launch_bounds__(256) sgr_sky_affine_kernel(const float* __restrict__ part, uint32_t nb,
                                                             float* __restrict__ dA) {
    __shared__ double lds[256][13];
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.0;
    for (uint32_t b = threadIdx.x; b < nb; b += 256)
#pragma unroll
        for (int k = 0; k < 12; k++) acc[k] += (double)part[(size_t)b * 12 + k];
#pragma unroll
    for (int k = 0; k < 12; k++) lds[threadIdx.x][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 12) {
        double s = 0.0;
        for (int t = 0; t < 256; t++) s += lds[t][threadIdx.x];
        dA[threadIdx.x] = (float)s;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
namespace {

int check(int H, int W, int R, int C) {
    if (C != 3) return sgr_set_error(SGR_E_INVALID, "sky: only C = 3 is supported");
    if (H < 1 || W < 1 || R < 1) return sgr_set_error(SGR_E_INVALID, "sky: need H, W, R >= 1");
    if ((int64_t)H * W > 0x7fffffffll) return sgr_set_error(SGR_E_INVALID, "sky: more than 2^31 - 1 pixels");
    if (!sgr_cube_seam()) return sgr_set_error(SGR_E_INVALID, "sky: the cube seam table could not be derived");
    return 0;
}

size_t tex_bytes(int H, int W, int R) { return sgr_texture_cube_workspace_bytes(1, 1, R, 3, (int64_t)H * W); }

}  // namespace

size_t sgr_sky_workspace_bytes(int H, int W, int R, int C, int part) {
    if (check(H, W, R, C) < 0) return 0;
    const int64_t HW = (int64_t)H * W;
    if (part == SGR_SKY_SAVED) return sgr_required([&](char* base, char** end) { carve_saved(base, HW, end); });
    if (part == SGR_SKY_SCRATCH) {
        const size_t tb = tex_bytes(H, W, R);
        if (!tb) return 0;
        return sgr_required([&](char* base, char** end) { carve_scratch(base, HW, tb, end); });
    }
    if (part == SGR_SKY_SCRATCH_DEFERRED)  // the texture stages work in the deferred workspace instead
        return sgr_required([&](char* base, char** end) { carve_scratch(base, HW, 0, end); });
    return 0;
}

int sgr_sky_forward(int H, int W, int R, int C, const float* rgb, const float* acc, const float* cube, const float* K,
                    const float* w2c, const uint8_t* sky_mask, const float* perturb_x, const float* perturb_y,
                    const float* affine, int flags, float* out, void* saved, void* stream_) {
    if (const int rc = check(H, W, R, C)) return rc;
    if (!rgb || !acc || !cube || !K || !w2c || !out || !saved)
        return sgr_set_error(SGR_E_INVALID, "sky: rgb, acc, cube, K, w2c, out and saved are required");
    if ((flags & SGR_SKY_TRAIN) && (!perturb_x || !perturb_y))
        return sgr_set_error(SGR_E_INVALID, "sky: training rays need perturb_x and perturb_y");
    hipStream_t s = (hipStream_t)stream_;
    const int64_t HW = (int64_t)H * W;
    SkySaved v = carve_saved((char*)sgr_align_up((size_t)saved, 256), HW);
    const SkyArgs a{H, W, R, HW, flags, rgb, acc, cube, K, w2c, perturb_x, perturb_y, affine, sky_mask};
    sgr_sky_flag_kernel<<<blocks(HW), kBlock, 0, s>>>(a, v.flag);
    sgr_launch_scan(v.flag, v.flag, (size_t)HW, v.scan_tmp, true, s, v.count, nullptr, 1, nullptr, nullptr);
    sgr_sky_fwd_kernel<<<blocks(HW), kBlock, 0, s>>>(a, *sgr_cube_seam(), v.flag, v.rays, v.sky, out);
    SGR_HIP(hipGetLastError());
    return 0;
}

namespace {

// Stages 4 and 5 of the backward, then stage 6 in one of its two forms: the whole texture backward into dL_dcube
// (sgr_sky_backward), or without the gather, into the deferred workspace and the activity bytes
// (sgr_sky_backward_deferred, include/sgr_sky_step.h).
int backward(int H, int W, int R, int C, const float* dL_dout, const float* rgb, const float* acc, const float* affine,
             int flags, const void* saved, float* dL_drgb, float* dL_dacc, float* dL_dcube, void* cube_work,
             uint8_t* active, float* dL_daffine, void* scratch, hipStream_t s) {
    if (const int rc = check(H, W, R, C)) return rc;
    const bool deferred = dL_dcube == nullptr;
    if (!dL_dout || !rgb || !acc || !saved || !dL_drgb || !dL_dacc || !scratch || (affine && !dL_daffine) ||
        (deferred && (!cube_work || !active)))
        return sgr_set_error(SGR_E_INVALID, "sky: a required pointer of the backward is missing");
    const int64_t HW = (int64_t)H * W;
    const SkySaved v = carve_saved((char*)sgr_align_up((size_t)saved, 256), HW);
    const SkyScratch w = carve_scratch((char*)sgr_align_up((size_t)scratch, 256), HW, deferred ? 0 : tex_bytes(H, W, R));
    const SkyArgs a{H, W, R, HW, flags, rgb, acc, nullptr, nullptr, nullptr, nullptr, nullptr, affine, nullptr};
    const unsigned nb = blocks(HW);
    if (affine) {
        sgr_sky_bwd_kernel<true><<<nb, kBlock, 0, s>>>(a, dL_dout, v.flag, v.sky, dL_drgb, dL_dacc, w.up, w.part);
        sgr_sky_affine_kernel<<<1, 256, 0, s>>>(w.part, nb, dL_daffine);
    } else {
        sgr_sky_bwd_kernel<false><<<nb, kBlock, 0, s>>>(a, dL_dout, v.flag, v.sky, dL_drgb, dL_dacc, w.up, w.part);
    }
    SGR_HIP(hipGetLastError());
    if (deferred) return sgr_texture_cube_deferred_impl(R, HW, v.rays, w.up, cube_work, v.count, active, s);
    return sgr_texture_cube_backward_impl(1, 1, R, 3, HW, v.rays, w.up, dL_dcube, w.tex_work, v.count, s);
}

}  // namespace

int sgr_sky_backward(int H, int W, int R, int C, const float* dL_dout, const float* rgb, const float* acc,
                     const float* affine, int flags, const void* saved, float* dL_drgb, float* dL_dacc, float* dL_dcube,
                     float* dL_daffine, void* scratch, void* stream_) {
    if (!dL_dcube) return sgr_set_error(SGR_E_INVALID, "sky: a required pointer of the backward is missing");
    return backward(H, W, R, C, dL_dout, rgb, acc, affine, flags, saved, dL_drgb, dL_dacc, dL_dcube, nullptr, nullptr,
                    dL_daffine, scratch, (hipStream_t)stream_);
}

// ---- the cube map's optimiser step (include/sgr_sky_step.h) -----------------------------------------------------------
int sgr_sky_step_block_texels(void) { return SGR_TX_STEP_BLOCK; }

size_t sgr_sky_step_workspace_bytes(int H, int W, int R) {
    if (check(H, W, R, 3) < 0) return 0;
    return sgr_texture_cube_deferred_bytes(R, (int64_t)H * W);
}

int sgr_sky_backward_deferred(int H, int W, int R, int C, const float* dL_dout, const float* rgb, const float* acc,
                              const float* affine, int flags, const void* saved, float* dL_drgb, float* dL_dacc,
                              void* cube_work, uint8_t* active, float* dL_daffine, void* scratch, void* stream_) {
    if (!cube_work || !active) return sgr_set_error(SGR_E_INVALID, "sky: cube_work and active are required");
    return backward(H, W, R, C, dL_dout, rgb, acc, affine, flags, saved, dL_drgb, dL_dacc, nullptr, cube_work, active,
                    dL_daffine, scratch, (hipStream_t)stream_);
}

int sgr_sky_adam_step(int R, float* cube, float* exp_avg, float* exp_avg_sq, const void* cube_work, const uint8_t* active,
                      float step_size, float bc2_sqrt, float eps, double beta1, double beta2, void* stream_) {
    if (R < 1) return sgr_set_error(SGR_E_INVALID, "sky: need R >= 1");
    return sgr_texture_cube_adam_step_impl(R, cube, exp_avg, exp_avg_sq, cube_work, active, step_size, bc2_sqrt, eps,
                                           beta1, beta2, (hipStream_t)stream_);
}

int sgr_sky_test_rays(int H, int W, const float* K, const float* w2c, const float* perturb_x, const float* perturb_y,
                      int flags, float* rays, float* kinv, void* stream_) {
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffll) return sgr_set_error(SGR_E_INVALID, "sky: need H, W >= 1");
    if (!K || !w2c || !rays || !kinv || ((flags & SGR_SKY_TRAIN) && (!perturb_x || !perturb_y)))
        return sgr_set_error(SGR_E_INVALID, "sky: K, w2c, rays, kinv (and the perturbation in training) are required");
    const int64_t HW = (int64_t)H * W;
    const SkyArgs a{H, W, 1, HW, flags, nullptr, nullptr, nullptr, K, w2c, perturb_x, perturb_y, nullptr, nullptr};
    sgr_sky_rays_kernel<<<blocks(HW), kBlock, 0, (hipStream_t)stream_>>>(a, rays, kinv);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_test_sort32_count(uint32_t* keys0, uint32_t* keys1, uint32_t* vals0, uint32_t* vals1, uint32_t n, int end_bit,
                          int max_bits, const uint32_t* dev_n, uint32_t* hist, uint32_t* scan_tmp, void* stream_) {
    if (max_bits != 8 && max_bits != 9) return sgr_set_error(SGR_E_INVALID, "sgr_test_sort32_count: max_bits must be 8 or 9");
    if (!dev_n) return sgr_set_error(SGR_E_INVALID, "sgr_test_sort32_count: dev_n is required");
    uint32_t* keys[2] = {keys0, keys1};
    uint32_t* vals[2] = {vals0, vals1};
    const int cur = sgr_launch_sort_pairs32(keys, vals, n, end_bit, hist, scan_tmp, (hipStream_t)stream_, false, nullptr,
                                            nullptr, max_bits, 0, dev_n);
    SGR_HIP(hipGetLastError());
    return cur;
}
