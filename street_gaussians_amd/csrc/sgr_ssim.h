// sgr_ssim.h -- the SSIM steps of sgr_loss.hip and sgr_frame_loss.hip, one text each: window, tile geometry, 11-tap passes,
// the SSIM point, the staging of the partial maps, the gradient flush.  __host__ __device__; the lane index and the LDS arrays
// are parameters and the barriers stay with the caller, so tests/host_math/host_math.hip runs a tile with a loop over tid.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define SGR_LS_T 16           // output tile edge
#define SGR_LS_R 5            // window radius (window_size 11)
#define SGR_LS_IN (SGR_LS_T + 2 * SGR_LS_R)  // 26
#define SGR_SSIM_HD __host__ __device__ __forceinline__

typedef float SsimHalo[SGR_LS_IN][SGR_LS_IN + 1];  // a staged 26x26 input plane
typedef float SsimRows[SGR_LS_IN][SGR_LS_T + 1];   // a plane after the horizontal pass: 26 rows x 16 columns

struct SgrGauss11 { float w[11]; };
// gaussian(11, 1.5) of loss_utils.py:70-72, evaluated like the reference: exp() in double, float32 tensor, / sum
static inline SgrGauss11 make_window() {
    SgrGauss11 g;
    float v[11], s = 0.f;
    for (int x = 0; x < 11; x++) {
        v[x] = (float)exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5));
        s += v[x];
    }
    for (int x = 0; x < 11; x++) g.w[x] = v[x] / s;
    return g;
}
static inline const SgrGauss11& ssim_window() { static const SgrGauss11 g = make_window(); return g; }

// horizontal pass of the forward: two staged planes -> the rows of mu1, mu2, E[x^2], E[y^2], E[xy]
SGR_SSIM_HD void ssim_hpass5(int tid, const SsimHalo& sx, const SsimHalo& sy, const SgrGauss11& g, SsimRows* hb) {
    for (int e = tid; e < SGR_LS_IN * SGR_LS_T; e += 256) {
        const int r = e / SGR_LS_T, q = e - r * SGR_LS_T;
        float m1 = 0.f, m2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float a = sx[r][q + k], b = sy[r][q + k], w = g.w[k];
            m1 += w * a; m2 += w * b; s11 += w * a * a; s22 += w * b * b; s12 += w * a * b;
        }
        hb[0][r][q] = m1; hb[1][r][q] = m2; hb[2][r][q] = s11; hb[3][r][q] = s22; hb[4][r][q] = s12;
    }
}
// horizontal pass over N staged planes (the backward's three partial maps)
template <int N>
SGR_SSIM_HD void ssim_hpass(int tid, const SsimHalo* sp, const SgrGauss11& g, SsimRows* hb) {
    for (int e = tid; e < SGR_LS_IN * SGR_LS_T; e += 256) {
        const int r = e / SGR_LS_T, q = e - r * SGR_LS_T;
        float a[N] = {};
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float w = g.w[k];
#pragma unroll
            for (int n = 0; n < N; n++) a[n] += w * sp[n][r][q + k];
        }
#pragma unroll
        for (int n = 0; n < N; n++) hb[n][r][q] = a[n];
    }
}
// vertical pass: the 11 rows below (ty, tx) of N planes
template <int N>
SGR_SSIM_HD void ssim_vpass(const SsimRows* hb, const SgrGauss11& g, int ty, int tx, float (&out)[N]) {
#pragma unroll
    for (int n = 0; n < N; n++) out[n] = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float w = g.w[k];
#pragma unroll
        for (int n = 0; n < N; n++) out[n] += w * hb[n][ty + k][tx];
    }
}

// loss_utils.py:104-118 at one position from m = {mu1, mu2, E[x^2], E[y^2], E[xy]}: the SSIM map value and
// part = {dM/dmu1, dM/dsigma1^2, dM/dsigma12} (a caller that does not read part pays nothing for it)
SGR_SSIM_HD void ssim_point(const float (&m)[5], float& val, float (&part)[3]) {
    const float m1 = m[0], m2 = m[1], s11 = m[2], s22 = m[3], s12 = m[4];
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
    const float sg1 = s11 - mu1_sq, sg2 = s22 - mu2_sq, sg12 = s12 - mu12;
    const float A = 2.f * mu12 + C1, B = 2.f * sg12 + C2, Cc = mu1_sq + mu2_sq + C1, D = sg1 + sg2 + C2;
    val = (A * B) / (Cc * D);
    const float icd = 1.0f / (Cc * D);
    part[0] = 2.f * m2 * (B - A) * icd - 2.f * m1 * val * (1.0f / Cc - 1.0f / D);
    part[1] = -val / D;
    part[2] = 2.f * A * icd;
}

// the backward's staging: channel c of the three partial maps [3][C][H][W] (cp = C * plane), zero outside the image
SGR_SSIM_HD void ssim_stage_partials(int tid, const float* partials, int c, size_t plane, size_t cp, int x0, int y0,
                                     int H, int W, SsimHalo* sp) {
    for (int e = tid; e < SGR_LS_IN * SGR_LS_IN; e += 256) {
        const int r = e / SGR_LS_IN, q = e - r * SGR_LS_IN;
        const int y = y0 + r - SGR_LS_R, x = x0 + q - SGR_LS_R;
        float a = 0.f, b = 0.f, d = 0.f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t o = c * plane + (size_t)y * W + x;
            a = partials[o]; b = partials[cp + o]; d = partials[2 * cp + o];
        }
        sp[0][r][q] = a; sp[1][r][q] = b; sp[2][r][q] = d;
    }
}
// d(mean SSIM)/dx at a pixel from the filtered partial maps: G*(dM/dmu1) + 2x G*(dM/ds11) + y G*(dM/ds12), times up / (C H W)
SGR_SSIM_HD float ssim_grad(float a, float b, float d, float xv, float yv, float up_over_cp) {
    return (a + 2.f * xv * b + yv * d) * up_over_cp;
}
SGR_SSIM_HD float l1_sign(float df) { return df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f); }  // torch: sign(0) = 0
