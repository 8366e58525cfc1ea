// sgr_cube.h -- the cube-map lookup as device functions, shared by the texture op (sgr_texture.hip) and the fused sky
// composite (sgr_sky.hip), and the texture backward's internal entry.  The arithmetic is the contract of
// include/sgr_texture.h; both sources inline the SAME tx_lookup, so a sky pixel's value is bit-identical to texture()'s.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Edges of a face: 0 = column -1, 1 = column R, 2 = row -1, 3 = row R.  A tap at position k along edge e of face f is
// texel (col, row) = (c0 (R-1) + c1 k, r0 (R-1) + r1 k) of face g; back = the edge of g that leads back to f.
struct SgrCubeSeam {
    int8_t g[6][4], c0[6][4], c1[6][4], r0[6][4], r1[6][4], back[6][4];
};

__device__ __forceinline__ float tx_su(int f) { return (f == 0 || f == 5) ? -1.f : 1.f; }  // SU = (-1, +1, +1, +1, +1, -1)
__device__ __forceinline__ float tx_sv(int f) { return f == 2 ? 1.f : -1.f; }              // SV = (-1, -1, +1, -1, -1, -1)

// Face and texel-space position (x, y) = (u R - 0.5, v R - 0.5) of direction d; false when (u, v) is not finite.
__device__ __forceinline__ bool tx_coords(float dx, float dy, float dz, int R, int& face, float& x, float& y) {
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    float c, s, t;
    if (az > fmaxf(ax, ay)) { c = dz; s = dx; t = dy; face = 4 + (c < 0.f); }
    else if (ay > ax) { c = dy; s = dx; t = dz; face = 2 + (c < 0.f); }
    else { c = dx; s = dz; t = dy; face = 0 + (c < 0.f); }
    const float m = 0.5f / fabsf(c);
    float u = s * tx_su(face) * m + 0.5f, v = t * tx_sv(face) * m + 0.5f;
    if (!isfinite(u) || !isfinite(v)) return false;
    u = fminf(fmaxf(u, 0.f), 1.f);
    v = fminf(fmaxf(v, 0.f), 1.f);
    x = u * (float)R - 0.5f;
    y = v * (float)R - 0.5f;
    return true;
}

// Texel (within one batch's 6 R R texels) of footprint tap (col, row) of face f, or -1 when it lies outside two edges.
__device__ __forceinline__ int64_t tx_tap(const SgrCubeSeam& sm, int R, int f, int col, int row) {
    const bool ox = col < 0 || col >= R, oy = row < 0 || row >= R;
    if (ox && oy) return -1;
    if (ox || oy) {
        const int e = ox ? (col < 0 ? 0 : 1) : (row < 0 ? 2 : 3);
        const int k = ox ? row : col;
        const int g = sm.g[f][e];
        col = sm.c0[f][e] * (R - 1) + sm.c1[f][e] * k;
        row = sm.r0[f][e] * (R - 1) + sm.r1[f][e] * k;
        f = g;
    }
    return ((int64_t)f * R + row) * R + col;
}

// The four taps of cell (x0, y0) of face f in the order (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1); a missing corner
// tap gets index -1.
__device__ __forceinline__ int tx_cell_taps(const SgrCubeSeam& sm, int R, int f, int x0, int y0, int64_t idx[4]) {
    int miss = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        idx[k] = tx_tap(sm, R, f, x0 + (k & 1), y0 + (k >> 1));
        if (idx[k] < 0) miss = k;
    }
    return miss;
}

__device__ __forceinline__ void tx_weights(float fx, float fy, float w[4]) {
    w[0] = (1.f - fx) * (1.f - fy);
    w[1] = fx * (1.f - fy);
    w[2] = (1.f - fx) * fy;
    w[3] = fx * fy;
}

// The bilinear lookup of one direction (dx, dy, dz) in the 6 R R C texels at T, written to o[0, C).  CT > 0: C = CT at
// compile time; CT = 0: C = Crt at run time.  A direction whose (u, v) is not finite gives 0.
template <int CT>
__device__ __forceinline__ void tx_lookup(const float* __restrict__ T, int R, int Crt, const SgrCubeSeam& sm, float dx,
                                          float dy, float dz, float* __restrict__ o) {
    const int C = CT > 0 ? CT : Crt;
    int face;
    float x, y;
    if (!tx_coords(dx, dy, dz, R, face, x, y)) {
        for (int ch = 0; ch < C; ch++) o[ch] = 0.f;
        return;
    }
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf;
    float w[4];
    tx_weights(x - xf, y - yf, w);
    int64_t idx[4];
    if (x0 >= 0 && y0 >= 0 && x0 < R - 1 && y0 < R - 1) {
        idx[0] = ((int64_t)face * R + y0) * R + x0;
        idx[1] = idx[0] + 1;
        idx[2] = idx[0] + R;
        idx[3] = idx[2] + 1;
    } else {
        const int miss = tx_cell_taps(sm, R, face, x0, y0, idx);
        if (miss >= 0) {  // the corner outside both edges: the mean of the other three texels
            const float share = w[miss] * (1.f / 3.f);
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] += share;
            w[miss] = 0.f;
            idx[miss] = idx[miss ^ 3];  // any valid texel: its weight is 0
        }
    }
    if constexpr (CT > 0) {
        float acc[CT];
#pragma unroll
        for (int ch = 0; ch < CT; ch++) acc[ch] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float* t = T + idx[k] * CT;
#pragma unroll
            for (int ch = 0; ch < CT; ch++) acc[ch] += w[k] * t[ch];
        }
#pragma unroll
        for (int ch = 0; ch < CT; ch++) o[ch] = acc[ch];
    } else {
        for (int ch = 0; ch < C; ch++) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) a += w[k] * T[idx[k] * C + ch];
            o[ch] = a;
        }
    }
}

// ---- host (sgr_texture.hip) -----------------------------------------------------------------------------------------
// The seam table (nullptr when it could not be derived).
const SgrCubeSeam* sgr_cube_seam();
// The texture backward of include/sgr_texture.h.  dev_n == nullptr: all B n samples, as sgr_texture_cube_backward.
// dev_n != nullptr (Bt = B = 1): only samples [0, *dev_n) exist -- a count that lives on the device, so the caller never
// reads it back; the launches stay sized by n, and the key, sort, starts and record stages neither read nor write past
// the count.  workspace: sgr_texture_cube_workspace_bytes(Bt, B, R, C, n).
int sgr_texture_cube_backward_impl(int Bt, int B, int R, int C, int64_t n, const float* uv, const float* dL_dout,
                                   float* dL_dtex, void* workspace, const uint32_t* dev_n, hipStream_t stream);

// The backward in two halves, for include/sgr_sky_step.h (C = 3, Bt = B = 1, a device-side count).  A block is
// SGR_TX_STEP_BLOCK consecutive texels of the flat [6, R, R] index.
#define SGR_TX_STEP_BLOCK 256
// bytes of the deferred workspace (0 when the arguments are invalid)
size_t sgr_texture_cube_deferred_bytes(int R, int64_t n);
// key, sort, records and starts into `work`, and active[b] = 1 for every block that holds a tap texel of a sample
int sgr_texture_cube_deferred_impl(int R, int64_t n, const float* uv, const float* dL_dout, void* work,
                                   const uint32_t* dev_n, uint8_t* active, hipStream_t stream);
// one launch over all blocks: the gather's sum of every texel of an active block, then adam1 on its three elements of
// p / m / v; work == nullptr: no samples (g = 0)
int sgr_texture_cube_adam_step_impl(int R, float* p, float* m, float* v, const void* work, const uint8_t* active,
                                    float step_size, float bc2_sqrt, float eps, double beta1, double beta2,
                                    hipStream_t stream);
