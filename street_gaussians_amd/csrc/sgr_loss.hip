// sgr_loss.hip -- the colour loss right after the rasterizer (include/sgr_loss.h) on gfx950.
//
// SSIM: the reference's 11x11 window is the outer product of a normalised 1-D Gaussian (loss_utils.py:70-78), so the
// five windowed means (mu1, mu2, E[x^2], E[y^2], E[xy]) are computed separably inside one workgroup: a 16x16 output tile
// stages its 26x26 input halo in LDS, filters the 26 rows horizontally (5 quantities), then the 16 columns
// vertically, evaluates the SSIM expression and -- for the backward -- its three partial derivatives per position.
// The backward filters those three maps the same way: dL/dx = G*(dM/dmu1) + 2x G*(dM/ds11) + y G*(dM/ds12)
// (the window is symmetric and the padding is zero, so the adjoint of the correlation is the correlation).
// 2 kernels instead of ~30 (MIOpen depthwise convs + elementwise autograd graph); HBM traffic: two images in, three
// maps out / three maps + two images in, one gradient out.
#include <string>

#include "../../include/sgr_loss.h"
#include "sgr_common.h"
#include "sgr_loss_internal.h"  // the SSIM steps, block sum and per-pixel terms shared with sgr_frame_loss.hip

template <bool WITH_PARTIALS>
__global__ void __launch_bounds__(256)
sgr_ssim_fwd_kernel(int H, int W, const float* __restrict__ img1, const float* __restrict__ img2,
                    const uint8_t* __restrict__ mask, SgrGauss11 g, float* __restrict__ partials,
                    float* __restrict__ block_sums) {
    __shared__ SsimHalo sx, sy;
    __shared__ SsimRows hb[5];
    __shared__ float lds4[4];
    const int c = blockIdx.z, x0 = blockIdx.x * SGR_LS_T, y0 = blockIdx.y * SGR_LS_T;
    const size_t plane = (size_t)H * W;
    const float* p1 = img1 + c * plane;
    const float* p2 = img2 + c * plane;
    for (int e = threadIdx.x; e < SGR_LS_IN * SGR_LS_IN; e += 256) {
        const int r = e / SGR_LS_IN, q = e - r * SGR_LS_IN;
        const int y = y0 + r - SGR_LS_R, x = x0 + q - SGR_LS_R;
        float a = 0.f, b = 0.f;
        if (x >= 0 && x < W && y >= 0 && y < H) {  // zero padding (F.conv2d padding=5); masked pixels are zeros (:92-94)
            const size_t o = (size_t)y * W + x;
            if (!mask || mask[o]) { a = p1[o]; b = p2[o]; }
        }
        sx[r][q] = a;
        sy[r][q] = b;
    }
    __syncthreads();
    ssim_hpass5(threadIdx.x, sx, sy, g, hb);
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float m[5];
    ssim_vpass<5>(hb, g, ty, tx, m);
    const int x = x0 + tx, y = y0 + ty;
    float val = 0.f;
    if (x < W && y < H) {
        float part[3];
        ssim_point(m, val, part);
        if (WITH_PARTIALS) {
            const size_t o = c * plane + (size_t)y * W + x, cp = (size_t)gridDim.z * plane;
            partials[o] = part[0];
            partials[cp + o] = part[1];
            partials[2 * cp + o] = part[2];
        }
    }
    const float s = block_sum_256(val, lds4);
    if (threadIdx.x == 0) block_sums[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

// one workgroup: out[0] = scale * sum(v[0..n)) in a fixed order; out[1] = optional second quantity (counts)
__global__ void __launch_bounds__(256)
sgr_final_sum_kernel(const float* __restrict__ v, size_t n, float scale, const float* __restrict__ v2, float* __restrict__ out,
                     int mean_by_second) {
    __shared__ float lds4[4];
    float a = 0.f, b = 0.f;
    for (size_t i = threadIdx.x; i < n; i += 256) {
        a += v[i];
        if (v2) b += v2[i];
    }
    const float sa = block_sum_256(a, lds4);
    __syncthreads();
    const float sb = v2 ? block_sum_256(b, lds4) : 0.f;
    if (threadIdx.x == 0) {
        if (mean_by_second) { out[0] = sa / sb; out[1] = sb; }
        else out[0] = sa * scale;
    }
}

__global__ void __launch_bounds__(256)
sgr_ssim_bwd_kernel(int H, int W, int C, const float* __restrict__ img1, const float* __restrict__ img2,
                    const uint8_t* __restrict__ mask, SgrGauss11 g, const float* __restrict__ partials,
                    const float* __restrict__ upstream, float* __restrict__ dimg1, float w_ssim, float w_l1,
                    const float* __restrict__ l1_out) {
    __shared__ SsimHalo sp[3];
    __shared__ SsimRows hb[3];
    const int c = blockIdx.z, x0 = blockIdx.x * SGR_LS_T, y0 = blockIdx.y * SGR_LS_T;
    const size_t plane = (size_t)H * W, cp = (size_t)C * plane;
    ssim_stage_partials(threadIdx.x, partials, c, plane, cp, x0, y0, H, W, sp);
    __syncthreads();
    ssim_hpass<3>(threadIdx.x, sp, g, hb);
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    float f[3];
    ssim_vpass<3>(hb, g, ty, tx, f);
    const size_t o = (size_t)y * W + x;
    float out = 0.f;
    if (!mask || mask[o]) {
        const float xv = img1[c * plane + o], yv = img2[c * plane + o];
        out = w_ssim * ssim_grad(f[0], f[1], f[2], xv, yv, upstream[0] / (float)cp);
        // fused colour loss: + w_l1 * d l1_loss / d img1  (loss_utils.py:21-37)
        if (l1_out != nullptr) out += w_l1 * upstream[0] * l1_sign(xv - yv) / l1_out[1];
    }
    dimg1[c * plane + o] = out;
}

// ---- L1 -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sgr_l1_fwd_kernel(int C, size_t plane, const float* __restrict__ a, const float* __restrict__ b,
                  const uint8_t* __restrict__ mask, float* __restrict__ sums, float* __restrict__ counts) {
    __shared__ float lds4[4];
    float s = 0.f, n = 0.f;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < plane; p += (size_t)gridDim.x * 256) {
        if (mask && !mask[p]) continue;
        for (int c = 0; c < C; c++) s += fabsf(a[c * plane + p] - b[c * plane + p]);
        n += (float)C;
    }
    const float ss = block_sum_256(s, lds4);
    __syncthreads();
    const float nn = block_sum_256(n, lds4);
    if (threadIdx.x == 0) { sums[blockIdx.x] = ss; counts[blockIdx.x] = nn; }
}

__global__ void __launch_bounds__(256)
sgr_l1_bwd_kernel(int C, size_t plane, const float* __restrict__ a, const float* __restrict__ b,
                  const uint8_t* __restrict__ mask, const float* __restrict__ out, const float* __restrict__ upstream,
                  float* __restrict__ da) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)C * plane) return;
    const size_t p = i % plane;
    float g = 0.f;
    if (!mask || mask[p]) g = l1_sign(a[i] - b[i]) * (upstream[0] / out[1]);
    da[i] = g;
}

// ---- accumulation terms (train.py:106-121) --------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sgr_bce_fwd_kernel(int n, int mode, const float* __restrict__ acc, const uint8_t* __restrict__ mask,
                   float* __restrict__ sums) {
    __shared__ float lds4[4];
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
        s += bce_term(mode, bce_clamp(acc[i]), mask && mask[i]);
    }
    const float t = block_sum_256(s, lds4);
    if (threadIdx.x == 0) sums[blockIdx.x] = t;
}
__global__ void __launch_bounds__(256)
sgr_bce_bwd_kernel(int n, int mode, const float* __restrict__ acc, const uint8_t* __restrict__ mask,
                   const float* __restrict__ upstream, float* __restrict__ dacc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const float x = acc[i];
    float g = 0.f;
    if (bce_clamp_passes(x)) g = bce_grad(mode, x, mask && mask[i]) * (upstream[0] / (float)n);
    dacc[i] = g;
}

// ---- LiDAR depth term with top-95 % selection (train.py:124-131) ---------------------------------------------------
// (LdWork, its carve and the per-pixel key / gradient: sgr_loss_internal.h)
__global__ void __launch_bounds__(256)
sgr_lidar_err_kernel(int n, const float* __restrict__ depth, const float* __restrict__ acc, const float* __restrict__ lidar,
                     const uint8_t* __restrict__ mask, LdWork w) {
    __shared__ uint32_t cnt[4];
    uint32_t c = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
        const float l = lidar[i];
        uint32_t key = 0xffffffffu;
        if (l > 0.f && (!mask || mask[i])) {  // depth_mask = (lidar_depth > 0) & mask
            key = lidar_key(depth[i], acc[i], l);
            c++;
        }
        w.key[i] = key;
    }
    wave_sums_to_lds(c, cnt);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&w.state[0], lds4_total(cnt));  // integers: order-independent
}
__global__ void sgr_lidar_k_kernel(LdWork w, double keep) {
    const uint32_t count = w.state[0];
    const uint32_t k = (uint32_t)(keep * (double)count);  // int(0.95 * depth_error.size(0)): Python float = double
    w.state[1] = k;
    w.state[2] = 0;  // prefix
    w.state[3] = k;  // we look for the k-th smallest (1-based) -> rank k inside the current prefix class
}
// histogram of byte `pass` (3 = most significant) over the selected keys whose higher bytes equal the prefix
__global__ void __launch_bounds__(256)
sgr_lidar_hist_kernel(int n, int pass, LdWork w) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t prefix = w.state[2];
    const int shift = 8 * pass;
    const uint32_t himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
        const uint32_t key = w.key[i];
        if (key != 0xffffffffu && (key & himask) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&w.hist[pass * 256 + threadIdx.x], h[threadIdx.x]);
}
__global__ void sgr_lidar_select_kernel(int pass, LdWork w) {  // one lane
    uint32_t k = w.state[3], acc = 0;
    if (w.state[1] == 0) return;
    int b = 0;
    for (; b < 256; b++) {
        const uint32_t c = w.hist[pass * 256 + b];
        if (acc + c >= k) break;
        acc += c;
    }
    if (b > 255) b = 255;
    w.state[2] |= (uint32_t)b << (8 * pass);
    w.state[3] = k - acc;  // rank inside the chosen bin; after the last pass: how many of the tied errors are taken
    if (pass == 0) {
        w.state[5] = w.hist[b];                 // errors equal to the threshold
        w.state[4] = w.state[1] - w.state[3];   // errors strictly below it
    }
}
__global__ void __launch_bounds__(256)
sgr_lidar_sum_kernel(int n, LdWork w) {
    __shared__ float lds4[4];
    const uint32_t t = w.state[2];
    float s = 0.f;
    if (w.state[1] > 0)
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
            const uint32_t key = w.key[i];
            if (key < t) s += __uint_as_float(key);
        }
    const float r = block_sum_256(s, lds4);
    if (threadIdx.x == 0) w.sums[blockIdx.x] = r;
}
__global__ void __launch_bounds__(256)
sgr_lidar_final_kernel(LdWork w, float* __restrict__ out) {
    __shared__ float lds4[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < SGR_L1_BLOCKS; i += 256) a += w.sums[i];
    const float below = block_sum_256(a, lds4);
    if (threadIdx.x == 0) {
        const uint32_t k = w.state[1];
        const float thr = __uint_as_float(w.state[2]);
        const uint32_t take = w.state[3];  // how many of the tied errors belong to the k smallest
        out[0] = k ? (below + (float)take * thr) / (float)k : __builtin_nanf("");  // mean of an empty tensor is NaN
        out[1] = (float)k;
        out[2] = thr;
        out[3] = (k && w.state[5]) ? (float)take / (float)w.state[5] : 0.f;
    }
}
__global__ void __launch_bounds__(256)
sgr_lidar_bwd_kernel(int n, const float* __restrict__ depth, const float* __restrict__ acc, const float* __restrict__ lidar,
                     const float* __restrict__ out, LdWork w, const float* __restrict__ upstream,
                     float* __restrict__ ddepth, float* __restrict__ dacc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    float gd, ga;
    lidar_grad(w.key[i], out, depth[i], acc[i], lidar[i], upstream[0], gd, ga);
    ddepth[i] = gd;
    dacc[i] = ga;
}

void sgr_lidar_select_launch(int n, const LdWork& w, double keep, float* out, hipStream_t stream) {
    sgr_lidar_k_kernel<<<1, 1, 0, stream>>>(w, keep);
    for (int pass = 3; pass >= 0; pass--) {
        sgr_lidar_hist_kernel<<<SGR_L1_BLOCKS, 256, 0, stream>>>(n, pass, w);
        sgr_lidar_select_kernel<<<1, 1, 0, stream>>>(pass, w);
    }
    sgr_lidar_sum_kernel<<<SGR_L1_BLOCKS, 256, 0, stream>>>(n, w);
    sgr_lidar_final_kernel<<<1, 256, 0, stream>>>(w, out);
}

extern "C" {

size_t sgr_ssim_workspace_floats(int C, int H, int W) {
    const dim3 g = tile_grid(C, H, W);
    return (size_t)g.x * g.y * g.z;
}

int sgr_ssim_forward(int C, int H, int W, const float* img1, const float* img2, const uint8_t* mask, float* out_ssim,
                     float* partials, float* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = ls_check_dims(C, H, W)) return rc;
    if (!img1 || !img2 || !out_ssim || !workspace) return sgr_set_error(SGR_E_INVALID, "img1, img2, out_ssim and workspace are required");
    const dim3 grid = tile_grid(C, H, W);
    if (partials) sgr_ssim_fwd_kernel<true><<<grid, 256, 0, stream>>>(H, W, img1, img2, mask, ssim_window(), partials, workspace);
    else sgr_ssim_fwd_kernel<false><<<grid, 256, 0, stream>>>(H, W, img1, img2, mask, ssim_window(), nullptr, workspace);
    sgr_final_sum_kernel<<<1, 256, 0, stream>>>(workspace, (size_t)grid.x * grid.y * grid.z,
                                                1.0f / ((float)C * (float)H * (float)W), nullptr, out_ssim, 0);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_ssim_backward(int C, int H, int W, const float* img1, const float* img2, const uint8_t* mask,
                      const float* partials, const float* upstream, float* dL_dimg1, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = ls_check_dims(C, H, W)) return rc;
    if (!img1 || !img2 || !partials || !upstream || !dL_dimg1)
        return sgr_set_error(SGR_E_INVALID, "img1, img2, partials, upstream and dL_dimg1 are required");
    sgr_ssim_bwd_kernel<<<tile_grid(C, H, W), 256, 0, stream>>>(H, W, C, img1, img2, mask, ssim_window(), partials, upstream,
                                                                dL_dimg1, 1.0f, 0.0f, nullptr);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_color_loss_backward(int C, int H, int W, const float* img1, const float* img2, const uint8_t* mask,
                            const float* partials, const float* l1_out, float w_l1, float w_ssim, const float* upstream,
                            float* dL_dimg1, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = ls_check_dims(C, H, W)) return rc;
    if (!img1 || !img2 || !partials || !l1_out || !upstream || !dL_dimg1)
        return sgr_set_error(SGR_E_INVALID, "img1, img2, partials, l1_out, upstream and dL_dimg1 are required");
    sgr_ssim_bwd_kernel<<<tile_grid(C, H, W), 256, 0, stream>>>(H, W, C, img1, img2, mask, ssim_window(), partials, upstream,
                                                                dL_dimg1, w_ssim, w_l1, l1_out);
    SGR_HIP(hipGetLastError());
    return 0;
}

size_t sgr_l1_workspace_floats(int C, int H, int W) {
    (void)C; (void)H; (void)W;
    return 2 * SGR_L1_BLOCKS;
}

int sgr_l1_forward(int C, int H, int W, const float* a, const float* b, const uint8_t* mask, float* out, float* workspace,
                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = ls_check_dims(C, H, W)) return rc;
    if (!a || !b || !out || !workspace) return sgr_set_error(SGR_E_INVALID, "a, b, out and workspace are required");
    const size_t plane = (size_t)H * W;
    sgr_l1_fwd_kernel<<<SGR_L1_BLOCKS, 256, 0, stream>>>(C, plane, a, b, mask, workspace, workspace + SGR_L1_BLOCKS);
    sgr_final_sum_kernel<<<1, 256, 0, stream>>>(workspace, SGR_L1_BLOCKS, 1.0f, workspace + SGR_L1_BLOCKS, out, 1);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_l1_backward(int C, int H, int W, const float* a, const float* b, const uint8_t* mask, const float* out,
                    const float* upstream, float* dL_da, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = ls_check_dims(C, H, W)) return rc;
    if (!a || !b || !out || !upstream || !dL_da) return sgr_set_error(SGR_E_INVALID, "a, b, out, upstream and dL_da are required");
    const size_t n = (size_t)C * H * W;
    sgr_l1_bwd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(C, (size_t)H * W, a, b, mask, out, upstream, dL_da);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_bce_forward(int n, int mode, const float* acc, const uint8_t* mask, float* out, float* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0 || (mode != SGR_BCE_SKY && mode != SGR_BCE_OBJECT)) return sgr_set_error(SGR_E_INVALID, "n > 0 and a valid mode are required");
    if (!acc || !out || !workspace) return sgr_set_error(SGR_E_INVALID, "acc, out and workspace are required");
    sgr_bce_fwd_kernel<<<SGR_L1_BLOCKS, 256, 0, stream>>>(n, mode, acc, mask, workspace);
    sgr_final_sum_kernel<<<1, 256, 0, stream>>>(workspace, SGR_L1_BLOCKS, 1.0f / (float)n, nullptr, out, 0);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_bce_backward(int n, int mode, const float* acc, const uint8_t* mask, const float* upstream, float* dL_dacc,
                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0 || (mode != SGR_BCE_SKY && mode != SGR_BCE_OBJECT)) return sgr_set_error(SGR_E_INVALID, "n > 0 and a valid mode are required");
    if (!acc || !upstream || !dL_dacc) return sgr_set_error(SGR_E_INVALID, "acc, upstream and dL_dacc are required");
    sgr_bce_bwd_kernel<<<(n + 255) / 256, 256, 0, stream>>>(n, mode, acc, mask, upstream, dL_dacc);
    SGR_HIP(hipGetLastError());
    return 0;
}

size_t sgr_lidar_work_bytes(int n) {
    return ld_work_bytes((size_t)(n > 0 ? n : 1));
}

int sgr_lidar_depth_forward(int n, const float* depth, const float* acc, const float* lidar_depth, const uint8_t* mask,
                            double keep, float* out, char* work, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0) return sgr_set_error(SGR_E_INVALID, "n must be positive");
    if (!depth || !acc || !lidar_depth || !out || !work) return sgr_set_error(SGR_E_INVALID, "depth, acc, lidar_depth, out and work are required");
    const LdWork w = ld_carve((char*)sgr_align_up((size_t)work, 256), (size_t)n);
    SGR_HIP(hipMemsetAsync(w.hist, 0, 4 * 256 * sizeof(uint32_t), stream));
    SGR_HIP(hipMemsetAsync(w.state, 0, 16 * sizeof(uint32_t), stream));
    sgr_lidar_err_kernel<<<SGR_L1_BLOCKS, 256, 0, stream>>>(n, depth, acc, lidar_depth, mask, w);
    sgr_lidar_select_launch(n, w, keep, out, stream);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_lidar_depth_backward(int n, const float* depth, const float* acc, const float* lidar_depth, const float* out,
                             const char* work, const float* upstream, float* dL_ddepth, float* dL_dacc, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0) return sgr_set_error(SGR_E_INVALID, "n must be positive");
    if (!depth || !acc || !lidar_depth || !out || !work || !upstream || !dL_ddepth || !dL_dacc)
        return sgr_set_error(SGR_E_INVALID, "all arrays are required");
    const LdWork w = ld_carve((char*)sgr_align_up((size_t)const_cast<char*>(work), 256), (size_t)n);
    sgr_lidar_bwd_kernel<<<(n + 255) / 256, 256, 0, stream>>>(n, depth, acc, lidar_depth, out, w, upstream, dL_ddepth, dL_dacc);
    SGR_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
