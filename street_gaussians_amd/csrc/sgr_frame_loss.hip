// sgr_frame_loss.hip -- every image-space term of a training step in one op (include/sgr_frame_loss.h)
// on gfx950.
//
// Forward: ONE map kernel, a 256-lane workgroup per 16x16 pixel tile.  The tile's mask is read once (the 26x26 halo's
// bits stay in a register of the lane that stages them), then per channel the halo of image and gt is staged in LDS and
// filtered separably with the steps of sgr_ssim.h: SSIM map value + its three partials, and from the staged
// centre value |a - b| and (a - b)^2.  acc / acc_obj / depth / lidar_depth are read once per pixel: sky term, object term,
// LiDAR key (written for the radix select of sgr_loss.hip, sgr_lidar_select_launch).  Six block sums per workgroup go to
// the workspace in block order; one finishing workgroup reduces them in a fixed order and evaluates the eight scalars.
// Backward: ONE kernel over the same tiles writes dL/dimage (the filter of the three partial maps + the L1 sign),
// dL/dacc (sky + LiDAR, added in registers), dL/ddepth and dL/dacc_obj, each once.
#include <string>

#include "../../include/sgr_frame_loss.h"
#include "sgr_common.h"
#include "sgr_loss_internal.h"

#define SGR_FL_SUMS 6  // block sums per workgroup: SSIM map, |a-b|, (a-b)^2, values counted, sky, object
#define SGR_FL_HEAD 64 // floats at the head of `saved`: [0..3] the LiDAR selection {loss, k, threshold, tie weight}, [4] values counted

struct FlSaved {
    float* head;      // [SGR_FL_HEAD]
    float* partials;  // [3][C][H][W]
    LdWork ld;
};
static FlSaved fl_carve(char* base, size_t C, size_t n) {
    FlSaved s;
    char* p = base;
    sgr_carve(p, s.head, SGR_FL_HEAD);
    sgr_carve(p, s.partials, 3 * C * n);
    p = (char*)sgr_align_up((size_t)p, 256);
    s.ld = ld_carve(p, n);
    return s;
}

struct FlWeights { float w_l1, lambda_dssim, lambda_sky, sky_scale, lambda_reg, lambda_lidar; };

// the six per-lane values -> six block sums, written by lanes 0..5 to sums[q * nblocks + block]
__device__ __forceinline__ void fl_block_sums(float (&v)[SGR_FL_SUMS], float (*lds)[4], float* __restrict__ sums, size_t nblocks,
                                              size_t block) {
#pragma unroll
    for (int q = 0; q < SGR_FL_SUMS; q++) wave_sums_to_lds(v[q], lds[q]);
    __syncthreads();
    if (threadIdx.x < SGR_FL_SUMS) {
        const int q = threadIdx.x;
        sums[q * nblocks + block] = lds4_total(lds[q]);
    }
}

__global__ void __launch_bounds__(256)
sgr_frame_loss_map_kernel(int C, int H, int W, sgr_frame_loss_args in, SgrGauss11 g, float* __restrict__ partials, LdWork ld,
                          float* __restrict__ block_sums) {
    __shared__ SsimHalo sx, sy;
    __shared__ SsimRows hb[5];
    __shared__ float red[SGR_FL_SUMS][4];
    __shared__ uint32_t cnt[4];
    const int x0 = blockIdx.x * SGR_LS_T, y0 = blockIdx.y * SGR_LS_T;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < W && y < H;
    const size_t plane = (size_t)H * W, cp = (size_t)C * plane, o = (size_t)y * W + x;
    const bool m = inside && (!in.mask || in.mask[o]);
    // the tile's mask, once: bit t = halo element t * 256 + lane is inside the image and the mask (zero padding of
    // F.conv2d(padding=5); masked pixels of both images are zeros, loss_utils.py:92-94)
    uint32_t live = 0;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int e = t * 256 + threadIdx.x;
        if (e < SGR_LS_IN * SGR_LS_IN) {
            const int r = e / SGR_LS_IN, q = e - r * SGR_LS_IN;
            const int yy = y0 + r - SGR_LS_R, xx = x0 + q - SGR_LS_R;
            if (xx >= 0 && xx < W && yy >= 0 && yy < H && (!in.mask || in.mask[(size_t)yy * W + xx])) live |= 1u << t;
        }
    }
    float v[SGR_FL_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; c++) {
        const float* p1 = in.image + c * plane;
        const float* p2 = in.gt + c * plane;
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const int e = t * 256 + threadIdx.x;
            if (e < SGR_LS_IN * SGR_LS_IN) {
                const int r = e / SGR_LS_IN, q = e - r * SGR_LS_IN;
                float a = 0.f, b = 0.f;
                if (live >> t & 1u) {
                    const size_t oo = (size_t)(y0 + r - SGR_LS_R) * W + (x0 + q - SGR_LS_R);
                    a = p1[oo];
                    b = p2[oo];
                }
                sx[r][q] = a;
                sy[r][q] = b;
            }
        }
        __syncthreads();
        const float ca = sx[ty + SGR_LS_R][tx + SGR_LS_R], cb = sy[ty + SGR_LS_R][tx + SGR_LS_R];
        ssim_hpass5(threadIdx.x, sx, sy, g, hb);
        __syncthreads();
        float mm[5];
        ssim_vpass<5>(hb, g, ty, tx, mm);
        if (inside) {
            float val, part[3];
            ssim_point(mm, val, part);
            const size_t oc = c * plane + o;
            partials[oc] = part[0];
            partials[cp + oc] = part[1];
            partials[2 * cp + oc] = part[2];
            v[0] += val;
            if (m) {  // l1_loss / psnr: the masked pixels' C values (loss_utils.py:21-37, :61-78)
                const float d = ca - cb;
                v[1] += fabsf(d);
                v[2] += d * d;
                v[3] += 1.0f;
            }
        }
        // (the next channel's staging writes sx / sy after every lane passed the second barrier, hb after its first)
    }
    uint32_t nl = 0;
    if (inside) {
        if (in.sky_mask) v[4] = bce_term(0, bce_clamp(in.acc[o]), in.sky_mask[o] != 0);        // train.py:107-108
        if (in.obj_bound) v[5] = bce_term(1, bce_clamp(in.acc_obj[o]), in.obj_bound[o] != 0);  // train.py:117-120
        if (in.lidar_depth) {  // depth_mask = (lidar_depth > 0) & mask, the UNCLAMPED acc (train.py:126-128)
            const float l = in.lidar_depth[o];
            uint32_t key = 0xffffffffu;
            if (l > 0.f && m) {
                key = lidar_key(in.depth[o], in.acc[o], l);
                nl = 1;
            }
            ld.key[o] = key;
        }
    }
    if (in.lidar_depth) wave_sums_to_lds(nl, cnt);
    fl_block_sums(v, red, block_sums, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
    // (fl_block_sums' barrier also orders cnt)  integers: the order of the adds does not matter
    if (in.lidar_depth && threadIdx.x == 0) atomicAdd(&ld.state[0], lds4_total(cnt));
}

// one workgroup: tot[q] = sum of sums[q][0..nblocks), lanes striding over the blocks, in a fixed order.  A trip covers
// 1024 blocks of all Q rows with unconditional loads (index clamped, value dropped past the end): 4 * Q loads are in flight
// per lane instead of one -- the single workgroup is latency-bound (one dependent load per trip measured 56 us at 9600 blocks)
#define SGR_FL_FINISH_SPAN 1024  // block sums per row one trip of the finishing loop covers (sgr_frame_loss_finish_span)
template <int Q>
__device__ __forceinline__ void fl_totals(const float* __restrict__ sums, size_t nblocks, float (&tot)[Q], float* lds4) {
    float a[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) a[q] = 0.f;
    for (size_t i0 = threadIdx.x; i0 < nblocks; i0 += SGR_FL_FINISH_SPAN) {
        float v[4][Q];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t i = i0 + 256 * u, ic = i < nblocks ? i : nblocks - 1;
#pragma unroll
            for (int q = 0; q < Q; q++) v[u][q] = sums[q * nblocks + ic];
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int q = 0; q < Q; q++) a[q] += (i0 + 256 * u < nblocks) ? v[u][q] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < Q; q++) {
        tot[q] = block_sum_256(a[q], lds4);
        __syncthreads();
    }
}
__device__ __forceinline__ float fl_psnr(float mse) { return 20.0f * log10f(1.0f / sqrtf(mse)); }  // loss_utils.py:77

__global__ void __launch_bounds__(256)
sgr_frame_loss_finish_kernel(int C, int H, int W, const float* __restrict__ block_sums, size_t nblocks, FlWeights wt, int sky_on,
                             int obj_on, int lidar_on, float* __restrict__ head, float* __restrict__ terms) {
    __shared__ float lds4[4];
    float tot[SGR_FL_SUMS];
    fl_totals(block_sums, nblocks, tot, lds4);
    if (threadIdx.x != 0) return;
    const float n = (float)H * (float)W;
    const float l1 = tot[1] / tot[3];  // an empty mask: 0 / 0 = NaN like torch's mean
    const float ssim = tot[0] * (1.0f / ((float)C * n));
    const float mse = tot[2] / tot[3];
    const float sky = sky_on ? __fmul_rn(tot[4] * (1.0f / n), wt.sky_scale) : 0.f;  // train.py:110: sky_loss *= scale
    const float obj = obj_on ? tot[5] * (1.0f / n) : 0.f;
    const float lidar = lidar_on ? head[0] : 0.f;
    // train.py:103,112,122,132 in float32, op by op (no fused multiply-add)
    float loss = __fadd_rn(__fmul_rn(wt.w_l1, l1), __fmul_rn(wt.lambda_dssim, __fsub_rn(1.0f, ssim)));
    if (sky_on) loss = __fadd_rn(loss, __fmul_rn(wt.lambda_sky, sky));
    if (obj_on) loss = __fadd_rn(loss, __fmul_rn(wt.lambda_reg, obj));
    if (lidar_on) loss = __fadd_rn(loss, __fmul_rn(wt.lambda_lidar, lidar));
    terms[SGR_FL_L1] = l1;
    terms[SGR_FL_SSIM] = ssim;
    terms[SGR_FL_SKY] = sky;
    terms[SGR_FL_OBJ] = obj;
    terms[SGR_FL_LIDAR] = lidar;
    terms[SGR_FL_MSE] = mse;
    terms[SGR_FL_PSNR] = fl_psnr(mse);
    terms[SGR_FL_LOSS] = loss;
    head[4] = tot[3];
}

__global__ void __launch_bounds__(256)
sgr_frame_loss_bwd_kernel(int C, int H, int W, sgr_frame_loss_args in, FlWeights wt, SgrGauss11 g,
                          const float* __restrict__ partials, const float* __restrict__ head, LdWork ld,
                          const float* __restrict__ upstream, float* __restrict__ dimg, float* __restrict__ dacc,
                          float* __restrict__ ddepth, float* __restrict__ dobj) {
    __shared__ SsimHalo sp[3];
    __shared__ SsimRows hb[3];
    const int x0 = blockIdx.x * SGR_LS_T, y0 = blockIdx.y * SGR_LS_T;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < W && y < H;
    const size_t plane = (size_t)H * W, cp = (size_t)C * plane, o = (size_t)y * W + x;
    const float up = upstream[0];
    if (dimg) {
        const bool m = inside && (!in.mask || in.mask[o]);
        const float w_ssim = -wt.lambda_dssim;  // the loss holds 1 - ssim
        for (int c = 0; c < C; c++) {
            ssim_stage_partials(threadIdx.x, partials, c, plane, cp, x0, y0, H, W, sp);
            __syncthreads();
            ssim_hpass<3>(threadIdx.x, sp, g, hb);
            __syncthreads();
            if (inside) {
                float out = 0.f;
                if (m) {
                    float f[3];
                    ssim_vpass<3>(hb, g, ty, tx, f);
                    const float xv = in.image[c * plane + o], yv = in.gt[c * plane + o];
                    out = w_ssim * ssim_grad(f[0], f[1], f[2], xv, yv, up / (float)cp);
                    out += wt.w_l1 * up * l1_sign(xv - yv) / head[4];
                }
                dimg[c * plane + o] = out;
            }
            // (the next channel writes sp after every lane passed the second barrier, hb after its first)
        }
    }
    if (!inside) return;
    const float n = (float)H * (float)W;
    float gd = 0.f, ga = 0.f;
    if (in.lidar_depth && (dacc || ddepth))
        lidar_grad(ld.key[o], head, in.depth[o], in.acc[o], in.lidar_depth[o], up * wt.lambda_lidar, gd, ga);
    if (ddepth) ddepth[o] = gd;
    if (dacc) {
        if (in.sky_mask) {
            const float xa = in.acc[o];
            if (bce_clamp_passes(xa)) ga += bce_grad(0, xa, in.sky_mask[o] != 0) * (up * wt.lambda_sky * wt.sky_scale / n);
        }
        dacc[o] = ga;
    }
    if (dobj) {
        const float xa = in.acc_obj[o];
        float go = 0.f;
        if (bce_clamp_passes(xa)) go = bce_grad(1, xa, in.obj_bound[o] != 0) * (up * wt.lambda_reg / n);
        dobj[o] = go;
    }
}

// ---- mse / psnr (loss_utils.py:61-78) ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sgr_mse_map_kernel(int C, size_t plane, const float* __restrict__ a, const float* __restrict__ b,
                   const uint8_t* __restrict__ mask, float* __restrict__ block_sums) {
    __shared__ float lds4[4];
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    float s = 0.f, n = 0.f;
    if (p < plane && (!mask || mask[p])) {
        for (int c = 0; c < C; c++) {
            const float d = a[c * plane + p] - b[c * plane + p];
            s += d * d;
        }
        n = (float)C;
    }
    const float ss = block_sum_256(s, lds4);
    __syncthreads();
    const float nn = block_sum_256(n, lds4);
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = ss;
        block_sums[gridDim.x + blockIdx.x] = nn;
    }
}
__global__ void __launch_bounds__(256)
sgr_mse_finish_kernel(const float* __restrict__ block_sums, size_t nblocks, float* __restrict__ out) {
    __shared__ float lds4[4];
    float tot[2];
    fl_totals(block_sums, nblocks, tot, lds4);
    if (threadIdx.x == 0) {
        const float mse = tot[0] / tot[1];
        out[0] = mse;
        out[1] = fl_psnr(mse);
        out[2] = tot[1];
    }
}

static int fl_check(int C, int H, int W, const sgr_frame_loss_args* a, bool& sky, bool& obj, bool& lidar) {
    if (const int rc = ls_check_dims(C, H, W)) return rc;
    if (!a || !a->image || !a->gt) return sgr_set_error(SGR_E_INVALID, "args, image and gt are required");
    if (a->sky_mask && !a->acc) return sgr_set_error(SGR_E_INVALID, "the sky term needs acc and sky_mask");
    if (!a->acc_obj != !a->obj_bound) return sgr_set_error(SGR_E_INVALID, "the object term needs acc_obj and obj_bound");
    if (!a->depth != !a->lidar_depth) return sgr_set_error(SGR_E_INVALID, "the LiDAR term needs depth and lidar_depth");
    if (a->depth && !a->acc) return sgr_set_error(SGR_E_INVALID, "the LiDAR term needs acc");
    if (a->acc && !a->sky_mask && !a->depth) return sgr_set_error(SGR_E_INVALID, "acc without sky_mask or depth: no term reads it");
    sky = a->sky_mask != nullptr;
    obj = a->obj_bound != nullptr;
    lidar = a->lidar_depth != nullptr;
    return 0;
}
static FlWeights fl_weights(const sgr_frame_loss_args* a) {
    return FlWeights{a->w_l1, a->lambda_dssim, a->lambda_sky, a->sky_scale, a->lambda_reg, a->lambda_depth_lidar};
}

extern "C" {

size_t sgr_frame_loss_saved_bytes(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    char* base = (char*)4096;
    const FlSaved s = fl_carve(base, (size_t)C, (size_t)H * W);
    return (size_t)((char*)s.ld.key - base) + ld_work_bytes((size_t)H * W) + 256;  // + 256: the pointer is re-aligned
}

int sgr_frame_loss_finish_span(void) { return SGR_FL_FINISH_SPAN; }

size_t sgr_frame_loss_workspace_floats(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    const dim3 g = tile_grid(1, H, W);
    return (size_t)SGR_FL_SUMS * g.x * g.y;
}

int sgr_frame_loss_forward(int C, int H, int W, const sgr_frame_loss_args* args, float* terms, char* saved,
                           float* workspace, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    bool sky, obj, lidar;
    if (const int rc = fl_check(C, H, W, args, sky, obj, lidar)) return rc;
    if (!terms || !saved || !workspace) return sgr_set_error(SGR_E_INVALID, "terms, saved and workspace are required");
    const FlSaved s = fl_carve((char*)sgr_align_up((size_t)saved, 256), (size_t)C, (size_t)H * W);
    const dim3 grid = tile_grid(1, H, W);
    const size_t nblocks = (size_t)grid.x * grid.y;
    if (lidar)  // hist [4][256] and state [16] lie back to back (ld_carve): one clear
        SGR_HIP(hipMemsetAsync(s.ld.hist, 0, (size_t)((char*)(s.ld.state + 16) - (char*)s.ld.hist), stream));
    sgr_frame_loss_map_kernel<<<grid, 256, 0, stream>>>(C, H, W, *args, ssim_window(), s.partials, s.ld, workspace);
    if (lidar) sgr_lidar_select_launch(H * W, s.ld, args->keep, s.head, stream);
    sgr_frame_loss_finish_kernel<<<1, 256, 0, stream>>>(C, H, W, workspace, nblocks, fl_weights(args), sky, obj, lidar, s.head,
                                                        terms);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_frame_loss_backward(int C, int H, int W, const sgr_frame_loss_args* args, const float* terms, const char* saved,
                            float* workspace, const float* upstream, float* dL_dimage, float* dL_dacc, float* dL_ddepth,
                            float* dL_dacc_obj, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    bool sky, obj, lidar;
    if (const int rc = fl_check(C, H, W, args, sky, obj, lidar)) return rc;
    if (!terms || !saved || !upstream) return sgr_set_error(SGR_E_INVALID, "terms, saved and upstream are required");
    if (dL_dacc && !sky && !lidar) return sgr_set_error(SGR_E_INVALID, "dL_dacc: neither the sky nor the LiDAR term is on");
    if (dL_ddepth && !lidar) return sgr_set_error(SGR_E_INVALID, "dL_ddepth: the LiDAR term is off");
    if (dL_dacc_obj && !obj) return sgr_set_error(SGR_E_INVALID, "dL_dacc_obj: the object term is off");
    if (!dL_dimage && !dL_dacc && !dL_ddepth && !dL_dacc_obj) return 0;
    const FlSaved s = fl_carve((char*)sgr_align_up((size_t)const_cast<char*>(saved), 256), (size_t)C, (size_t)H * W);
    sgr_frame_loss_bwd_kernel<<<tile_grid(1, H, W), 256, 0, stream>>>(C, H, W, *args, fl_weights(args), ssim_window(), s.partials,
                                                                     s.head, s.ld, upstream, dL_dimage, dL_dacc, dL_ddepth,
                                                                     dL_dacc_obj);
    SGR_HIP(hipGetLastError());
    return 0;
}

size_t sgr_mse_workspace_floats(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * (((size_t)H * W + 255) / 256);
}

int sgr_mse_forward(int C, int H, int W, const float* a, const float* b, const uint8_t* mask, float* out, float* workspace,
                    void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = ls_check_dims(C, H, W)) return rc;
    if (!a || !b || !out || !workspace) return sgr_set_error(SGR_E_INVALID, "a, b, out and workspace are required");
    const size_t plane = (size_t)H * W, nblocks = (plane + 255) / 256;
    sgr_mse_map_kernel<<<(unsigned)nblocks, 256, 0, stream>>>(C, plane, a, b, mask, workspace);
    sgr_mse_finish_kernel<<<1, 256, 0, stream>>>(workspace, nblocks, out);
    SGR_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
