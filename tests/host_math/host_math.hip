// TEST INFRASTRUCTURE.  Host (x86) build of the __host__ __device__ maths in
// street_gaussians_amd/csrc/sgr_math.h, sgr_pergauss.h, sgr_quat.h, sgr_ssim.h and sgr_radix.h, so the formulas the gfx950
// kernels run can be checked against the oracle without a GPU (tests/test_host_math.py, tests/test_pergauss_host_cpu.py,
// tests/test_quat_cpu.py, tests/test_ssim_host_cpu.py, tests/test_radix_host_cpu.py).
// Built with `hipcc -x hip --cuda-host-only`; never loaded by the product.
#include "../../street_gaussians_amd/csrc/sgr_math.h"
#include "../../street_gaussians_amd/csrc/sgr_pergauss.h"
#include "../../street_gaussians_amd/csrc/sgr_quat.h"
#include "../../street_gaussians_amd/csrc/sgr_ssim.h"
#include "../../street_gaussians_amd/csrc/sgr_radix.h"

// forward staging of one lane as sgr_ssim_fwd_kernel does it (the kernels keep theirs: they differ in how they read the mask)
static void ssim_stage_images(int tid, const float* p1, const float* p2, const unsigned char* mask, int x0, int y0, int H, int W,
                              SsimHalo& sx, SsimHalo& sy) {
    for (int e = tid; e < SGR_LS_IN * SGR_LS_IN; e += 256) {
        const int r = e / SGR_LS_IN, q = e - r * SGR_LS_IN;
        const int y = y0 + r - SGR_LS_R, x = x0 + q - SGR_LS_R;
        float a = 0.f, b = 0.f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t o = (size_t)y * W + x;
            if (!mask || mask[o]) { a = p1[o]; b = p2[o]; }
        }
        sx[r][q] = a;
        sy[r][q] = b;
    }
}

static SgrCam make_cam(const float* view, const float* proj, const float* campos, float tanx, float tany, int W, int H,
                       float mod) {
    SgrCam c;
    for (int i = 0; i < 16; i++) { c.view[i] = view[i]; c.proj[i] = proj[i]; }
    for (int i = 0; i < 3; i++) c.campos[i] = campos ? campos[i] : 0.f;
    c.tan_fovx = tanx; c.tan_fovy = tany;
    c.focal_y = H / (2.0f * tany);
    c.focal_x = W / (2.0f * tanx);
    c.W = W; c.H = H;
    c.gx = (W + 15) / 16; c.gy = (H + 15) / 16;
    c.scale_modifier = mod;
    return c;
}

// ---- csrc/sgr_radix.h (tests/test_radix_host_cpu.py): digit counts -> first slots as the radix kernels run it, owner by owner.
// cnt [waves][bins] in place; the exclusive scan of the owners' sums (the kernels' wave / block scan) is this harness's own.
// first[d] = what per_bin reports for digit d (0xffffffff where it was not called).  Returns 0 for a (waves, bins, bins per
// owner) no kernel instantiates.
template <int WAVES, int NB, int BPO>
static int bin_starts_run(int owners, unsigned* cnt_flat, unsigned* first) {
    auto cnt = reinterpret_cast<uint32_t (*)[NB]>(cnt_flat);
    auto c = new uint32_t[owners][BPO][WAVES];
    uint32_t* sum = new uint32_t[owners];
    for (int o = 0; o < owners; o++) sum[o] = sgr_bin_counts<WAVES, NB, BPO>(cnt, o, c[o]);
    uint32_t run = 0;
    for (int o = 0; o < owners; o++) {
        sgr_bin_starts<WAVES, NB, BPO>(cnt, o, c[o], run, [&](int bin, int j, uint32_t start) { (void)j; first[bin] = start; });
        run += sum[o];
    }
    delete[] c;
    delete[] sum;
    return 1;
}

extern "C" {

void hm_forward(int P, int D, int M, const float* means, const float* scales, const float* rots, const float* opac,
                const float* shs, const float* view, const float* proj, const float* campos, float tanx, float tany,
                int W, int H, float mod, int* radii, float* means2D, float* depths, float* conic, float* cov3D,
                unsigned* tiles, float* rgb, unsigned char* clamped, float* extents) {
    const SgrCam cam = make_cam(view, proj, campos, tanx, tany, W, H, mod);
    for (int i = 0; i < P; i++) {
        radii[i] = 0; tiles[i] = 0;
        sgr_cov3d(scales + 3 * i, mod, rots + 4 * i, cov3D + 6 * i);
        SgrProj pr = sgr_project(means + 3 * i, cov3D + 6 * i, cam);
        depths[i] = pr.depth;
        if (!pr.ok) continue;
        radii[i] = pr.radius;
        tiles[i] = (pr.rx1 - pr.rx0) * (pr.ry1 - pr.ry0);
        means2D[2 * i] = pr.px; means2D[2 * i + 1] = pr.py;
        conic[3 * i] = pr.con_x; conic[3 * i + 1] = pr.con_y; conic[3 * i + 2] = pr.con_z;
        sgr_extent(opac[i], pr.cov_a, pr.cov_c, pr.con_x, pr.con_y, pr.con_z, extents[2 * i], extents[2 * i + 1]);
        // SH colour: the calls sgr_preprocess_kernel makes (sgr_pergauss.h)
        float dor[3], dir[3], Y[16];
        sgr_view_dir<true>(means + 3 * i, cam.campos, dor, dir);
        sgr_sh_basis(D, dir[0], dir[1], dir[2], Y);
        float c[3] = {0, 0, 0};
        sgr_sh_fold_row(shs + (size_t)i * M * 3, Y, (D + 1) * (D + 1), c);
        uint32_t cl;
        sgr_sh_finish(c, cl);
        for (int ch = 0; ch < 3; ch++) {
            clamped[3 * i + ch] = (cl >> ch) & 1u;
            rgb[3 * i + ch] = c[ch];
        }
    }
}

// per-Gaussian backward from the blend-stage gradients, as sgr_gauss_bwd_kernel composes it
void hm_backward(int P, int D, int M, const float* means, const float* scales, const float* rots, const float* shs,
                 const float* cov3D, const unsigned char* clamped, const int* radii, const float* view, const float* proj,
                 const float* campos, float tanx, float tany, int W, int H, float mod, const float* dmean2D,
                 const float* dconic, const float* dcolor, const float* ddepth, float* dmean3D, float* dcov3D,
                 float* dscale, float* drot, float* dsh) {
    const SgrCam cam = make_cam(view, proj, campos, tanx, tany, W, H, mod);
    for (int i = 0; i < P; i++) {
        if (!(radii[i] > 0)) continue;
        float dmean[3], dcov[6];
        sgr_cov2d_backward(means + 3 * i, cov3D + 6 * i, cam, dconic[4 * i], dconic[4 * i + 1], dconic[4 * i + 3], dcov, dmean);
        sgr_proj_depth_backward(means + 3 * i, cam, dmean2D[3 * i], dmean2D[3 * i + 1], ddepth[i], dmean);
        sgr_cov3d_backward(scales + 3 * i, mod, rots + 4 * i, dcov, dscale + 3 * i, drot + 4 * i);
        float dRGB[3], dor[3], dir[3];
        const uint32_t cl = (clamped[3 * i] ? 1u : 0u) | (clamped[3 * i + 1] ? 2u : 0u) | (clamped[3 * i + 2] ? 4u : 0u);
        sgr_mask_clamped(cl, dcolor + 3 * i, dRGB);
        sgr_view_dir(means + 3 * i, cam.campos, dor, dir);
        float Y[16];
        sgr_sh_basis(D, dir[0], dir[1], dir[2], Y);
        const float* sh = shs + (size_t)i * M * 3;
        float t[16] = {0};
        for (int k = 0; k < (D + 1) * (D + 1); k++)
            for (int ch = 0; ch < 3; ch++) { t[k] += sh[3 * k + ch] * dRGB[ch]; dsh[((size_t)i * M + k) * 3 + ch] = Y[k] * dRGB[ch]; }
        float ddir[3], dm[3];
        sgr_sh_dir_backward(D, dir[0], dir[1], dir[2], t, ddir);
        sgr_dnormvdv(dor, ddir, dm);
        for (int k = 0; k < 3; k++) dmean3D[3 * i + k] = dmean[k] + dm[k];
        for (int k = 0; k < 6; k++) dcov3D[6 * i + k] = dcov[k];
    }
}

// quadrant masks of n splats for the tile whose first pixel is (tx0, ty0)
void hm_quadrant_masks(int n, const float* means2D, const float* conic_opacity, const float* extents, float tx0, float ty0,
                       unsigned* masks) {
    for (int i = 0; i < n; i++) {
        const float4 a = make_float4(means2D[2 * i], means2D[2 * i + 1], extents[2 * i], extents[2 * i + 1]);
        const float4 b = make_float4(conic_opacity[4 * i], conic_opacity[4 * i + 1], conic_opacity[4 * i + 2], conic_opacity[4 * i + 3]);
        masks[i] = sgr_quadrant_mask(a, b, tx0, ty0);
    }
}

// tile masks of n splats over their rects {x0, y0, x1, y1} (tiles), and the two bit utilities the mask needs
void hm_tile_masks(int n, const float* means2D, const float* conic_opacity, const unsigned* rects, unsigned long long* masks) {
    for (int i = 0; i < n; i++)
        masks[i] = sgr_tile_mask(means2D[2 * i], means2D[2 * i + 1], conic_opacity[4 * i], conic_opacity[4 * i + 1],
                                 conic_opacity[4 * i + 2], conic_opacity[4 * i + 3], rects[4 * i], rects[4 * i + 1], rects[4 * i + 2],
                                 rects[4 * i + 3]);
}
void hm_tile_masks_per_tile(int n, const float* means2D, const float* conic_opacity, const unsigned* rects, unsigned long long* masks) {
    for (int i = 0; i < n; i++)
        masks[i] = sgr_tile_mask_per_tile(means2D[2 * i], means2D[2 * i + 1], conic_opacity[4 * i], conic_opacity[4 * i + 1],
                                          conic_opacity[4 * i + 2], conic_opacity[4 * i + 3], rects[4 * i], rects[4 * i + 1],
                                          rects[4 * i + 2], rects[4 * i + 3]);
}
unsigned hm_select_bit(unsigned long long m, unsigned k) { return sgr_select_bit(m, k); }
unsigned hm_row_of(unsigned rect, unsigned tx, unsigned ty, const unsigned* u0, const unsigned long long* tmask, unsigned g) {
    return sgr_row_of(rect, tx, ty, u0, (const uint64_t*)tmask, g);
}

// ---- csrc/sgr_pergauss.h (tests/test_pergauss_host_cpu.py) ----
// slot k of a rect word -> its tile {tx, ty}, with the caller's reciprocal of the rect's width
void hm_slot_tile(unsigned rect, unsigned long long mask, unsigned k, float rcp_w, unsigned* txy) {
    const uint2 t = sgr_slot_tile(rect, (uint64_t)mask, k, rcp_w);
    txy[0] = t.x; txy[1] = t.y;
}
int hm_mark_live(unsigned live_rect, unsigned live_n, unsigned long long mask, unsigned tx, unsigned ty) {
    return sgr_mark_live(live_rect, live_n, (uint64_t)mask, tx, ty) ? 1 : 0;
}
// the preprocess's rect decision per Gaussian of a scene: ref = the reference rect {x0, y0, x1, y1} (zeros when culled),
// out = {rect word, nemit} and the mask as sgr_tight_rect returns it
void hm_tight_rects(int P, const float* means, const float* scales, const float* rots, const float* opac, const float* view,
                    const float* proj, float tanx, float tany, int W, int H, float mod, int tight, unsigned* ref, unsigned* out,
                    unsigned long long* tmask) {
    const SgrCam cam = make_cam(view, proj, nullptr, tanx, tany, W, H, mod);
    for (int i = 0; i < P; i++) {
        float cov3D[6], hx, hy;
        sgr_cov3d(scales + 3 * i, mod, rots + 4 * i, cov3D);
        const SgrProj pr = sgr_project(means + 3 * i, cov3D, cam);
        for (int k = 0; k < 4; k++) ref[4 * i + k] = 0u;
        out[2 * i] = out[2 * i + 1] = 0u;
        tmask[i] = 0ull;
        if (!pr.ok) continue;
        sgr_extent(opac[i], pr.cov_a, pr.cov_c, pr.con_x, pr.con_y, pr.con_z, hx, hy);
        const SgrTightRect t = sgr_tight_rect(pr, hx, hy, opac[i], tight);
        ref[4 * i] = pr.rx0; ref[4 * i + 1] = pr.ry0; ref[4 * i + 2] = pr.rx1; ref[4 * i + 3] = pr.ry1;
        out[2 * i] = t.rect; out[2 * i + 1] = t.nemit;
        tmask[i] = t.tmask;
    }
}
// persistent rows of n indices through a segment map (nseg == 0: identity)
void hm_stat_sink_rows(int nseg, const int* start, const int* count, const int* shift, int n, const int* idx, long long* rows) {
    SgrStatSink sink;
    sink.nseg = nseg;
    for (int s = 0; s < nseg; s++) { sink.start[s] = start[s]; sink.count[s] = count[s]; sink.shift[s] = shift[s]; }
    for (int i = 0; i < n; i++) rows[i] = sgr_stat_sink_row(sink, idx[i]);
}

float hm_power2(float qa, float qb, float qc, float dx, float dy) { return sgr_power2(qa, qb, qc, dx, dy); }
// parity mode: the staged power expression against the reference's own, and the shared-reciprocal quotient for a given
// reciprocal seed (the test perturbs the seed by an ulp either way: the device's v_rcp_f32 is only accurate to 1 ulp)
void hm_power_ref_pair(int n, const float* c, const float* d, float* ref, float* staged) {
    for (int i = 0; i < n; i++) {
        ref[i] = sgr_power_ref(c[3 * i], c[3 * i + 1], c[3 * i + 2], d[2 * i], d[2 * i + 1]);
        staged[i] = sgr_power_ref_staged(-0.5f * c[3 * i], -c[3 * i + 1], -0.5f * c[3 * i + 2], d[2 * i], d[2 * i + 1]);
    }
}
// blend backward, the moments identity: the seven values of n pairs (d = {dx, dy}, Gd) for a conic {cx, cy, cz, opacity}
// staged for the default or the parity mode, and the gradients from their sums s[0..5] (in place)
void hm_bwd_moments(int n, int exact, const float* conic_opacity, const float* d, const float* Gd, int W, int H, float* v) {
    const float4 b = make_float4(conic_opacity[0], conic_opacity[1], conic_opacity[2], conic_opacity[3]);
    const float4 q = exact ? sgr_stage_conic_mode<true>(b) : sgr_stage_conic_mode<false>(b);
    const SgrNdcScale k = sgr_ndc_scale(W, H, exact != 0);
    for (int i = 0; i < n; i++) sgr_bwd_moments(Gd[i], q.x, q.y, q.z, d[2 * i], d[2 * i + 1], k.kx, k.ky, v + 7 * i);
}
void hm_moments_to_grads(int exact, const float* conic_opacity, int W, int H, float* s) {
    const float4 b = make_float4(conic_opacity[0], conic_opacity[1], conic_opacity[2], conic_opacity[3]);
    const float4 q = exact ? sgr_stage_conic_mode<true>(b) : sgr_stage_conic_mode<false>(b);
    const SgrNdcScale k = sgr_ndc_scale(W, H, exact != 0);
    sgr_moments_to_grads(q.x, q.y, q.z, q.w, k.kx, k.ky, s[0], s[1], s[2], s[3], s[4], s[5]);
}
// ---- csrc/sgr_quat.h (tests/test_quat_cpu.py): n rows per call, nc = 1 the f<true> flavour, 0 the default one ----
void hm_quat_mul(int n, int nc, const float* a, const float* b, float* o) {
    for (int i = 0; i < n; i++) {
        const Q4 r = nc ? qmul<true>(qload(a + 4 * i), qload(b + 4 * i)) : qmul(qload(a + 4 * i), qload(b + 4 * i));
        o[4 * i] = r.w; o[4 * i + 1] = r.x; o[4 * i + 2] = r.y; o[4 * i + 3] = r.z;
    }
}
void hm_quat_normalize(int n, int nc, const float* a, float* y, float* norm) {
    for (int i = 0; i < n; i++) {
        const Q4 r = nc ? qnormalize<true>(qload(a + 4 * i), norm[i]) : qnormalize(qload(a + 4 * i), norm[i]);
        y[4 * i] = r.w; y[4 * i + 1] = r.x; y[4 * i + 2] = r.y; y[4 * i + 3] = r.z;
    }
}
void hm_quat_normalize_bwd(int n, int nc, const float* y, const float* norm, const float* dy, const unsigned char* clamped,
                           float* da) {
    for (int i = 0; i < n; i++) {
        const Q4 r = nc ? qnormalize_bwd<true>(qload(y + 4 * i), norm[i], qload(dy + 4 * i), clamped[i] != 0)
                        : qnormalize_bwd(qload(y + 4 * i), norm[i], qload(dy + 4 * i), clamped[i] != 0);
        da[4 * i] = r.w; da[4 * i + 1] = r.x; da[4 * i + 2] = r.y; da[4 * i + 3] = r.z;
    }
}
void hm_quat_to_matrix(int n, int nc, const float* q, float* R, float* qn, float* norm) {
    for (int i = 0; i < n; i++) {
        float M[9];
        Q4 u;
        if (nc) qtomat<true>(qload(q + 4 * i), M, u, norm[i]);
        else qtomat(qload(q + 4 * i), M, u, norm[i]);
        for (int k = 0; k < 9; k++) R[9 * i + k] = M[k];
        qn[4 * i] = u.w; qn[4 * i + 1] = u.x; qn[4 * i + 2] = u.y; qn[4 * i + 3] = u.z;
    }
}
void hm_quat_rot_apply(int n, int nc, const float* R, const float* t, float* x) {  // x <- R x + t, in place
    for (int i = 0; i < n; i++) {
        float v[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
        if (nc) rot_apply<true>(R + 9 * i, t + 3 * i, v);
        else rot_apply(R + 9 * i, t + 3 * i, v);
        x[3 * i] = v[0]; x[3 * i + 1] = v[1]; x[3 * i + 2] = v[2];
    }
}
void hm_quat_rot_pullback(int n, int nc, const float* R, const float* g, float* o) {
    for (int i = 0; i < n; i++) {
        if (nc) rot_pullback<true>(R + 9 * i, g + 3 * i, o + 3 * i);
        else rot_pullback(R + 9 * i, g + 3 * i, o + 3 * i);
    }
}
void hm_quat_dquat_of_R(int n, int nc, const float* q, const float* G, float* d) {
    for (int i = 0; i < n; i++) {
        const Q4 r = nc ? dquat_of_R<true>(qload(q + 4 * i), G + 9 * i) : dquat_of_R(qload(q + 4 * i), G + 9 * i);
        d[4 * i] = r.w; d[4 * i + 1] = r.x; d[4 * i + 2] = r.y; d[4 * i + 3] = r.z;
    }
}

// ---- csrc/sgr_ssim.h (tests/test_ssim_host_cpu.py): the steps sgr_ssim_fwd_kernel / sgr_ssim_bwd_kernel run, lane by lane ----
// mean SSIM of two [C][H][W] images (mask [H][W] or null) and d(mean SSIM)/d img1: per 16x16 tile every step for tid = 0..255
// in sequence (a loop's end stands for the kernel's barrier).  Own text: the forward staging loop and the final mean.
void hm_ssim_tiles(int C, int H, int W, const float* img1, const float* img2, const unsigned char* mask, float* partials,
                   double* ssim, float* grad) {
    static SsimHalo sx, sy, sp[3];
    static SsimRows hb[5];
    const SgrGauss11& g = ssim_window();
    const size_t plane = (size_t)H * W, cp = (size_t)C * plane;
    double sum = 0.0;
    for (int pass = 0; pass < 2; pass++)  // 0: map value and partials of every tile, 1: the gradient from the partial maps
        for (int c = 0; c < C; c++)
            for (int y0 = 0; y0 < H; y0 += SGR_LS_T)
                for (int x0 = 0; x0 < W; x0 += SGR_LS_T) {
                    for (int tid = 0; tid < 256; tid++) {
                        if (pass) ssim_stage_partials(tid, partials, c, plane, cp, x0, y0, H, W, sp);
                        else ssim_stage_images(tid, img1 + c * plane, img2 + c * plane, mask, x0, y0, H, W, sx, sy);
                    }
                    for (int tid = 0; tid < 256; tid++) {
                        if (pass) ssim_hpass<3>(tid, sp, g, hb);
                        else ssim_hpass5(tid, sx, sy, g, hb);
                    }
                    for (int tid = 0; tid < 256; tid++) {
                        const int tx = tid & 15, ty = tid >> 4, x = x0 + tx, y = y0 + ty;
                        if (x >= W || y >= H) continue;
                        const size_t o = c * plane + (size_t)y * W + x;
                        if (pass) {
                            float f[3];
                            ssim_vpass<3>(hb, g, ty, tx, f);
                            const bool m = !mask || mask[(size_t)y * W + x];
                            grad[o] = m ? ssim_grad(f[0], f[1], f[2], img1[o], img2[o], 1.0f / (float)cp) : 0.f;
                        } else {
                            float m5[5], val, part[3];
                            ssim_vpass<5>(hb, g, ty, tx, m5);
                            ssim_point(m5, val, part);
                            for (int k = 0; k < 3; k++) partials[k * cp + o] = part[k];
                            sum += val;
                        }
                    }
                }
    *ssim = sum / (double)cp;
}
void hm_ssim_point(int n, const float* m, float* val, float* part) {
    for (int i = 0; i < n; i++) {
        float m5[5], p[3];
        for (int k = 0; k < 5; k++) m5[k] = m[5 * i + k];
        ssim_point(m5, val[i], p);
        for (int k = 0; k < 3; k++) part[3 * i + k] = p[k];
    }
}

// ---- csrc/sgr_radix.h (tests/test_radix_host_cpu.py): bin_starts_run above, per (waves, bins, bins per owner) of a kernel ----
int hm_bin_starts(int waves, int bins, int owners, int bpo, unsigned* cnt, unsigned* first) {
    for (int d = 0; d < bins; d++) first[d] = 0xffffffffu;
#define HM_BS(W, NB, BPO) if (waves == W && bins == NB && bpo == BPO) return bin_starts_run<W, NB, BPO>(owners, cnt, first)
    HM_BS(4, 32, 1); HM_BS(4, 64, 1); HM_BS(4, 128, 2); HM_BS(4, 256, 4); HM_BS(4, 512, 8);  // the scatter, wave 0's lanes
    HM_BS(4, 256, 1);                                                                         // its one-sweep form, 256 threads
    HM_BS(1, 512, 8);                                                                         // one wave per tile
    HM_BS(8, 512, 1); HM_BS(16, 512, 1);                                                      // one workgroup per tile
#undef HM_BS
    return 0;
}

void hm_div_by_seed(int n, const float* a, const float* b, const float* seed, float* q) {
    for (int i = 0; i < n; i++) {
        const float y0 = seed[i];
        const float y = fmaf(fmaf(-b[i], y0, 1.0f), y0, y0);
        q[i] = sgr_div_by(a[i], b[i], y);
    }
}
}
