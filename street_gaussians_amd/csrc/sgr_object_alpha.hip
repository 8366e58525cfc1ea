// sgr_object_alpha.hip -- the OBJECT-ALPHA head of the training render (include/sgr_object_alpha.h): the alpha image of
// Gaussians [split, P) blended alone, and the partial-gradient rows of its backward, both from the composite's finished
// tile lists.  What the reference gets from a second whole render + backward per training iteration (render_object,
// lib/models/street_gaussian_renderer.py:58-72, called from train.py:114-122) is two launches beside the shipped path here;
// the shipped row sum and per-Gaussian backward (sgr_gauss_bwd.hip) consume the rows unchanged.
//
// Why the lists can be shared: see sgr_blend_layers.hip.  Both kernels have the shape of sgr_tile_walk.h and take their
// arithmetic from it, and walk only the entries with g >= split that are not marked dead: the others are skipped without
// a record fetch.
//
// FORWARD (sgr_object_alpha_fwd_kernel): layer 1 of sgr_blend_layers_kernel without colour (no r[2] fetch, no background)
// -- the same sgr_walk_pairs and blend step, so the alpha image is bit for bit the layer kernel's acc_rest, i.e. the alpha
// of a forward over the subset alone -- plus, per pixel, the 1-based position inside the tile's range of the last entry
// that was blended: the layer's n_contrib (forward.cu:431-445).
//
// BACKWARD (sgr_object_alpha_bwd_kernel): the alpha part of backward.cu:505-640, back to front over the positions below
// the tile's largest recorded position, 128 per round.  Per visit the blend backward's power, G (sgr_G_bwd: with the parity
// mode's guard at the 1/255 threshold) and alpha from sgr_walk_pairs, its hit test (sgr_bwd_hit), v_rcp_f32 for
// T / (1 - alpha) and the moments of G * dL/dopa (sgr_bwd_moments); which quadrants visit an entry is the geometric cull, redone (the shipped kernel's NO_HITS path: the lanes that take part
// are decided per pixel, so the cull only removes visits without any).  No global atomics and no LDS float atomics: a
// visit's seven sums are reduced across the wave (sgr_wave_reduce_fold) and stored into the slot's row OF THAT QUADRANT
// (one writer per element); after the round one thread per slot adds the rows of the quadrants that visited it, in
// quadrant order, turns the moments into gradients (sgr_moments_to_grads) and writes the row once.
#include "sgr_tile_walk.h"
#include "sgr_launch.h"
#include "sgr_reduce.h"

#define SGR_OA_BATCH 128  // list positions per round of the backward (20 KB of LDS: occupancy is set by registers)

template <bool EXACT>
__global__ void __launch_bounds__(SGR_TILE_THREADS) __attribute__((amdgpu_waves_per_eu(8)))
sgr_object_alpha_fwd_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, int gy,
                            const float4* __restrict__ rec, uint32_t split, float* __restrict__ out_alpha,
                            uint32_t* __restrict__ out_last) {
    // fused multiply-adds are written out (fmaf), as in the forward whose bits this kernel reproduces
#pragma clang fp contract(off)
    __shared__ float4 sA[SGR_TILE_THREADS];  // {x, y, -, -}
    __shared__ float4 sB[SGR_TILE_THREADS];  // {qa, qb, qc, opacity}
    __shared__ uint64_t sBits[4][4];       // [quadrant][chunk of 64 entries]: survivors of the cull
    __shared__ uint32_t sDone[4];          // [wave]: all 64 pixels are finished

    SgrTilePixel tp;
    if (!sgr_tile_pixel(tp, gx, gy, ranges)) return;
    const int tid = tp.tid, lane = tp.lane, wave = tp.wave;
    const bool inside = tp.inside(W, H);
    const uint2 range = ranges[tp.tile];

    float T = 1.0f, Wt = 0.f;
    uint32_t last = 0;
    // finished pixels (outside the image, or T exhausted): the wave's scalar lane mask and the per-lane alpha threshold that
    // becomes +inf (sgr_blend_begin)
    uint64_t done_mask = sgr_uniform_u64(__builtin_amdgcn_ballot_w64(!inside));
    float thr = inside ? SGR_ALPHA_MIN : __builtin_inff();
    const float tx0 = tp.tx0(), ty0 = tp.ty0();

    for (uint32_t base = range.x; base < range.y; base += SGR_TILE_THREADS) {
        // tile-wide state; also the barrier that protects LDS reuse
        if (lane == 0) sDone[wave] = done_mask == ~0ull ? 1u : 0u;
        __syncthreads();
        if (sDone[0] & sDone[1] & sDone[2] & sDone[3]) break;

        const uint32_t idx = base + tid;
        uint32_t mask4 = 0;
        const uint32_t g = idx < range.y ? point_list[idx] : SGR_DEAD;
        // dead entries (marked-list mode) and entries of the other layer: skipped without a fetch
        if (!(g & SGR_DEAD) && g >= split) {
            const float4* r = rec + 4 * (size_t)g;
            const float4 a = r[0];
            const float4 b = r[1];
            sA[tid] = a;
            sB[tid] = sgr_stage_conic_mode<EXACT>(b);
            mask4 = sgr_quadrant_mask(a, b, tx0, ty0);
        }
        sgr_store_cull_ballots(mask4, lane, wave, sBits);
        __syncthreads();

        const uint32_t pos0 = base - range.x + 1u;  // 1-based position of slot 0 inside the tile's range
        if (done_mask != ~0ull) {
            for (int chunk = 0; chunk < 4; chunk++) {
                uint64_t m = sgr_uniform_u64(sBits[wave][chunk]);
                sgr_walk_pairs<EXACT, false>(m, chunk, sA, sB, tp.pxf, tp.pyf, [&](const SgrVisit& v) __attribute__((always_inline)) {
                    SgrBlendStep<true> b;
                    if (!sgr_blend_begin(b, T, thr, v.power, v.alpha)) return;
                    Wt += b.w;
                    sgr_blend_end(b, T, thr, done_mask, m);
                    last = b.sel(pos0 + (uint32_t)v.j, last);
                });
                if (done_mask == ~0ull) break;
            }
        }
    }

    if (inside) {
        const size_t pix_id = (size_t)W * tp.py + tp.px;
        out_alpha[pix_id] = Wt;
        out_last[pix_id] = last;
    }
}

template <bool EXACT>
__global__ void __launch_bounds__(SGR_TILE_THREADS) __attribute__((amdgpu_waves_per_eu(8)))
sgr_object_alpha_bwd_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, int gy,
                            const float4* __restrict__ rec, const uint32_t* __restrict__ u0, const uint64_t* __restrict__ tmask,
                            uint32_t split, const float* __restrict__ layer_alpha, const uint32_t* __restrict__ layer_last,
                            const float* __restrict__ dL_dlayer_alpha, float* __restrict__ partials, int row_stride,
                            uint8_t* __restrict__ touched, uint32_t row_limit) {
    // every fused multiply-add is written out, as in sgr_blend_bwd.hip
#pragma clang fp contract(off)
    constexpr int BATCH = SGR_OA_BATCH, NCH = BATCH / 64;
    __shared__ float4 sA[BATCH];  // {x, y, bits of the instance's partial-row index u, -}
    __shared__ float4 sB[BATCH];  // {qa, qb, qc, opacity}
    __shared__ uint64_t sBits[4][NCH];  // [quadrant][chunk]: survivors of the cull
    __shared__ uint64_t sVis[4][NCH];   // [quadrant][chunk]: the slots whose visit had a hitting pixel (= wrote its row)
    __shared__ int sMax[4];
    // [quadrant][slot][S gx, S gy, S abs, S gxx, S gxy, S gyy, S Gd, -]: one writer per element, read only where sVis says so
    __shared__ __attribute__((aligned(16))) float sAcc[4][BATCH][8];

    SgrTilePixel tp;
    if (!sgr_tile_pixel(tp, gx, gy, ranges)) return;
    const int tid = tp.tid, lane = tp.lane, wave = tp.wave;
    const uint32_t tx = tp.tx, ty = tp.ty;
    const bool inside = tp.inside(W, H);
    const size_t pix_id = (size_t)W * tp.py + tp.px;
    const uint2 range = ranges[tp.tile];
    const int len = (int)(range.y - range.x);

    // backward.cu:466-500 for the layer: T_final = 1 - alpha, the layer's own last contributor
    float T = inside ? (1.0f - layer_alpha[pix_id]) : 0.0f;
    // (a position beyond the list cannot come from this frame's forward: clamped, so that nothing outside the range is read)
    const int lastc = inside ? min((int)layer_last[pix_id], len) : 0;
    const float dLdA = inside ? dL_dlayer_alpha[pix_id] : 0.0f;
    float accA = 0.f, last_alpha = 0.f;
    const SgrNdcScale ks = sgr_ndc_scale(W, H, EXACT);
    const float kx = ks.kx, ky = ks.ky;

    int mx = lastc;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) sMax[wave] = mx;
    sgr_lds_barrier();
    const int maxc = max(max(sMax[0], sMax[1]), max(sMax[2], sMax[3]));
    const float tx0 = tp.tx0(), ty0 = tp.ty0();
    // sgr_wave_reduce_fold<8>: the first lane of banks 0 and 2 of every 16-lane row k holds the wave total of value
    // 4 t + {0, 2, 1, 3}[k], t = 0 for bank 0 and 1 for bank 2 -- eight lanes, eight values
    const int fold_bank = (lane >> 2) & 3;
    const bool fold_writer = (lane & 3) == 0 && (fold_bank & 1) == 0;
    const int fold_val = 4 * (fold_bank >> 1) + ((0x3120 >> ((lane >> 4) * 4)) & 3);

    for (int hi = maxc - 1; hi >= 0; hi -= BATCH) {
        // slot t of this round holds list position hi - t (descending: back to front)
        sgr_lds_barrier();  // previous round fully consumed before LDS is overwritten
        const bool stager = tid < BATCH;  // whole waves
        const int pos = stager ? hi - tid : -1;
        uint32_t mask4 = 0;
        const uint32_t g = pos >= 0 ? point_list[range.x + (uint32_t)pos] : SGR_DEAD;
        if (!(g & SGR_DEAD) && g >= split) {
            const float4* r = rec + 4 * (size_t)g;
            const float4 a = r[0];
            const float4 b = r[1];
            const float4 d4 = r[3];
            sB[tid] = sgr_stage_conic_mode<EXACT>(b);
            const bool live = sgr_stage_bwd_row(a, d4, g, tx, ty, u0, tmask, row_limit, sA[tid]);
            mask4 = sgr_quadrant_mask(a, b, tx0, ty0);
            if (!live) mask4 = 0;
        }
        if (stager) sgr_store_cull_ballots(mask4, lane, wave, sBits);
        sgr_lds_barrier();

        uint64_t vis = 0;  // the slots of the current chunk this wave wrote a row for (scalar)
        auto process = [&](const SgrVisit& vt) __attribute__((always_inline)) {
            const int j = vt.j;
            const float4 q = vt.q;
            const float dx = vt.dx, dy = vt.dy, power2 = vt.power, G = vt.G, alpha = vt.alpha;
            const SgrBwdHit h = sgr_bwd_hit(hi - j, lastc, power2, alpha);  // hi - j: 0-based list position
            if (h.hm == 0) return;  // no pixel takes part: no row
            vis = sgr_bitset1(vis, j & 63);
            float Gd = 0.0f;  // G * dL/dopa: zero off the hit lanes
            if (h.hit) {
                const float oma = 1.0f - alpha;
                T = T * __builtin_amdgcn_rcpf(oma);  // T = T / (1 - alpha) (backward.cu:547), as the blend backward
                accA = fmaf(1.0f - last_alpha, accA, last_alpha);
                last_alpha = alpha;
                Gd = G * (((1.0f - accA) * dLdA) * T);
            }
            float v[8];
            sgr_bwd_moments(Gd, q.x, q.y, q.z, dx, dy, kx, ky, v);
            v[7] = 0.0f;
            float r[1];
            sgr_wave_reduce_fold<8>(v, r);
            if (fold_writer) sAcc[wave][j][fold_val] = r[0];
        };
        for (int chunk = 0; chunk < NCH; chunk++) {
            uint64_t m = sgr_uniform_u64(sBits[wave][chunk]);
            sgr_walk_pairs<EXACT, true>(m, chunk, sA, sB, tp.pxf, tp.pyf, process);
            if (lane == 0) sVis[wave][chunk] = vis;
            vis = 0;
        }
        sgr_lds_barrier();
        // One row per (tile, instance) some quadrant was asked to visit, written exactly once (a row of zeros when every
        // visit found no pixel): the rows of the quadrants that visited the slot, added in quadrant order
        if (mask4 != 0) {
            float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if ((sVis[q][tid >> 6] >> (tid & 63)) & 1ull) {
                    const float4* src = reinterpret_cast<const float4*>(&sAcc[q][tid][0]);
                    const float4 t0 = src[0], t1 = src[1];
                    s[0] += t0.x; s[1] += t0.y; s[2] += t0.z; s[3] += t0.w;
                    s[4] += t1.x; s[5] += t1.y; s[6] += t1.z;
                }
            }
            const float4 qq = sB[tid];
            const uint32_t u = __float_as_uint(sA[tid].z);
            touched[u] = 1;
            float4* row = reinterpret_cast<float4*>(partials + (size_t)u * row_stride);
            float4 r0 = make_float4(s[0], s[1], s[2], s[3]), r1 = make_float4(s[4], s[5], s[6], 0.0f);
            sgr_moments_to_grads(qq.x, qq.y, qq.z, qq.w, kx, ky, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y);
            row[0] = r0;  // dL/dmean2D.x, .y, sum |x| + |y|, dL/dconic.x
            row[1] = r1;  // dL/dconic.y, .w, dL/dopacity, colour r
            row[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);    // colour g, b, depth, padding
        }
    }
}

void sgr_launch_object_alpha_fwd(bool exact, const SgrTileLists& tl, int split, float* out_alpha, uint32_t* out_last, hipStream_t s) {
    const unsigned tiles = tl.blocks();
    if (tiles) sgr_with_flag(exact, [&](auto E) {
        sgr_object_alpha_fwd_kernel<E><<<tiles, SGR_TILE_THREADS, 0, s>>>(tl.ranges, tl.point_list, tl.W, tl.H, tl.gx, tl.gy, tl.rec, (uint32_t)split, out_alpha, out_last);
    });
}

void sgr_launch_object_alpha_bwd(bool exact, const SgrTileLists& tl, const uint32_t* u0, const uint64_t* tmask, int split,
                                 const float* layer_alpha, const uint32_t* layer_last, const float* dL_dlayer_alpha,
                                 float* partials, int row_stride, uint8_t* touched, uint32_t row_limit, hipStream_t s) {
    const unsigned tiles = tl.blocks();
    if (tiles) sgr_with_flag(exact, [&](auto E) {
        sgr_object_alpha_bwd_kernel<E><<<tiles, SGR_TILE_THREADS, 0, s>>>(tl.ranges, tl.point_list, tl.W, tl.H, tl.gx, tl.gy, tl.rec, u0, tmask, (uint32_t)split,
                                                                        layer_alpha, layer_last, dL_dlayer_alpha, partials, row_stride, touched, row_limit);
    });
}
