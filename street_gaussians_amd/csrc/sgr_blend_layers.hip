// sgr_blend_layers.hip -- the two LAYER images of a frame (include/sgr_layers.h): Gaussians [0, split) and [split, P), each
// blended alone over its own background with its own transmittance, from the composite's finished tile lists.  What the
// reference gets from two more whole forwards (StreetGaussianRenderer.render_background / render_object,
// lib/models/street_gaussian_renderer.py:42-72) is ONE more launch behind sgr_blend_fwd_kernel here.
//
// Why the lists can be shared: the preprocess is per Gaussian, and a tile's (depth, index)-sorted list of a contiguous
// subset is the full frame's list with the other Gaussians taken out.  The two layers never interact, so the walk of a
// 64-entry chunk does not have to interleave them: it walks the chunk's layer-0 survivors in list order, then its layer-1
// survivors in list order -- two straight copies of the forward's walk, each on its own accumulator set, picked by a scalar
// test on one more ballot mask per chunk (entry g >= split).
//
// Shape and arithmetic: sgr_tile_walk.h -- the forward's staging, cull, walk and blend step, on T, three colour sums and the
// alpha sum per pixel and layer (no depth, semantics, n_contrib or hit record: nothing of the composite's buffers is
// written).  A layer image is therefore bit for bit the image of a forward over that subset alone: the colour sums are
// FMAs in both modes, the store is C + T * bg with contraction off, as the forward's.
//
// Termination is per layer (forward.cu:394-396, 431-436): a pixel's layer stops at its own test_T < 0.0001; a wave drops
// the entries of a layer all its 64 pixels have finished; a wave stops when both layers are finished; the tile stops when
// its four waves have.  The composite's transmittance plays no part.  A layer that all FOUR waves have finished is not
// staged any more either: its entries are treated like dead ones (no record fetch), which is what keeps the walk behind an
// opaque background wall cheap while the object layer is still looking for its splats.
#include "sgr_tile_walk.h"
#include "sgr_launch.h"

__device__ __forceinline__ float sgr_layer_out(float v, int clamp) {  // NaN stays NaN, as torch.clamp
    return clamp ? (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v)) : v;
}

template <bool EXACT>
__global__ void __launch_bounds__(SGR_TILE_THREADS) __attribute__((amdgpu_waves_per_eu(8)))
sgr_blend_layers_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, int gy,
                        const float4* __restrict__ rec, uint32_t split, uint32_t P, const float* __restrict__ bg_color,
                        int clamp, float* __restrict__ color0, float* __restrict__ alpha0, float* __restrict__ color1,
                        float* __restrict__ alpha1) {
    // fused multiply-adds are written out (fmaf), as in the forward whose bits this kernel reproduces
#pragma clang fp contract(off)
    __shared__ float4 sA[SGR_TILE_THREADS];  // {x, y, -, -}
    __shared__ float4 sB[SGR_TILE_THREADS];  // {qa, qb, qc, opacity}
    __shared__ float4 sC[SGR_TILE_THREADS];  // {r, g, b, -}
    __shared__ uint64_t sBits[4][4];          // [quadrant][chunk of 64 entries]: survivors of the cull
    __shared__ uint64_t sLayer[4];            // [chunk]: entries of layer 1 (g >= split)
    __shared__ uint32_t sDone[4];             // [wave]: bit l = layer l is finished for all 64 pixels

    SgrTilePixel tp;
    if (!sgr_tile_pixel(tp, gx, gy, ranges)) return;
    const int tid = tp.tid, lane = tp.lane, wave = tp.wave;
    const bool inside = tp.inside(W, H);
    const uint2 range = ranges[tp.tile];

    float Ta = 1.0f, Ca0 = 0.f, Ca1 = 0.f, Ca2 = 0.f, Wa = 0.f;  // layer 0
    float Tb = 1.0f, Cb0 = 0.f, Cb1 = 0.f, Cb2 = 0.f, Wb = 0.f;  // layer 1
    // finished pixels (outside the image, or the layer's T exhausted): the wave's scalar lane mask and the per-lane alpha
    // threshold that becomes +inf (sgr_blend_begin), once per layer
    // (an EMPTY layer -- split == 0 or split == P -- starts finished: it keeps T = 1, sums 0, and does not hold the tile)
    const uint64_t outside = sgr_uniform_u64(__builtin_amdgcn_ballot_w64(!inside));
    uint64_t done_a = split == 0u ? ~0ull : outside, done_b = split >= P ? ~0ull : outside;
    float thr_a = inside ? SGR_ALPHA_MIN : __builtin_inff(), thr_b = thr_a;

    const float tx0 = tp.tx0(), ty0 = tp.ty0();

    // The forward's walk of the set bits of m (list slots chunk * 64 + bit) on one layer's accumulators.
    auto walk = [&](uint64_t m, const int chunk, float& T, float& C0, float& C1, float& C2, float& Wt, float& thr,
                    uint64_t& done_mask) __attribute__((always_inline)) {
        sgr_walk_pairs<EXACT, false>(m, chunk, sA, sB, tp.pxf, tp.pyf, [&](const SgrVisit& v) __attribute__((always_inline)) {
            SgrBlendStep<true> b;
            if (!sgr_blend_begin(b, T, thr, v.power, v.alpha)) return;
            const float4 c = sC[v.j];
            C0 = fmaf(c.x, b.w, C0);
            C1 = fmaf(c.y, b.w, C1);
            C2 = fmaf(c.z, b.w, C2);
            Wt += b.w;
            sgr_blend_end(b, T, thr, done_mask, m);
        });
    };

    for (uint32_t base = range.x; base < range.y; base += SGR_TILE_THREADS) {
        // tile-wide state of the two layers; also the barrier that protects LDS reuse
        if (lane == 0) sDone[wave] = (done_a == ~0ull ? 1u : 0u) | (done_b == ~0ull ? 2u : 0u);
        __syncthreads();
        const uint32_t fin = sDone[0] & sDone[1] & sDone[2] & sDone[3];  // bit l: layer l is finished in the whole tile
        if (fin == 3u) break;

        const uint32_t idx = base + tid;
        uint32_t mask4 = 0;
        const uint32_t g = idx < range.y ? point_list[idx] : SGR_DEAD;
        const bool live = !(g & SGR_DEAD);
        const bool upper = live && g >= split;
        // dead entries (marked-list mode) and entries of a layer no wave has a pixel left for: skipped without a fetch
        if (live && !((fin >> (upper ? 1 : 0)) & 1u)) {
            const float4* r = rec + 4 * (size_t)g;  // one 64-byte line
            const float4 a = r[0];
            const float4 b = r[1];
            sA[tid] = a;
            sB[tid] = sgr_stage_conic_mode<EXACT>(b);
            sC[tid] = r[2];
            mask4 = sgr_quadrant_mask(a, b, tx0, ty0);
        }
        sgr_store_cull_ballots(mask4, lane, wave, sBits);
        {
            const uint64_t m = __ballot(upper);
            if (lane == 0) sLayer[wave] = m;
        }
        __syncthreads();

        if ((done_a & done_b) != ~0ull) {
            for (int chunk = 0; chunk < 4; chunk++) {
                const uint64_t m = sgr_uniform_u64(sBits[wave][chunk]);
                const uint64_t up = sgr_uniform_u64(sLayer[chunk]);
                const uint64_t ma = done_a == ~0ull ? 0ull : (m & ~up);
                const uint64_t mb = done_b == ~0ull ? 0ull : (m & up);
                if (ma) walk(ma, chunk, Ta, Ca0, Ca1, Ca2, Wa, thr_a, done_a);
                if (mb) walk(mb, chunk, Tb, Cb0, Cb1, Cb2, Wb, thr_b, done_b);
                if ((done_a & done_b) == ~0ull) break;
            }
        }
    }

    if (inside) {
        const size_t pix_id = (size_t)W * tp.py + tp.px;
        const size_t plane = (size_t)H * W;
        const float b0 = bg_color[0], b1 = bg_color[1], b2 = bg_color[2];
        color0[pix_id] = sgr_layer_out(Ca0 + Ta * b0, clamp);
        color0[plane + pix_id] = sgr_layer_out(Ca1 + Ta * b1, clamp);
        color0[2 * plane + pix_id] = sgr_layer_out(Ca2 + Ta * b2, clamp);
        alpha0[pix_id] = Wa;
        color1[pix_id] = sgr_layer_out(Cb0 + Tb * b0, clamp);
        color1[plane + pix_id] = sgr_layer_out(Cb1 + Tb * b1, clamp);
        color1[2 * plane + pix_id] = sgr_layer_out(Cb2 + Tb * b2, clamp);
        alpha1[pix_id] = Wb;
    }
}

// P == 0 (street_gaussian_renderer.py:138-151): both layers are the background colour with alpha 0.
__global__ void __launch_bounds__(256) sgr_layers_fill_kernel(size_t N, const float* __restrict__ bg_color, int clamp,
                                                              float* __restrict__ color0, float* __restrict__ alpha0,
                                                              float* __restrict__ color1, float* __restrict__ alpha1) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float v = sgr_layer_out(bg_color[ch], clamp);
        color0[ch * N + i] = v;
        color1[ch * N + i] = v;
    }
    alpha0[i] = 0.0f;
    alpha1[i] = 0.0f;
}

void sgr_launch_blend_layers(bool exact, const SgrTileLists& tl, int split, int P, const float* bg, int clamp,
                             float* const color[2], float* const alpha[2], hipStream_t s) {
    const unsigned tiles = tl.blocks();
    if (tiles) sgr_with_flag(exact, [&](auto E) {
        sgr_blend_layers_kernel<E><<<tiles, SGR_TILE_THREADS, 0, s>>>(tl.ranges, tl.point_list, tl.W, tl.H, tl.gx, tl.gy, tl.rec, (uint32_t)split,
                                                                    (uint32_t)P, bg, clamp, color[0], alpha[0], color[1], alpha[1]);
    });
}

void sgr_launch_layers_fill(int W, int H, const float* bg, int clamp, float* const color[2], float* const alpha[2], hipStream_t s) {
    const size_t N = (size_t)W * H;
    if (N == 0) return;
    sgr_layers_fill_kernel<<<(unsigned)((N + 255) / 256), 256, 0, s>>>(N, bg, clamp, color[0], alpha[0], color[1], alpha[1]);
}
