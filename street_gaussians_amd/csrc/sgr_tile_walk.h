// sgr_tile_walk.h -- the walk of a tile's depth-sorted list that every blend kernel shares: sgr_blend_fwd.hip,
// sgr_blend_layers.hip, sgr_object_alpha.hip (forward and backward) and sgr_blend_bwd.hip.
//
// Shape (CDNA4): one 16x16 tile per 256-thread workgroup, one wave64 per 8x8 pixel QUADRANT (compact footprint, so a whole
// wave can skip a splat).  The list is staged through LDS a batch at a time: every staging lane gathers one record,
// pre-scales the conic and tests the splat's conservative alpha >= 1/255 box against the four quadrants; four wave ballots
// turn the tests into one 64-bit survivor mask per (quadrant, 64-entry chunk), and each wave walks only the set bits of its
// own masks, reading the survivor's record from LDS as a broadcast.
//
// RULE: a kernel that promises bit equality with the forward or the backward (a layer image = the forward over the subset,
// the object-alpha rows = the subset render's backward) takes its arithmetic from HERE -- the staged conic, power, G, the
// alpha cut, the order of two visits, the blend step -- and adds only its own sums.  Everything is inlined into the calling
// kernel, whose `#pragma clang fp contract(off)` and source order of float operations these functions keep.
#ifndef SGR_TILE_WALK_H
#define SGR_TILE_WALK_H
#include "sgr_pergauss.h"  // sgr_row_of

#define SGR_TILE_THREADS 256
#ifndef SGR_EXACT_TRIM
#define SGR_EXACT_TRIM 1  // parity mode: sgr_expf_ref / sgr_div_by instead of the library's expf and `/` (same bits, sgr_math.h)
#endif
// Parity mode, backward (round 5).  What north_star asks of the gradients is rel 1e-4, not the reference's bits -- those are
// asked of the tile / bin indices and met by the forward, whose alpha test decides them.  SGR_EXACT_BWD_FAST=1: the backward
// of the parity mode keeps the reference's own power expression (cancellation in it is what can cost digits) but takes
// G = exp(power) from v_exp_f32 and T / (1 - alpha) from the reciprocal, like the default mode -- EXCEPT that a visit with any
// pixel whose alpha lands within 4e-6 (relative) of the 1/255 threshold recomputes G with the accurate expf for the whole
// wave (a wave-uniform branch, taken about once in 10^4 visits): every blend / skip decision is therefore the forward's, and
// what differs from the all-exact backward is rounding-level (<= 4e-7 relative in G, <= 1 ulp per layer in T).
#ifndef SGR_EXACT_BWD_FAST
#define SGR_EXACT_BWD_FAST 1  // 0: every function of the backward with the reference's bits (A/B: tools/build_variant.py)
#endif
#ifndef SGR_EXACT_BWD_GUARD
#define SGR_EXACT_BWD_GUARD 1  // 0 only for tools/valu_model.py (a static count of the loop without its rare branch)
#endif

// lane in m ? a : b, the lane mask in a scalar register pair (v_cndmask_b32_e64 with an SGPR-pair mask: 4.6 cycles per wave
// instruction measured, against 23 for back-to-back selects on VCC, tools/ubench/valu_rates.hip)
__device__ __forceinline__ float sgr_sel_mask(uint64_t m, float a, float b) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
    return r;
}

// x, through an empty volatile asm: a statement the optimiser may not execute speculatively.  An `if` on a wave-uniform
// condition whose only statement assigns sgr_keep_branch(...) stays a scalar branch around that arithmetic; without it
// hipcc computes both arms on every lane and selects (v_cndmask), which costs a loop the skipped arm on every trip.
__device__ __forceinline__ float sgr_keep_branch(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// min(0.99, x), the alpha cap, for an x that a multiplication produced.  fminf() has to quiet a signalling NaN first, and
// where hipcc cannot see the producer of x (another basic block: the second visit of a pair) it issues v_max_f32 x, x
// for that in front of the v_min_f32.  A product is never a signalling NaN, so the bare v_min_f32 returns fminf's bits:
// the smaller operand, and 0.99 for a (quiet) NaN.
__device__ __forceinline__ float sgr_alpha_cap(float x) {
    float r;
    asm("v_min_f32 %0, 0x3f7d70a4, %1" : "=v"(r) : "v"(x));  // 0.99f
    return r;
}

// __syncthreads() preceded by an explicit LDS drain.  hipcc (ROCm 7.2, gfx950) emits the post-walk barrier of the blend
// backward as a bare s_barrier at a branch target: the last trip's ds_add_f32 / ds_write_b32 of a wave may still be in
// flight when the other waves are released and flush the rows (seen on MI355X as a rare wrong row with 64-entry
// rounds; every other barrier of the library has hipcc's own s_waitcnt lgkmcnt(0) in front of it).
__device__ __forceinline__ void sgr_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// A thread's place in the launch: its workgroup's tile (sgr_wg_tile: supertile or longest-first order) and its pixel --
// wave q owns quadrant q, lane l the pixel (l & 7, l >> 3) of it.
// (Not carried as fields: the tile's list range, which the kernels load themselves -- `ranges[tp.tile]` -- and inside /
// tx0 / ty0, which are functions called where the kernels had the expressions.  As fields filled here they moved the
// register allocation of the wide forward and backward instantiations into new spills.)
struct SgrTilePixel {
    int tid, lane, wave;
    uint32_t tx, ty, tile, px, py;
    float pxf, pyf;  // pixel centre
    __device__ __forceinline__ bool inside(int W, int H) const { return px < (uint32_t)W && py < (uint32_t)H; }
    // the tile's first pixel: what the staging lanes' quadrant cull is measured from
    __device__ __forceinline__ float tx0() const { return (float)(tx * SGR_BLOCK_X); }
    __device__ __forceinline__ float ty0() const { return (float)(ty * SGR_BLOCK_Y); }
};
// false: padding block, the whole workgroup leaves
__device__ __forceinline__ bool sgr_tile_pixel(SgrTilePixel& p, int gx, int gy, const uint2* __restrict__ ranges) {
    p.tid = threadIdx.x;
    p.lane = p.tid & 63;
    p.wave = p.tid >> 6;
    if (!sgr_wg_tile(blockIdx.x, gx, gy, ranges, p.tx, p.ty)) return false;
    p.tile = p.ty * (uint32_t)gx + p.tx;
    p.px = p.tx * SGR_BLOCK_X + (p.wave & 1) * 8 + (p.lane & 7);
    p.py = p.ty * SGR_BLOCK_Y + (p.wave >> 1) * 8 + (p.lane >> 3);
    p.pxf = (float)p.px;
    p.pyf = (float)p.py;
    return true;
}

// The staging lanes' cull results (bit q of mask4 = quadrant q has to visit my entry) as one survivor mask per quadrant:
// sBits[q][row], row = the 64-entry chunk this wave staged.
template <int NCH>
__device__ __forceinline__ void sgr_store_cull_ballots(const uint32_t mask4, const int lane, const int row, uint64_t (&sBits)[4][NCH]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint64_t m = __ballot((mask4 >> q) & 1u);
        if (lane == 0) sBits[q][row] = m;
    }
}

// G = exp(power) of the forward family: one v_exp_f32 on the pre-scaled power, or the reference's expf
template <bool EXACT>
__device__ __forceinline__ float sgr_exp_fwd(const float power) {
    return EXACT ? (SGR_EXACT_TRIM ? sgr_expf_ref(power) : expf(power)) : __builtin_amdgcn_exp2f(power);
}
// G of the backward family.  Parity mode: power is in natural-log units, and v_exp_f32 is guarded at the 1/255 threshold
// (see SGR_EXACT_BWD_FAST)
template <bool EXACT>
__device__ __forceinline__ float sgr_G_bwd(const float power, const float opacity) {
    if constexpr (!EXACT) {
        return __builtin_amdgcn_exp2f(power);
    } else if constexpr (SGR_EXACT_BWD_FAST != 0) {
        float g = __builtin_amdgcn_exp2f(power * SGR_LOG2E);
        const bool near = fabsf(opacity * g - SGR_ALPHA_MIN) <= 4.0e-6f * SGR_ALPHA_MIN;
        if (SGR_EXACT_BWD_GUARD && __builtin_amdgcn_ballot_w64(near) != 0) g = SGR_EXACT_TRIM ? sgr_expf_ref(power) : expf(power);
        return g;
    } else {
        return SGR_EXACT_TRIM ? sgr_expf_ref(power) : expf(power);
    }
}

// alpha = min(0.99, opacity * G).  BARE: through sgr_alpha_cap (same bits) -- for the second visit of a pair in the parity
// mode's backward family, whose guard (sgr_G_bwd) splits the pair's blocks: hipcc keeps the product in the first block and
// sinks the fminf to the second visit, where it paid the canonicalisation.  Everywhere else the product and its fminf share a
// block, hipcc issues none, and the plain form stays (an asm statement there only costs the s_nop hipcc puts behind it).
template <bool BARE>
__device__ __forceinline__ float sgr_alpha_of(const float opacity, const float G) {
    return BARE ? sgr_alpha_cap(opacity * G) : fminf(0.99f, opacity * G);
}

// One (quadrant, entry) visit as the walk hands it to a kernel's step: LDS slot j = chunk * 64 + bit of the batch, the
// staged record q, the pixel's offsets, power, G and alpha = min(0.99, opacity * G).  Wave-uniform: j, bit, q.
struct SgrVisit {
    int j, bit;
    uint32_t ja;  // byte offset of slot j in the staged float4 arrays (sgr_slot_addr): sgr_slot(sC, v.ja) = sC[v.j]
    float4 q;
    float dx, dy, power, G, alpha;
};

// The byte offset of slot j in a staged float4 array, and the slot at such an offset.  j is wave-uniform, so the address
// register of the LDS reads is a v_mov from a scalar; hipcc lets the 128-bit read of the record land on it and
// rematerialises it for the step's own read (sC).  KEEP: the move is an asm statement, which cannot be rematerialised --
// one register held from the walk's reads to the step's, one v_mov less per visit that blends.  Where that register has
// to be spilled instead (tools/occupancy_audit.py), leave KEEP off.
template <bool KEEP>
__device__ __forceinline__ uint32_t sgr_slot_addr(const int j) {
    uint32_t a = (uint32_t)j * 16u;
    if constexpr (KEEP) asm("v_mov_b32 %0, %1" : "=v"(a) : "s"(a));
    return a;
}
__device__ __forceinline__ float4 sgr_slot(const float4* s, const uint32_t ja) {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s) + ja);
}
// Walks the set bits of m -- the survivors of chunk `chunk`, lowest (= first in walk order) first -- and calls step(visit)
// for each.  Scalar bookkeeping kept short (SALU issues once per four cycles per SIMD): s_ff1 + s_bitset0 per survivor, and
// the odd survivor is taken first so that the loop is pairs only.  A step may clear m to end the walk (the wave finished).
// BWD: G from sgr_G_bwd (the backward family) instead of sgr_exp_fwd.  KEEP: see sgr_slot_addr.
template <bool EXACT, bool BWD, bool KEEP = false, class Step>
__device__ __forceinline__ void sgr_walk_pairs(uint64_t& m, const int chunk, const float4* sA, const float4* sB, const float pxf,
                                               const float pyf, Step step) {
    if (__builtin_popcountll(m) & 1) {
        const int b0 = sgr_pop_lowest(m);
        const int j0 = chunk * 64 + b0;
        const uint32_t ja0 = sgr_slot_addr<KEEP>(j0);
        const float4 a0 = sgr_slot(sA, ja0), q0 = sgr_slot(sB, ja0);
        const float dx0 = a0.x - pxf, dy0 = a0.y - pyf;
        const float pw0 = EXACT ? sgr_power_ref_staged(q0.x, q0.y, q0.z, dx0, dy0) : sgr_power2(q0.x, q0.y, q0.z, dx0, dy0);
        const float G0 = BWD ? sgr_G_bwd<EXACT>(pw0, q0.w) : sgr_exp_fwd<EXACT>(pw0);
        step(SgrVisit{j0, b0, ja0, q0, dx0, dy0, pw0, G0, sgr_alpha_of<false>(q0.w, G0)});
    }
    while (m) {
        // two survivors per trip: their LDS reads and exp() are independent of each other, only the steps are ordered
        const int b0 = sgr_pop_lowest(m);
        const int b1 = sgr_pop_lowest(m);
        const int j0 = chunk * 64 + b0, j1 = chunk * 64 + b1;
        const uint32_t ja0 = sgr_slot_addr<KEEP>(j0), ja1 = sgr_slot_addr<KEEP>(j1);
        const float4 a0 = sgr_slot(sA, ja0), q0 = sgr_slot(sB, ja0);
        const float4 a1 = sgr_slot(sA, ja1), q1 = sgr_slot(sB, ja1);
        const float dx0 = a0.x - pxf, dy0 = a0.y - pyf, dx1 = a1.x - pxf, dy1 = a1.y - pyf;
        const float pw0 = EXACT ? sgr_power_ref_staged(q0.x, q0.y, q0.z, dx0, dy0) : sgr_power2(q0.x, q0.y, q0.z, dx0, dy0);
        const float pw1 = EXACT ? sgr_power_ref_staged(q1.x, q1.y, q1.z, dx1, dy1) : sgr_power2(q1.x, q1.y, q1.z, dx1, dy1);
        const float G0 = BWD ? sgr_G_bwd<EXACT>(pw0, q0.w) : sgr_exp_fwd<EXACT>(pw0);
        const float G1 = BWD ? sgr_G_bwd<EXACT>(pw1, q1.w) : sgr_exp_fwd<EXACT>(pw1);
        const float al0 = sgr_alpha_of<false>(q0.w, G0), al1 = sgr_alpha_of<EXACT && BWD>(q1.w, G1);
        step(SgrVisit{j0, b0, ja0, q0, dx0, dy0, pw0, G0, al0});
        step(SgrVisit{j1, b1, ja1, q1, dx1, dy1, pw1, G1, al1});  // forward: if the wave finished on j0 every threshold is +inf, a no-op
    }
}

// "this lane blends ? a : b" of a forward blend step.  MASK: on the SGPR-pair lane mask the step's ballots leave behind
// (sgr_sel_mask); else plain ?: (the compiler's v_cndmask on VCC -- the forward's SGR_FWD_SEL=0 A/B)
template <bool MASK>
struct SgrBlendSel {
    uint64_t bm;
    bool blend;
    __device__ __forceinline__ float operator()(const float a, const float b) const {
        if constexpr (MASK) return sgr_sel_mask(bm, a, b);
        else return blend ? a : b;
    }
    __device__ __forceinline__ uint32_t operator()(const uint32_t a, const uint32_t b) const {
        return __float_as_uint((*this)(__uint_as_float(a), __uint_as_float(b)));
    }
};

// One forward blend step (forward.cu:425-445) on a pixel's transmittance T.  Finished pixels (outside the image, or T
// exhausted) are tracked twice: `done_mask` is the wave's scalar lane mask (wave- and tile-wide exits are scalar compares), and
// `thr`, the per-lane alpha threshold, becomes +inf so that a finished lane fails the alpha test without a separate predicate
// (hipcc turns ballot(compound bool) and __any / __all into v_cndmask + v_cmp pairs; direct compares combined with scalar
// ANDs cost no VALU).  The step comes in two halves with the kernel's own sums in between, because those read the T from
// before the step:
//     SgrBlendStep<MASK> b;
//     if (!sgr_blend_begin(b, T, thr, v.power, v.alpha)) return;   // no lane passes the alpha test
//     Wt += b.w; ...                                               // the kernel's accumulators, on b.w and b.sel
//     sgr_blend_end(b, T, thr, done_mask, m);                      // T, finished pixels; clears m when the wave is finished
// (Some lane passing is a superset of some lane blending: if every passing lane finishes on this very entry nothing is
// blended.)
// AE: the kernel also sums on ae = "blends ? alpha : 0" (the parity mode's unfused depth and channel sums).  The step then
// selects ae and forms w = ae * T -- one select for both, the bits of the selected product (sgr_blend_weight, sgr_math.h).
// A kernel that sums on w alone keeps the selected product: the same instruction count, and the code it had.
template <bool MASK, bool AE = false>
struct SgrBlendStep {
    SgrBlendSel<MASK> sel;  // this lane blends ? a : b
    float ae;               // AE: blends ? alpha : 0
    float w;                // blends ? alpha * T : 0
    float test_T;
    uint64_t sm;            // the lanes that finish on this entry
    bool fin;               // ... this lane among them
};
template <bool MASK, bool AE>
__device__ __forceinline__ bool sgr_blend_begin(SgrBlendStep<MASK, AE>& b, const float T, const float thr, const float power, const float alpha) {
    // skip if power > 0 or alpha < 1/255 (or the pixel is finished: thr = inf)
    const bool k1 = !(power > 0.0f), k2 = !(alpha < thr);
    const uint64_t hm = __builtin_amdgcn_ballot_w64(k1) & __builtin_amdgcn_ballot_w64(k2);
    if (hm == 0) return false;
    b.test_T = T * (1.0f - alpha);
    const bool k3 = b.test_T < 0.0001f;  // forward.cu:431-436
    const uint64_t k3m = __builtin_amdgcn_ballot_w64(k3);
    b.sel = SgrBlendSel<MASK>{hm & ~k3m, k1 && k2 && !k3};
    if constexpr (AE) {
        b.ae = b.sel(alpha, 0.0f);
        b.w = sgr_blend_weight(b.ae, T);
    } else {
        b.w = b.sel(alpha * T, 0.0f);
    }
    b.sm = hm & k3m;
    b.fin = k1 && k2 && k3;
    return true;
}
template <bool MASK, bool AE>
__device__ __forceinline__ void sgr_blend_end(const SgrBlendStep<MASK, AE>& b, float& T, float& thr, uint64_t& done_mask, uint64_t& m) {
    T = b.sel(b.test_T, T);
    if (b.sm != 0) {
        thr = b.fin ? __builtin_inff() : thr;
        done_mask |= b.sm;
        if (done_mask == ~0ull) m = 0;
    }
}

// ---- the backward family: back to front, slot t of a round holds list position hi - t (per-pair arithmetic: sgr_math.h)
// The second half of staging a record (a, d4: its words 0 and 3) into a backward slot, after slotB = sgr_stage_conic_mode(b):
// slotA = {x, y, bits of the instance's partial-row index, 0} -- first row of the Gaussian (compact array, L2-resident) +
// rank of this tile among the tiles it is emitted for, in the spare word (written and read back by the staging thread only).
// false: the row lies past the row array -- a lazy forward (sgr_set_lazy) whose frame had more instances than the list
// capacity numbers its rows over ALL instances: the caller clears the slot's quadrant mask (the frame is reported invalid
// one call later; nothing may be written outside the buffers meanwhile).
__device__ __forceinline__ bool sgr_stage_bwd_row(const float4 a, const float4 d4, const uint32_t g, const uint32_t tx, const uint32_t ty,
                                                  const uint32_t* __restrict__ u0, const uint64_t* __restrict__ tmask, const uint32_t row_limit,
                                                  float4& slotA) {
    const uint32_t urow = sgr_row_of(__float_as_uint(d4.y), tx, ty, u0, tmask, g);
    slotA = make_float4(a.x, a.y, __uint_as_float(urow), 0.0f);
    return urow < row_limit;
}

// Which pixels of the wave take part in the visit of list position posj (backward.cu:527-545; pixels outside the image have
// lastc = 0): hm = their lane mask, hit = this lane among them.  The mask is taken from the three compare masks with scalar
// ANDs: ballot(compound bool) costs hipcc a v_cndmask + v_cmp per survivor.
struct SgrBwdHit { uint64_t hm; bool hit; };
__device__ __forceinline__ SgrBwdHit sgr_bwd_hit(const int posj, const int lastc, const float power, const float alpha) {
    const bool k0 = posj < lastc, k1 = !(power > 0.0f), k2 = !(alpha < SGR_ALPHA_MIN);
    const uint64_t hm = __builtin_amdgcn_ballot_w64(k0) & __builtin_amdgcn_ballot_w64(k1) & __builtin_amdgcn_ballot_w64(k2);
    return {hm, k0 && k1 && k2};
}
#endif
