// sgr_radix.h -- the steps the binning chain's kernels share, one text each: the wave and the workgroup scan, eight elements
// per thread around a scan, the wave64 ballot-match rank, digit counts to first slots.  Used by sgr_scan_sort.hip,
// sgr_tile_sort.hip and the duplicate / tile-order kernels of sgr_preprocess.hip.  What needs no wave intrinsic is
// __host__ __device__ with the owner index and the arrays as parameters and the barriers left to the caller, so
// tests/host_math/host_math.hip runs it owner by owner.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SGR_RADIX_HD __host__ __device__ __forceinline__

__device__ __forceinline__ uint32_t sgr_wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan of one value per thread over a workgroup of WAVES waves (lds: WAVES words); the workgroup's total in `total`
template <int WAVES>
__device__ __forceinline__ uint32_t sgr_block_excl_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = sgr_wave_incl_scan(v, lane);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t t = lds[w];
        if (w < WAVES - 1) base += w < wave ? t : 0u;  // (the last wave's sum is in nobody's base)
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}
__device__ __forceinline__ uint32_t sgr_block_excl_scan256(uint32_t v, uint32_t* lds4, uint32_t& total) {
    return sgr_block_excl_scan<4>(v, lds4, total);
}

// Eight consecutive elements per thread around a block scan: v[i] = load(base + i), 0 at and past n; returns their sum ...
template <typename I, typename L>
SGR_RADIX_HD uint32_t sgr_load8_sum(uint32_t (&v)[8], I base, I n, L&& load) {
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = (base + i < n) ? load(base + i) : 0u;
        s += v[i];
    }
    return s;
}
// ... and the running prefix written back: out[base + i] = run + v[0] + .. + v[i - 1] (inclusive: + v[i])
template <typename I>
SGR_RADIX_HD void sgr_store8_prefix(const uint32_t (&v)[8], I base, I n, uint32_t run, bool inclusive, uint32_t* out) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (inclusive) run += v[i];
        if (base + i < n) out[base + i] = run;
        if (!inclusive) run += v[i];
    }
}

// Wave64 ballot-match rank: this lane's key among the wave's keys of digit d seen so far (earlier calls + lower lanes), and
// the wave's counter c[d] moved on by the call's count.  Every lane of the wave calls it (valid = holds a key; the bits of a
// lane without one do not matter, it is not in vm).  No atomics: deterministic.
template <int BITS>
__device__ __forceinline__ uint32_t sgr_ballot_rank(uint32_t* c, uint32_t d, bool valid) {
    // the lanes that share this lane's digit: per bit, keep the lanes whose bit equals mine -- m &= ballot XNOR (my bit
    // spread over the word).  On 32-bit halves with v_bfe_i32 / v_xor / v_and: a `bit ? bal : ~bal` select compiles to
    // v_cndmask on VCC, 23 cycles per wave instruction back to back on gfx950 (profiles/r5/valu_rates2.jsonl)
    const uint64_t vm = __builtin_amdgcn_ballot_w64(valid);
    uint32_t mlo = (uint32_t)vm, mhi = (uint32_t)(vm >> 32);
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        const int y = __builtin_amdgcn_sbfe((int)d, b, 1);  // 0 or -1
        const uint64_t bal = __builtin_amdgcn_ballot_w64(y != 0);
        mlo &= ~((uint32_t)bal ^ (uint32_t)y);
        mhi &= ~((uint32_t)(bal >> 32) ^ (uint32_t)y);
    }
    const uint32_t prefix = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));  // set bits of m below this lane
    // every lane of the group reads the wave's counter of the digit, its lowest lane moves it on by the group's size
    const uint32_t prev = valid ? c[d] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (valid && prefix == 0) c[d] = prev + (uint32_t)(__builtin_popcount(mlo) + __builtin_popcount(mhi));
    __builtin_amdgcn_wave_barrier();
    return prev + prefix;
}

// Digit counts -> first slots.  In: cnt[w][d] = the keys of digit d that wave w holds.  Out: cnt[w][d] = the first slot of
// those keys -- digits ascending, inside a digit the waves ascending.  An owner (a lane or a thread) holds the BPO consecutive
// bins from owner * BPO on; owners past bin NB - 1 idle.  sgr_bin_counts takes the owner's counts into registers and returns
// their sum; the caller scans the sums over the owners (its own wave or block scan, its own barriers); sgr_bin_starts gets the
// exclusive prefix and walks the owner's bins.  per_bin(bin, j, start): whatever else the caller keeps per bin, called with the
// bin's first slot (j = the bin's index among the owner's).
template <int WAVES, int NB, int BPO>
SGR_RADIX_HD uint32_t sgr_bin_counts(const uint32_t (*cnt)[NB], int owner, uint32_t (&c)[BPO][WAVES]) {
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < BPO; j++) {
        const int bin = owner * BPO + j;
#pragma unroll
        for (int w = 0; w < WAVES; w++) c[j][w] = 0u;
        if (bin < NB) {  // (one test around the WAVES reads, so that they can pair up)
#pragma unroll
            for (int w = 0; w < WAVES; w++) {
                c[j][w] = cnt[w][bin];
                sum += c[j][w];
            }
        }
    }
    return sum;
}
template <int WAVES, int NB, int BPO, typename F>
SGR_RADIX_HD void sgr_bin_starts(uint32_t (*cnt)[NB], int owner, const uint32_t (&c)[BPO][WAVES], uint32_t run, F&& per_bin) {
#pragma unroll
    for (int j = 0; j < BPO; j++) {
        const int bin = owner * BPO + j;
        if (bin < NB) {
            per_bin(bin, j, run);
#pragma unroll
            for (int w = 0; w < WAVES; w++) {
                cnt[w][bin] = run;
                run += c[j][w];
            }
        }
    }
}
template <int WAVES, int NB, int BPO>
SGR_RADIX_HD void sgr_bin_starts(uint32_t (*cnt)[NB], int owner, const uint32_t (&c)[BPO][WAVES], uint32_t run) {
    sgr_bin_starts<WAVES, NB, BPO>(cnt, owner, c, run, [](int, int, uint32_t) {});
}
