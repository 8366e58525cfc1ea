// sgr_densify_scene.hip -- density control of a whole flat scene in one pass (include/sgr_densify_scene.h).
//
// The per-model plan (sgr_densify.hip) ranks four masks with exclusive scans.  Here the masks of ALL models' rows are
// scanned once; a segment's totals are the differences of the scan at its two ends and a row's rank inside its segment is
// its scan value minus the scan value at the segment's first row -- no segmented scan.  Rows (and later candidates, and
// the workgroups of the ragged gather) find their segment by a binary search over the segments' starts, staged in LDS.
// The decisions themselves are the device functions of sgr_densify_rules.h, which the per-model kernels call too.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sgr_densify_scene.h"
#include "sgr_densify_rules.h"

typedef sgr_densify_scene_segment DnSeg;
#define DN_MAXSEG SGR_DENSIFY_SCENE_MAX_SEGMENTS

// what the plan derives per segment (device memory, written by dn_scene_totals_kernel)
struct DnSegLay {
    uint32_t off0[4];  // the four scans at the segment's first row
    uint32_t tot[4];   // nA nB nS nC of the segment
    uint32_t cand_base, normals_base, box_base, pad;
};
struct DnSceneWork {
    DnWork w;
    DnSegLay* lay;         // [nseg]
    int32_t* cand_start;   // [nseg + 1] candidate row starts (the last = n_cand)
    uint32_t* seg_totals;  // [nseg, 4] read-back 1
    uint32_t* counts;      // [nseg, 5] read-back 2: low, big, outside, pruned, survivors
    int32_t* res_start;    // [nseg + 1] result row starts
    int32_t* blk_start;    // [nseg + 1] first workgroup of each segment in the ragged gather
    int64_t* out_off;      // [2, nseg] element offset of the segment's block in the result's features_dc / semantic
};
static DnSceneWork dn_scene_carve(char* base, size_t n, size_t nseg, char** end = nullptr) {
    DnSceneWork s;
    char* p = nullptr;
    s.w = dn_carve(base, n, &p);
    sgr_carve(p, s.lay, nseg);
    sgr_carve(p, s.cand_start, nseg + 1);
    sgr_carve(p, s.seg_totals, 4 * nseg);
    sgr_carve(p, s.counts, 5 * nseg);
    sgr_carve(p, s.res_start, nseg + 1);
    sgr_carve(p, s.blk_start, nseg + 1);
    sgr_carve(p, s.out_off, 2 * nseg);
    if (end) *end = p;
    return s;
}

// the last segment whose start is <= key (empty segments share their start with the next one, which wins); starts[0] <= key
__device__ __forceinline__ int dn_find_segment(const int32_t* starts, int nseg, int32_t key) {
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
dn_scene_flags_kernel(int N, int nseg, const DnSeg* __restrict__ segs, const float* __restrict__ accum,
                      const float* __restrict__ denom, const float* __restrict__ scaling, const float* __restrict__ opacity,
                      DnWork w) {
    __shared__ int32_t sStart[DN_MAXSEG];
    for (int k = threadIdx.x; k < nseg; k += 256) sStart[k] = segs[k].start;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    sgr_densify_params p = segs[dn_find_segment(sStart, nseg, i)].params;
    p.defer_prune = 1;
    dn_store_masks(w, (size_t)i, dn_decide_flags(p, accum, denom, scaling, opacity, (size_t)i));
}

// One workgroup: per segment the scans at its two ends (the scan "at N" is the grand total), then the prefix sums of the
// layout rule -- the device's statement of sgr_densify_scene_layout.  Clears the prune counters of read-back 2.
__global__ void __launch_bounds__(256)
dn_scene_totals_kernel(int N, int nseg, const DnSeg* __restrict__ segs, DnSceneWork sw) {
    const uint32_t* off[4] = {sw.w.offA, sw.w.offB, sw.w.offS, sw.w.offC};
    for (int s = threadIdx.x; s < nseg; s += 256) {
        const int a = segs[s].start, b = a + segs[s].count;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t va = a < N ? off[k][a] : sw.w.totals[k], vb = b < N ? off[k][b] : sw.w.totals[k];
            sw.lay[s].off0[k] = va;
            sw.lay[s].tot[k] = sw.seg_totals[4 * s + k] = vb - va;
        }
        for (int k = 0; k < 5; k++) sw.counts[5 * s + k] = 0u;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t cand = 0, nrm = 0, box = 0;
    for (int s = 0; s < nseg; s++) {
        DnSegLay& L = sw.lay[s];
        const uint32_t n_split = (uint32_t)segs[s].params.n_split;
        const uint32_t n_cand = L.tot[0] + L.tot[1] + n_split * L.tot[3];
        L.cand_base = cand; L.normals_base = nrm; L.box_base = box; L.pad = 0u;
        sw.cand_start[s] = (int32_t)cand;
        cand += n_cand;
        nrm += n_split * L.tot[2];
        if (segs[s].variant == SGR_PRUNE_ACTOR && segs[s].params.prune_big) box += n_cand;
    }
    sw.cand_start[nseg] = (int32_t)cand;
}

__global__ void __launch_bounds__(256)
dn_scene_map_kernel(int N, int nseg, const DnSeg* __restrict__ segs, DnSceneWork sw, int32_t* __restrict__ src,
                    uint8_t* __restrict__ kind, int32_t* __restrict__ sample_row) {
    __shared__ int32_t sStart[DN_MAXSEG];
    for (int k = threadIdx.x; k < nseg; k += 256) sStart[k] = segs[k].start;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int s = dn_find_segment(sStart, nseg, i);
    const DnSegLay L = sw.lay[s];
    const DnWork& w = sw.w;
    dn_map_row(w.flags[i], i, L.cand_base, L.tot[0], L.tot[1], L.tot[2], L.tot[3], w.offA[i] - L.off0[0], w.offB[i] - L.off0[1],
               w.offS[i] - L.off0[2], w.offC[i] - L.off0[3], segs[s].params.n_split, L.normals_base, src, kind, sample_row);
}

// keep[c] = 1 for the candidates that stay.  The four counters per segment are integers (order-independent): LDS atomics
// per candidate that is pruned, then one global atomic per non-zero counter and workgroup.
__global__ void __launch_bounds__(256)
dn_scene_prune_kernel(int n, int nseg, const DnSeg* __restrict__ segs, DnSceneWork sw, const float* __restrict__ xyz,
                      const float* __restrict__ scaling, const float* __restrict__ rotation, const float* __restrict__ opacity,
                      const float* __restrict__ box_normals, uint32_t* __restrict__ keep) {
    __shared__ int32_t sStart[DN_MAXSEG];
    __shared__ uint32_t sCnt[4 * DN_MAXSEG];
    for (int k = threadIdx.x; k < nseg; k += 256) sStart[k] = sw.cand_start[k];
    for (int k = threadIdx.x; k < 4 * nseg; k += 256) sCnt[k] = 0u;
    __syncthreads();
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) {
        const int s = dn_find_segment(sStart, nseg, c);
        const DnSeg& g = segs[s];
        const int variant = g.variant;
        const DnSphere sph = {g.sphere[0], g.sphere[1], g.sphere[2], g.sphere[3]};
        const DnBox box = {{g.box[0], g.box[1], g.box[2]}, {g.box[3], g.box[4], g.box[5]}};
        const float* zn = nullptr;
        if (variant == SGR_PRUNE_ACTOR && g.params.prune_big)
            zn = box_normals + 6 * ((size_t)sw.lay[s].box_base + (size_t)(c - sStart[s]));
        const uint32_t d = dn_decide_prune(g.params, variant, xyz, scaling, rotation, opacity, sph, box, zn, (size_t)c);
        keep[c] = d ? 0u : 1u;
        if (d) {
            if (d & DN_LOW) atomicAdd(&sCnt[4 * s + 0], 1u);
            if (d & DN_BIG) atomicAdd(&sCnt[4 * s + 1], 1u);
            if (d & DN_OUTSIDE) atomicAdd(&sCnt[4 * s + 2], 1u);
            atomicAdd(&sCnt[4 * s + 3], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 4 * nseg; k += 256)
        if (sCnt[k]) atomicAdd(&sw.counts[5 * (k >> 2) + (k & 3)], sCnt[k]);
}

__global__ void __launch_bounds__(256)
dn_scene_compact_kernel(int n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ off,
                        const int32_t* __restrict__ src, const uint8_t* __restrict__ kind, int32_t* __restrict__ sel,
                        int32_t* __restrict__ src_out, uint8_t* __restrict__ kind_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n || !keep[c]) return;
    const uint32_t o = off[c];
    sel[o] = c; src_out[o] = src[c]; kind_out[o] = kind[c];
}

// One workgroup: the survivors per segment (differences of the keep scan at the segment's candidate range), then where
// each segment's block starts in the result: its row, its first workgroup of the ragged gather and the element offsets
// of its features_dc / semantic rows.
__global__ void __launch_bounds__(256)
dn_scene_result_kernel(int n, int nseg, const DnSeg* __restrict__ segs, DnSceneWork sw, const uint32_t* __restrict__ off,
                       const uint32_t* __restrict__ total) {
    for (int s = threadIdx.x; s < nseg; s += 256) {
        const int a = sw.cand_start[s], b = sw.cand_start[s + 1];
        sw.counts[5 * s + 4] = (b < n ? off[b] : *total) - (a < n ? off[a] : *total);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int32_t row = 0, blk = 0;
    int64_t dc = 0, sem = 0;
    for (int s = 0; s < nseg; s++) {
        const int32_t cnt = (int32_t)sw.counts[5 * s + 4];
        sw.res_start[s] = row; sw.blk_start[s] = blk; sw.out_off[s] = dc; sw.out_off[nseg + s] = sem;
        row += cnt;
        blk += (cnt + SGR_DN_ROWS - 1) / SGR_DN_ROWS;
        dc += (int64_t)cnt * segs[s].dc_width;
        sem += (int64_t)cnt * segs[s].sem_width;
    }
    sw.res_start[nseg] = row; sw.blk_start[nseg] = blk;
}

// One workgroup builds up to SGR_DN_ROWS consecutive result rows of ONE segment, like sgr_densify_gather_kernel: source rows
// and kinds staged in LDS, one lane per float (or per 16 bytes, where the segment's width and both blocks' addresses allow)
// over the rows * width outputs -- coalesced stores, row-wise contiguous loads.
__global__ void __launch_bounds__(256)
dn_scene_gather_ragged_kernel(int nseg, const DnSeg* __restrict__ segs, DnSceneWork sw, int which, const float* __restrict__ in,
                              const int32_t* __restrict__ src, const uint8_t* __restrict__ kind, int zero_new,
                              float* __restrict__ out) {
    __shared__ int32_t sStart[DN_MAXSEG];
    __shared__ int32_t sSrc[SGR_DN_ROWS];
    __shared__ uint8_t sKind[SGR_DN_ROWS];
    for (int k = threadIdx.x; k < nseg; k += 256) sStart[k] = sw.blk_start[k];
    __syncthreads();
    if ((int32_t)blockIdx.x >= sw.blk_start[nseg]) return;  // a grid sized from other counts than the device's
    const int s = dn_find_segment(sStart, nseg, (int32_t)blockIdx.x);
    const DnSeg& g = segs[s];
    const uint32_t w = (uint32_t)(which ? g.sem_width : g.dc_width);
    if (w == 0u) return;
    const int first = sw.res_start[s], r0 = first + ((int)blockIdx.x - sStart[s]) * SGR_DN_ROWS;
    const int rows = min(SGR_DN_ROWS, sw.res_start[s + 1] - r0);
    if ((int)threadIdx.x < rows) {
        sSrc[threadIdx.x] = src[r0 + threadIdx.x] - g.start;  // row inside the segment's block
        sKind[threadIdx.x] = kind[r0 + threadIdx.x];
    }
    __syncthreads();
    const float* ib = in + (which ? g.sem_offset : g.dc_offset);
    float* o = out + sw.out_off[which * nseg + s] + (size_t)(r0 - first) * w;
    if ((w & 3u) == 0u && (((uintptr_t)ib | (uintptr_t)o) & 15u) == 0) {
        const uint32_t w4 = w >> 2;
        const float4* in4 = reinterpret_cast<const float4*>(ib);
        float4* o4 = reinterpret_cast<float4*>(o);
        for (uint32_t e = threadIdx.x; e < (uint32_t)rows * w4; e += 256) {
            const uint32_t r = e / w4, j = e - r * w4;
            o4[e] = (zero_new && sKind[r] != SGR_KIND_KEEP) ? make_float4(0.f, 0.f, 0.f, 0.f) : in4[(size_t)sSrc[r] * w4 + j];
        }
        return;
    }
    for (uint32_t e = threadIdx.x; e < (uint32_t)rows * w; e += 256) {
        const uint32_t r = e / w, j = e - r * w;
        o[e] = (zero_new && sKind[r] != SGR_KIND_KEEP) ? 0.0f : ib[(size_t)sSrc[r] * w + j];
    }
}

// The argument checks every entry point makes before its first HIP call.  0, or the (negative) error.
static int dn_scene_check(int64_t N, int nseg, const DnSeg* h) {
    if (nseg < 1 || nseg > DN_MAXSEG) return sgr_set_error(SGR_E_INVALID, "nseg must be in [1, " + std::to_string(DN_MAXSEG) + "]");
    if (!h) return sgr_set_error(SGR_E_INVALID, "the host copy of the segment table is required");
    for (int s = 1; s < nseg; s++)
        if (h[s].start < h[s - 1].start) return sgr_set_error(SGR_E_INVALID, "segments must be sorted by their first row");
    int64_t row = 0;
    for (int s = 0; s < nseg; s++) {
        const DnSeg& g = h[s];
        const std::string at = "segment " + std::to_string(s) + ": ";
        if (g.count < 0) return sgr_set_error(SGR_E_INVALID, at + "negative count");
        if (g.start < row) return sgr_set_error(SGR_E_INVALID, at + "segments must not overlap");
        if (g.start > row) return sgr_set_error(SGR_E_INVALID, at + "segments must cover [0, N) without gaps");
        row += g.count;
        if (g.dc_width < 0 || g.sem_width < 0 || g.dc_offset < 0 || g.sem_offset < 0)
            return sgr_set_error(SGR_E_INVALID, at + "negative width or offset");
        if (g.params.n_split < 1 || g.params.n_split != h[0].params.n_split)
            return sgr_set_error(SGR_E_INVALID, at + "n_split >= 1, one value for all segments");
        if (g.params.grad_column < 0 || g.params.grad_column > 1) return sgr_set_error(SGR_E_INVALID, at + "grad_column in {0,1}");
        if (g.variant < SGR_PRUNE_BASE || g.variant > SGR_PRUNE_ACTOR) return sgr_set_error(SGR_E_INVALID, at + "unknown prune variant");
        if (g.variant == SGR_PRUNE_BKGD && !(g.sphere[3] >= 0.0f && std::isfinite(g.sphere[0] + g.sphere[1] + g.sphere[2] + g.sphere[3])))
            return sgr_set_error(SGR_E_INVALID, at + "the background rule needs sphere = {cx, cy, cz, radius}");
        if (g.variant == SGR_PRUNE_ACTOR && g.params.prune_big)
            for (int a = 0; a < 3; a++)
                if (!(g.box[a] <= g.box[3 + a]) || !std::isfinite(g.box[a]) || !std::isfinite(g.box[3 + a]))
                    return sgr_set_error(SGR_E_INVALID, at + "the actor rule needs box = {min xyz, max xyz}");
    }
    if (row != N || N > 0x7fffffff) return sgr_set_error(SGR_E_INVALID, "segments must cover [0, N) without gaps");
    return 0;
}

extern "C" {

size_t sgr_densify_scene_work_bytes(int n, int nseg) {
    char* base = (char*)4096;
    char* end = nullptr;
    dn_scene_carve(base, (size_t)(n > 0 ? n : 1), (size_t)(nseg > 0 ? nseg : 1), &end);
    return (size_t)(end - base) + 512;
}

int sgr_densify_scene_plan(int N, int nseg, const DnSeg* segs_host, const DnSeg* segs, const float* xyz_gradient_accum,
                           const float* denom, const float* scaling, const float* opacity, char* work, int64_t* totals,
                           void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0) return sgr_set_error(SGR_E_INVALID, "N must not be negative");
    if (const int rc = dn_scene_check(N, nseg, segs_host)) return rc;
    if (!totals) return sgr_set_error(SGR_E_INVALID, "totals is required");
    for (int k = 0; k < 4 * nseg; k++) totals[k] = 0;
    if (N == 0) return 0;
    if (!segs || !xyz_gradient_accum || !denom || !scaling || !opacity || !work)
        return sgr_set_error(SGR_E_INVALID, "the device table, statistics, scaling, opacity and work are required");
    const DnSceneWork sw = dn_scene_carve((char*)sgr_align_up((size_t)work, 256), (size_t)N, (size_t)nseg);
    const DnWork& w = sw.w;
    dn_scene_flags_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, nseg, segs, xyz_gradient_accum, denom, scaling, opacity, w);
    sgr_launch_scan(w.offA, w.offA, (size_t)N, w.tmp, false, stream, w.totals + 0);
    sgr_launch_scan(w.offB, w.offB, (size_t)N, w.tmp, false, stream, w.totals + 1);
    sgr_launch_scan(w.offS, w.offS, (size_t)N, w.tmp, false, stream, w.totals + 2);
    sgr_launch_scan(w.offC, w.offC, (size_t)N, w.tmp, false, stream, w.totals + 3);
    dn_scene_totals_kernel<<<1, 256, 0, stream>>>(N, nseg, segs, sw);
    std::vector<uint32_t> t(4 * (size_t)nseg);
    SGR_HIP(hipMemcpyAsync(t.data(), sw.seg_totals, t.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SGR_HIP(hipStreamSynchronize(stream));
    for (size_t k = 0; k < t.size(); k++) totals[k] = t[k];
    return 0;
}

int sgr_densify_scene_layout(int nseg, const DnSeg* segs_host, const int64_t* totals, int64_t* layout) {
    if (nseg < 1 || !segs_host || !totals || !layout) return sgr_set_error(SGR_E_INVALID, "segments, totals and layout are required");
    int64_t cand = 0, nrm = 0, box = 0;
    for (int s = 0; s <= nseg; s++) {
        layout[3 * s] = cand; layout[3 * s + 1] = nrm; layout[3 * s + 2] = box;
        if (s == nseg) break;
        const int64_t n_split = segs_host[s].params.n_split;
        const int64_t n_cand = totals[4 * s] + totals[4 * s + 1] + n_split * totals[4 * s + 3];
        cand += n_cand;
        nrm += n_split * totals[4 * s + 2];
        if (segs_host[s].variant == SGR_PRUNE_ACTOR && segs_host[s].params.prune_big) box += n_cand;
    }
    if (cand > 0x7fffffff) return sgr_set_error(SGR_E_INVALID, "more than 2^31 points after densification");
    return 0;
}

int sgr_densify_scene_map(int N, int nseg, const DnSeg* segs_host, const DnSeg* segs, const char* work, int32_t* src,
                          uint8_t* kind, int32_t* sample_row, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0) return sgr_set_error(SGR_E_INVALID, "N must not be negative");
    if (const int rc = dn_scene_check(N, nseg, segs_host)) return rc;
    if (N == 0) return 0;
    if (!segs || !work || !src || !kind || !sample_row)
        return sgr_set_error(SGR_E_INVALID, "the device table, work, src, kind and sample_row are required");
    const DnSceneWork sw = dn_scene_carve((char*)sgr_align_up((size_t)work, 256), (size_t)N, (size_t)nseg);
    dn_scene_map_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, nseg, segs, sw, src, kind, sample_row);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_densify_scene_prune(int n_cand, int nseg, const DnSeg* segs_host, const DnSeg* segs, const float* xyz,
                            const float* scaling, const float* rotation, const float* opacity, const float* box_normals,
                            const int32_t* src, const uint8_t* kind, char* work, char* cand_work, int32_t* sel,
                            int32_t* src_out, uint8_t* kind_out, int64_t* counts, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t N = 0;
    for (int s = 0; segs_host && s < nseg && s < DN_MAXSEG; s++) N += segs_host[s].count;
    if (const int rc = dn_scene_check(N, nseg, segs_host)) return rc;
    if (n_cand < 0 || !counts) return sgr_set_error(SGR_E_INVALID, "n_cand >= 0 and counts are required");
    for (int k = 0; k < 5 * nseg; k++) counts[k] = 0;
    if (n_cand == 0) return 0;
    if (!segs || !xyz || !scaling || !rotation || !opacity || !src || !kind || !work || !cand_work || !sel || !src_out || !kind_out)
        return sgr_set_error(SGR_E_INVALID, "the device table, the candidates' arrays, both work areas and the outputs are required");
    for (int s = 0; s < nseg; s++)
        if (segs_host[s].variant == SGR_PRUNE_ACTOR && segs_host[s].params.prune_big && segs_host[s].count > 0 && !box_normals)
            return sgr_set_error(SGR_E_INVALID, "segment " + std::to_string(s) + ": the actor rule needs box_normals");
    const DnSceneWork sw = dn_scene_carve((char*)sgr_align_up((size_t)work, 256), (size_t)N, (size_t)nseg);
    const DnWork cw = dn_carve((char*)sgr_align_up((size_t)cand_work, 256), (size_t)n_cand);
    uint32_t *keep = cw.flags, *off = cw.offA;
    dn_scene_prune_kernel<<<std::min((n_cand + 255) / 256, 2048), 256, 0, stream>>>(n_cand, nseg, segs, sw, xyz, scaling, rotation,
                                                                                   opacity, box_normals, keep);
    sgr_launch_scan(keep, off, (size_t)n_cand, cw.tmp, false, stream, cw.totals + 0);
    dn_scene_compact_kernel<<<(n_cand + 255) / 256, 256, 0, stream>>>(n_cand, keep, off, src, kind, sel, src_out, kind_out);
    dn_scene_result_kernel<<<1, 256, 0, stream>>>(n_cand, nseg, segs, sw, off, cw.totals + 0);
    std::vector<uint32_t> t(5 * (size_t)nseg);
    SGR_HIP(hipMemcpyAsync(t.data(), sw.counts, t.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SGR_HIP(hipStreamSynchronize(stream));
    for (size_t k = 0; k < t.size(); k++) counts[k] = t[k];
    return 0;
}

int sgr_densify_scene_gather_ragged(int nseg, const DnSeg* segs_host, const DnSeg* segs, const int64_t* new_counts,
                                    const char* work, int which, const float* in, const int32_t* src, const uint8_t* kind,
                                    int zero_new, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t N = 0;
    for (int s = 0; segs_host && s < nseg && s < DN_MAXSEG; s++) N += segs_host[s].count;
    if (const int rc = dn_scene_check(N, nseg, segs_host)) return rc;
    if (which < 0 || which > 1 || !new_counts) return sgr_set_error(SGR_E_INVALID, "which in {0,1} and new_counts are required");
    int64_t blocks = 0, floats = 0;
    for (int s = 0; s < nseg; s++) {
        if (new_counts[s] < 0) return sgr_set_error(SGR_E_INVALID, "negative new_counts");
        blocks += (new_counts[s] + SGR_DN_ROWS - 1) / SGR_DN_ROWS;
        floats += new_counts[s] * (which ? segs_host[s].sem_width : segs_host[s].dc_width);
    }
    if (blocks == 0 || floats == 0) return 0;
    if (blocks > 0x7fffffff) return sgr_set_error(SGR_E_INVALID, "more than 2^31 points after densification");
    if (!segs || !work || !in || !src || !kind || !out)
        return sgr_set_error(SGR_E_INVALID, "the device table, work, in, src, kind and out are required");
    const DnSceneWork sw = dn_scene_carve((char*)sgr_align_up((size_t)work, 256), (size_t)N, (size_t)nseg);
    dn_scene_gather_ragged_kernel<<<(unsigned)blocks, 256, 0, stream>>>(nseg, segs, sw, which, in, src, kind, zero_new, out);
    SGR_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
