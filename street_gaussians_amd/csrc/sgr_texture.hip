// sgr_texture.hip -- bilinear cube-map lookup and its deterministic backward (include/sgr_texture.h) on gfx950.
//
// Forward: one lane per sample.  The face / (u, v) arithmetic is the contract of include/sgr_texture.h; a footprint that
// stays inside its face reads four texels directly, one that leaves it goes through the seam table (derived once on the
// host from the face orientation) and the corner rule.
//
// Backward, without float atomics and writing every gradient element once:
//   1. key     every sample gets the id of the 2x2 texel cell of its footprint on an EXTENDED grid of (R + 1)^2 cells
//              per face (cell (x0, y0), x0, y0 in [-1, R-1]): footprints that leave the face are cells of the border
//              ring, so they need no list of their own.  Samples with no footprint get the sentinel key ncells.
//   2. sort    stable LSD radix sort of (key, sample index) -- sgr_launch_sort_pairs32, iota values.
//   3. starts  starts[c] = first sorted position with key >= c, for c in [0, ncells] (a binary search per cell: every
//              entry written once; empty cells, e.g. the faces a camera does not see, cost no serial fill).
//   4. records sorted position i -> (fx, fy) of its sample and its dL/dout, contiguous in cell order.
//   5. gather  one lane per texel (per texel and channel for C != 3) walks the runs of the cells that have it as a tap:
//              its four own cells and, on a face edge, the two border cells of each neighbouring face whose outside tap
//              lands on it; a fixed order, so the sums are bit-reproducible.
// With a device-side sample count (sgr_texture_cube_backward_impl, the fused sky composite's compacted sky pixels), the
// key, sort, starts and record stages stop at that count; their grids stay sized by the host's upper bound.
//
// The sky cube map's optimiser (include/sgr_sky_step.h) splits the backward in two: the deferred backward runs stages
// 1-4 and marks the blocks of 256 texels its samples touch (sgr_texture_cube_deferred_impl); the step is stage 5's
// kernel in a second flavour that applies Adam to the texel's sum instead of storing it, over the blocks ever marked
// (sgr_texture_cube_adam_step_impl).  The flavour lives in this file so that the sum is compiled with the gather's
// floating-point settings; the Adam arithmetic carries its own (sgr_adam_math.h).
#include <string>

#include "../../include/sgr_texture.h"
#include "sgr_adam_math.h"
#include "sgr_common.h"
#include "sgr_cube.h"

// ---- forward --------------------------------------------------------------------------------------------------------
template <int CT>
__global__ void __launch_bounds__(256)
sgr_texture_cube_fwd_kernel(int Bt, int R, int Crt, int64_t n, int64_t total, const float* __restrict__ tex,
                            const float* __restrict__ uv, float* __restrict__ out, SgrCubeSeam sm) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= total) return;
    const int64_t b = s / n;
    const float* T = tex + (Bt == 1 ? 0 : b) * 6 * (int64_t)R * R * (CT > 0 ? CT : Crt);
    tx_lookup<CT>(T, R, Crt, sm, uv[3 * s], uv[3 * s + 1], uv[3 * s + 2], out + s * (CT > 0 ? CT : Crt));
}

// ---- backward -------------------------------------------------------------------------------------------------------
struct TxGrid {
    int Bt, R;
    int64_t n, total;     // samples per batch, B * n
    uint32_t ncells;      // Bt * 6 * (R + 1)^2; the sentinel key of samples with no footprint
};

__device__ __forceinline__ uint32_t tx_cell_key(const TxGrid& g, int bt, int f, int x0, int y0) {
    const uint32_t E = (uint32_t)g.R + 1u;
    return (((uint32_t)bt * 6u + (uint32_t)f) * E + (uint32_t)(y0 + 1)) * E + (uint32_t)(x0 + 1);
}

__global__ void __launch_bounds__(256)
sgr_texture_cube_key_kernel(TxGrid g, const float* __restrict__ uv, uint32_t* __restrict__ keys,
                            const uint32_t* __restrict__ dev_n) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= g.total || (dev_n && s >= (int64_t)*dev_n)) return;
    int face;
    float x, y;
    uint32_t key = g.ncells;
    if (tx_coords(uv[3 * s], uv[3 * s + 1], uv[3 * s + 2], g.R, face, x, y))
        key = tx_cell_key(g, g.Bt == 1 ? 0 : (int)(s / g.n), face, (int)floorf(x), (int)floorf(y));
    keys[s] = key;
}

__global__ void __launch_bounds__(256)
sgr_texture_cube_starts_kernel(uint32_t ncells, uint32_t nsorted, const uint32_t* __restrict__ keys,
                               uint32_t* __restrict__ starts, const uint32_t* __restrict__ dev_n) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > ncells) return;
    if (dev_n) nsorted = min(nsorted, *dev_n);
    uint32_t lo = 0, hi = nsorted;  // first position with key >= c
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
    }
    starts[c] = lo;
}

__global__ void __launch_bounds__(256)
sgr_texture_cube_record_kernel(TxGrid g, int C, const float* __restrict__ uv, const float* __restrict__ dout,
                               const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                               float2* __restrict__ rec, float* __restrict__ gs, const uint32_t* __restrict__ dev_n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.total || (dev_n && i >= (int64_t)*dev_n) || keys[i] >= g.ncells) return;  // the sentinel run at the end is never read
    const int64_t s = order[i];
    int face;
    float x, y;
    tx_coords(uv[3 * s], uv[3 * s + 1], uv[3 * s + 2], g.R, face, x, y);
    rec[i] = make_float2(x - floorf(x), y - floorf(y));
    for (int ch = 0; ch < C; ch++) gs[i * C + ch] = dout[s * C + ch];
}

// Adds the contributions of the samples of cell (x0, y0) of face f to texel `t` (index within its batch's 6 R R).
// CT > 0: all CT channels; CT = 0: channel ch of C.
template <int CT>
__device__ __forceinline__ void tx_walk_cell(const TxGrid& g, const SgrCubeSeam& sm, const uint32_t* __restrict__ starts,
                                             const float2* __restrict__ rec, const float* __restrict__ gs, int C, int ch,
                                             int bt, int f, int x0, int y0, int64_t t, double* acc) {
    const uint32_t key = tx_cell_key(g, bt, f, x0, y0);
    const uint32_t i0 = starts[key], i1 = starts[key + 1];
    if (i0 == i1) return;
    // weight of t in this cell = sum_k coef[k] w_k(fx, fy): coef[k] = 1 where tap k is t; a missing corner tap's weight
    // is shared by the other three, so it carries 1/3 for each of them that is t
    int64_t idx[4];
    const int miss = tx_cell_taps(sm, g.R, f, x0, y0, idx);
    float coef[4];
    float hits = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        coef[k] = (idx[k] == t) ? 1.f : 0.f;
        hits += coef[k];
    }
    if (miss >= 0) coef[miss] = hits * (1.f / 3.f);
    for (uint32_t i = i0; i < i1; i++) {
        const float2 r = rec[i];
        float w[4];
        tx_weights(r.x, r.y, w);
        const float wt = coef[0] * w[0] + coef[1] * w[1] + coef[2] * w[2] + coef[3] * w[3];
        if constexpr (CT > 0) {
#pragma unroll
            for (int c = 0; c < CT; c++) acc[c] += (double)(wt * gs[(size_t)i * CT + c]);
        } else {
            acc[0] += (double)(wt * gs[(size_t)i * C + ch]);
        }
    }
}

// The deferred backward (include/sgr_sky_step.h) leaves its key, sort, starts and record stages in a workspace that the
// optimiser step reads later knowing only R: the first 256 bytes say where starts, rec and gs lie (byte offsets from
// the workspace's aligned base), written on the device by the mark kernel.
struct TxDeferredHeader {
    uint64_t starts_off, rec_off, gs_off;
};

// The step flavour's arguments: the parameter and its moments [6 R R 3], the activity bytes (one per 256 texels), the
// deferred workspace (nullptr: no samples) and Adam's scalars (sgr_adam_math.h).
struct TxStep {
    float *p, *m, *v;
    const uint8_t* active;
    const char* work;
    AdamConsts k;
    float ss, bc2s, eps;
};

// STEP = false: the gather, dL/dtex written once per element.  STEP = true (CT = 3, Bt = 1): the same sum in the same
// order for the texels of the active blocks only, rounded to f32 once and consumed by adam1 in place of a stored
// gradient; starts / rec / gs come from the deferred workspace's header, dtex is not used.
template <int CT, bool STEP = false>
__global__ void __launch_bounds__(256)
sgr_texture_cube_gather_kernel(TxGrid g, SgrCubeSeam sm, int Crt, const uint32_t* __restrict__ starts,
                               const float2* __restrict__ rec, const float* __restrict__ gs, float* __restrict__ dtex,
                               TxStep st) {
    if constexpr (STEP) {
        if (!st.active[blockIdx.x]) return;  // one byte per workgroup, the same address in every lane
        if (st.work) {
            const TxDeferredHeader h = *reinterpret_cast<const TxDeferredHeader*>(st.work);
            starts = reinterpret_cast<const uint32_t*>(st.work + h.starts_off);
            rec = reinterpret_cast<const float2*>(st.work + h.rec_off);
            gs = reinterpret_cast<const float*>(st.work + h.gs_off);
        }
    }
    const int C = CT > 0 ? CT : Crt;
    const int R = g.R;
    const int64_t per = 6 * (int64_t)R * R;
    const int64_t lane = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t tg = CT > 0 ? lane : lane / C;  // texel over all Bt batches
    const int ch = CT > 0 ? 0 : (int)(lane - tg * C);
    if (tg >= g.Bt * per) return;
    const int bt = (int)(tg / per);
    const int64_t t = tg - bt * per;
    const int f = (int)(t / ((int64_t)R * R));
    const int y = (int)((t / R) % R), x = (int)(t % R);
    double acc[CT > 0 ? CT : 1];  // double sums: a texel of a small map collects thousands of samples
#pragma unroll
    for (int c = 0; c < (CT > 0 ? CT : 1); c++) acc[c] = 0.0;
    if (!STEP || st.work) {  // a step without a workspace: no samples, every gradient is +0
        // own cells: the texel is tap (x - x0, y - y0) of cells x0 in {x-1, x}, y0 in {y-1, y}
#pragma unroll
        for (int k = 0; k < 4; k++)
            tx_walk_cell<CT>(g, sm, starts, rec, gs, C, ch, bt, f, x - 1 + (k & 1), y - 1 + (k >> 1), t, acc);
        // a texel on edge e of its face is the outside tap of the two border cells of the neighbouring face next to it
        for (int e = 0; e < 4; e++) {
            const bool on = e == 0 ? x == 0 : e == 1 ? x == R - 1 : e == 2 ? y == 0 : y == R - 1;
            if (!on) continue;
            const int k = e < 2 ? y : x;
            const int gf = sm.g[f][e], be = sm.back[f][e];
            const int gc = sm.c0[f][e] * (R - 1) + sm.c1[f][e] * k, gr = sm.r0[f][e] * (R - 1) + sm.r1[f][e] * k;
            for (int j = 0; j < 2; j++) {
                int cx, cy;
                if (be < 2) { cx = be == 0 ? -1 : R - 1; cy = gr - 1 + j; }
                else { cy = be == 2 ? -1 : R - 1; cx = gc - 1 + j; }
                tx_walk_cell<CT>(g, sm, starts, rec, gs, C, ch, bt, gf, cx, cy, t, acc);
            }
        }
    }
    if constexpr (STEP) {
        static_assert(CT == 3, "the step flavour is the sky cube map's: three channels");
        // the texel's 12 bytes of p, m and v, as the gather writes dtex: consecutive lanes, consecutive texels
        float* __restrict__ p = st.p + tg * 3;
        float* __restrict__ m = st.m + tg * 3;
        float* __restrict__ v = st.v + tg * 3;
        float P[3], M[3], V[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { P[c] = p[c]; M[c] = m[c]; V[c] = v[c]; }
#pragma unroll
        for (int c = 0; c < 3; c++) adam1(P[c], (float)acc[c], M[c], V[c], st.k, st.ss, st.bc2s, st.eps);
        // array by array: three neighbouring stores merge into one 12-byte store per lane
#pragma unroll
        for (int c = 0; c < 3; c++) p[c] = P[c];
#pragma unroll
        for (int c = 0; c < 3; c++) m[c] = M[c];
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = V[c];
    } else if constexpr (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; c++) dtex[tg * CT + c] = (float)acc[c];
    } else {
        dtex[tg * C + ch] = (float)acc[0];
    }
}

// Deferred backward: the activity bytes of this backward's samples.  One lane per sorted position below the device
// count: every texel that is a tap of the sample's cell (tx_cell_taps: seam taps on the neighbouring face included, a
// missing corner tap not) marks its block of 256 texels.  Many lanes store the same byte value: plain stores.  Lane 0
// also writes the workspace's header.
__global__ void __launch_bounds__(256)
sgr_texture_cube_mark_kernel(TxGrid g, SgrCubeSeam sm, const uint32_t* __restrict__ keys,
                             const uint32_t* __restrict__ dev_n, uint8_t* __restrict__ active,
                             TxDeferredHeader* __restrict__ hdr, TxDeferredHeader h) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *hdr = h;
    if (i >= g.total || (dev_n && i >= (int64_t)*dev_n)) return;
    const uint32_t key = keys[i];
    if (key >= g.ncells) return;  // the sentinel: no footprint
    const uint32_t E = (uint32_t)g.R + 1u;
    const int x0 = (int)(key % E) - 1, y0 = (int)((key / E) % E) - 1, f = (int)(key / (E * E));
    int64_t idx[4];
    tx_cell_taps(sm, g.R, f, x0, y0, idx);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (idx[k] >= 0) active[idx[k] / SGR_TX_STEP_BLOCK] = 1;
}
static_assert(SGR_TX_STEP_BLOCK == 256, "one workgroup of the gather is one activity block");

// ---- host -----------------------------------------------------------------------------------------------------------
namespace {

const int kSU[6] = {-1, 1, 1, 1, 1, -1}, kSV[6] = {-1, -1, 1, -1, -1, -1};

// the contract's face choice and (u, v), in double
void face_uv(const double d[3], int& f, double& u, double& v) {
    const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
    double c, s, t;
    if (az > fmax(ax, ay)) { c = d[2]; s = d[0]; t = d[1]; f = 4 + (c < 0); }
    else if (ay > ax) { c = d[1]; s = d[0]; t = d[2]; f = 2 + (c < 0); }
    else { c = d[0]; s = d[2]; t = d[1]; f = 0 + (c < 0); }
    const double m = 0.5 / fabs(c);
    u = s * kSU[f] * m + 0.5;
    v = t * kSV[f] * m + 0.5;
}

// its inverse: the direction through texel centre (col, row) of face f, which may lie one texel outside the face
void texel_dir(int f, int R, int col, int row, double d[3]) {
    const double s = (2.0 * (col + 0.5) / R - 1.0) * kSU[f], t = (2.0 * (row + 0.5) / R - 1.0) * kSV[f];
    const double c = (f & 1) ? -1.0 : 1.0;
    if (f < 2) { d[0] = c; d[1] = t; d[2] = s; }
    else if (f < 4) { d[0] = s; d[1] = c; d[2] = t; }
    else { d[0] = s; d[1] = t; d[2] = c; }
}

// Seam table: a tap one texel across edge e of face f points into the neighbouring face; the texel it lands on there
// is the one that shares the edge segment (the along-edge coordinate is kept, the across-edge one is the border texel).
// Derived at two resolutions and checked at every edge position.
bool derive_seam(SgrCubeSeam& sm) {
    for (int f = 0; f < 6; f++)
        for (int e = 0; e < 4; e++) {
            for (int pass = 0; pass < 2; pass++) {
                const int R = pass ? 7 : 8;
                int coef[2][2] = {{0, 0}, {0, 0}}, g0 = -1;
                for (int k = 0; k < R; k++) {
                    const int col = e == 0 ? -1 : e == 1 ? R : k, row = e == 2 ? -1 : e == 3 ? R : k;
                    double d[3], u, v;
                    int g;
                    texel_dir(f, R, col, row, d);
                    face_uv(d, g, u, v);
                    const int gc = (int)floor(u * R), gr = (int)floor(v * R);
                    if (gc < 0 || gc >= R || gr < 0 || gr >= R || g == f) return false;
                    if (k == 0) {
                        g0 = g;
                        coef[0][0] = gc == 0 ? 0 : gc == R - 1 ? 1 : -1;
                        coef[1][0] = gr == 0 ? 0 : gr == R - 1 ? 1 : -1;
                        if (coef[0][0] < 0 || coef[1][0] < 0) return false;
                    } else if (k == 1) {
                        coef[0][1] = gc - coef[0][0] * (R - 1);
                        coef[1][1] = gr - coef[1][0] * (R - 1);
                    }
                    if (g != g0 || gc != coef[0][0] * (R - 1) + coef[0][1] * k || gr != coef[1][0] * (R - 1) + coef[1][1] * k)
                        return false;
                }
                const int8_t ent[5] = {(int8_t)g0, (int8_t)coef[0][0], (int8_t)coef[0][1], (int8_t)coef[1][0],
                                       (int8_t)coef[1][1]};
                int8_t* dst[5] = {&sm.g[f][e], &sm.c0[f][e], &sm.c1[f][e], &sm.r0[f][e], &sm.r1[f][e]};
                for (int q = 0; q < 5; q++) {
                    if (pass && *dst[q] != ent[q]) return false;  // the same table at both resolutions
                    *dst[q] = ent[q];
                }
            }
        }
    for (int f = 0; f < 6; f++)
        for (int e = 0; e < 4; e++) {
            const int g = sm.g[f][e];
            int back = -1;
            for (int b = 0; b < 4; b++)
                if (sm.g[g][b] == f) back = back < 0 ? b : 4;  // exactly one edge of g leads back
            if (back < 0 || back > 3) return false;
            sm.back[f][e] = (int8_t)back;
        }
    return true;
}

}  // namespace

const SgrCubeSeam* sgr_cube_seam() {
    static SgrCubeSeam sm;
    static const bool ok = derive_seam(sm);
    return ok ? &sm : nullptr;
}

namespace {

int check_args(int Bt, int B, int R, int C, int64_t n, TxGrid& g) {
    if (R < 1 || C < 1 || B < 1 || n < 0 || !(Bt == 1 || Bt == B))
        return sgr_set_error(SGR_E_INVALID, "texture: need R >= 1, C >= 1, B >= 1, n >= 0 and Bt = 1 or B");
    const uint64_t E = (uint64_t)R + 1, ncells = (uint64_t)Bt * 6 * E * E;
    if (ncells >= 0xffffffffull)
        return sgr_set_error(SGR_E_INVALID, "texture: Bt * 6 * (R + 1)^2 cell keys do not fit in 32 bits");
    if ((uint64_t)B * (uint64_t)n > 0x7fffffffull)
        return sgr_set_error(SGR_E_INVALID, "texture: more than 2^31 - 1 samples");
    if (!sgr_cube_seam()) return sgr_set_error(SGR_E_INVALID, "texture: the cube seam table could not be derived");
    g.Bt = Bt;
    g.R = R;
    g.n = n;
    g.total = (int64_t)B * n;
    g.ncells = (uint32_t)ncells;
    return 0;
}

struct TxWork {
    uint32_t *keys[2], *vals[2], *hist, *scan_tmp, *starts;
    float2* rec;
    float* gs;
};

TxWork carve(char* base, const TxGrid& g, int C, char** end = nullptr) {
    TxWork w;
    char* p = base;
    const size_t n = g.total ? (size_t)g.total : 1;
    sgr_carve(p, w.keys[0], n);
    sgr_carve(p, w.keys[1], n);
    sgr_carve(p, w.vals[0], n);
    sgr_carve(p, w.vals[1], n);
    sgr_carve(p, w.hist, sgr_sort_hist_words(n));
    sgr_carve(p, w.scan_tmp, sgr_scan_tmp_count(1));
    sgr_carve(p, w.starts, (size_t)g.ncells + 1);
    sgr_carve(p, w.rec, n);
    sgr_carve(p, w.gs, n * C);
    if (end) *end = p;
    return w;
}

unsigned blocks(uint64_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace

size_t sgr_texture_cube_workspace_bytes(int Bt, int B, int R, int C, int64_t n) {
    TxGrid g;
    if (check_args(Bt, B, R, C, n, g) < 0) return 0;
    return sgr_required([&](char* base, char** end) { carve(base, g, C, end); });
}

int sgr_texture_cube_forward(int Bt, int B, int R, int C, int64_t n, const float* tex, const float* uv, float* out,
                             void* stream_) {
    TxGrid g;
    if (const int rc = check_args(Bt, B, R, C, n, g)) return rc;
    if (!tex || !uv || !out) return sgr_set_error(SGR_E_INVALID, "texture: tex, uv and out are required");
    if (g.total == 0) return 0;
    hipStream_t s = (hipStream_t)stream_;
    const SgrCubeSeam& sm = *sgr_cube_seam();
    if (C == 3) sgr_texture_cube_fwd_kernel<3><<<blocks(g.total), 256, 0, s>>>(Bt, R, C, n, g.total, tex, uv, out, sm);
    else sgr_texture_cube_fwd_kernel<0><<<blocks(g.total), 256, 0, s>>>(Bt, R, C, n, g.total, tex, uv, out, sm);
    SGR_HIP(hipGetLastError());
    return 0;
}

namespace {

// stages 1-4 of the backward: key, sort, records, starts; returns which of w.keys holds the sorted keys
int sort_stages(const TxGrid& g, int C, const float* uv, const float* dL_dout, const TxWork& w, const uint32_t* dev_n,
                hipStream_t s) {
    int cur = 0;
    if (g.total) {
        sgr_texture_cube_key_kernel<<<blocks(g.total), 256, 0, s>>>(g, uv, w.keys[0], dev_n);
        int end_bit = 1;
        while (end_bit < 32 && (g.ncells >> end_bit)) end_bit++;  // the sentinel ncells is the largest key
        cur = sgr_launch_sort_pairs32(w.keys, w.vals, (uint32_t)g.total, end_bit, w.hist, w.scan_tmp, s, true, nullptr,
                                      nullptr, 8, 0, dev_n);
        sgr_texture_cube_record_kernel<<<blocks(g.total), 256, 0, s>>>(g, C, uv, dL_dout, w.keys[cur], w.vals[cur], w.rec,
                                                                       w.gs, dev_n);
    }
    sgr_texture_cube_starts_kernel<<<blocks((uint64_t)g.ncells + 1), 256, 0, s>>>(g.ncells, (uint32_t)g.total, w.keys[cur],
                                                                                  w.starts, dev_n);
    return cur;
}

constexpr size_t kDeferredHeaderBytes = 256;

}  // namespace

int sgr_texture_cube_backward_impl(int Bt, int B, int R, int C, int64_t n, const float* uv, const float* dL_dout,
                                   float* dL_dtex, void* workspace, const uint32_t* dev_n, hipStream_t s) {
    TxGrid g;
    if (const int rc = check_args(Bt, B, R, C, n, g)) return rc;
    if (!uv || !dL_dout || !dL_dtex || !workspace)
        return sgr_set_error(SGR_E_INVALID, "texture: uv, dL_dout, dL_dtex and workspace are required");
    if (dev_n && (Bt != 1 || B != 1)) return sgr_set_error(SGR_E_INVALID, "texture: a device-side count needs Bt = B = 1");
    const SgrCubeSeam& sm = *sgr_cube_seam();
    TxWork w = carve((char*)sgr_align_up((size_t)workspace, 256), g, C);
    sort_stages(g, C, uv, dL_dout, w, dev_n, s);
    const uint64_t texels = (uint64_t)Bt * 6 * R * R;
    if (C == 3)
        sgr_texture_cube_gather_kernel<3><<<blocks(texels), 256, 0, s>>>(g, sm, C, w.starts, w.rec, w.gs, dL_dtex, TxStep{});
    else
        sgr_texture_cube_gather_kernel<0><<<blocks(texels * C), 256, 0, s>>>(g, sm, C, w.starts, w.rec, w.gs, dL_dtex,
                                                                             TxStep{});
    SGR_HIP(hipGetLastError());
    return 0;
}

size_t sgr_texture_cube_deferred_bytes(int R, int64_t n) {
    const size_t tb = sgr_texture_cube_workspace_bytes(1, 1, R, 3, n);
    return tb ? tb + kDeferredHeaderBytes : 0;
}

int sgr_texture_cube_deferred_impl(int R, int64_t n, const float* uv, const float* dL_dout, void* work,
                                   const uint32_t* dev_n, uint8_t* active, hipStream_t s) {
    TxGrid g;
    if (const int rc = check_args(1, 1, R, 3, n, g)) return rc;
    if (!uv || !dL_dout || !work || !active || !dev_n)
        return sgr_set_error(SGR_E_INVALID, "texture: uv, dL_dout, the workspace, active and the count are required");
    char* base = (char*)sgr_align_up((size_t)work, 256);
    TxWork w = carve(base + kDeferredHeaderBytes, g, 3);
    const int cur = sort_stages(g, 3, uv, dL_dout, w, dev_n, s);
    const TxDeferredHeader h{(uint64_t)((char*)w.starts - base), (uint64_t)((char*)w.rec - base),
                             (uint64_t)((char*)w.gs - base)};
    sgr_texture_cube_mark_kernel<<<blocks(g.total ? g.total : 1), 256, 0, s>>>(g, *sgr_cube_seam(), w.keys[cur], dev_n,
                                                                               active, (TxDeferredHeader*)base, h);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_texture_cube_adam_step_impl(int R, float* p, float* m, float* v, const void* work, const uint8_t* active,
                                    float step_size, float bc2_sqrt, float eps, double beta1, double beta2, hipStream_t s) {
    TxGrid g;
    if (const int rc = check_args(1, 1, R, 3, 0, g)) return rc;
    if (!p || !m || !v || !active) return sgr_set_error(SGR_E_INVALID, "texture: p, m, v and active are required");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return sgr_set_error(SGR_E_INVALID, "adam: betas must lie in [0, 1)");
    const TxStep st{p, m, v, active, work ? (const char*)sgr_align_up((size_t)work, 256) : nullptr,
                    adam_consts(beta1, beta2), step_size, bc2_sqrt, eps};
    const uint64_t texels = (uint64_t)6 * R * R;
    sgr_texture_cube_gather_kernel<3, true><<<blocks(texels), 256, 0, s>>>(g, *sgr_cube_seam(), 3, nullptr, nullptr, nullptr,
                                                                          nullptr, st);
    SGR_HIP(hipGetLastError());
    return 0;
}

int sgr_texture_cube_backward(int Bt, int B, int R, int C, int64_t n, const float* uv, const float* dL_dout,
                              float* dL_dtex, void* workspace, void* stream_) {
    return sgr_texture_cube_backward_impl(Bt, B, R, C, n, uv, dL_dout, dL_dtex, workspace, nullptr, (hipStream_t)stream_);
}
