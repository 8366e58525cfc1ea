/* sgr_texture.h -- C ABI of the cube-map lookup of the reference's sky model: nvdiffrast's texture() with
 * boundary_mode='cube' and bilinear filtering, restricted to what lib/models/sky_cubemap.py calls:
 *
 *   sky_cubemap.py:99-120   dr.texture(sky_cube_map[None], rays_d[None], filter_mode='linear', boundary_mode='cube')
 *                           on every pixel ([1,H,W,3]) or on the sky pixels only ([1,1,N,3]), once per iteration, with
 *                           the gradient flowing to the learnable 6 x R x R x 3 cube map
 *   sky_cubemap.py:178-191  cubemap_to_latlong: the same lookup at R x 2R directions on every checkpoint save
 *
 * Layouts (DEVICE arrays, float32, contiguous):
 *   tex      [Bt, 6, R, R, C]    texel (col, row) of face f of batch bt = tex[bt, f, row, col, :]
 *   uv       [B, n, 3]           direction vectors (need not be normalised); Bt is 1 (one map for all B) or B
 *   out      [B, n, C]
 * Per direction: the major axis picks the face (ties go to x over y, and to x or y over z), the other two coordinates
 * divided by the major one give (u, v) in [0, 1], clamped; bilinear over texel centres.  A footprint texel one step
 * outside its face takes the texel of the neighbouring face that shares that edge segment (the seam table is derived
 * from the face orientation at library load, not written by hand); a footprint corner outside both edges has no texel,
 * its value is the mean of the other three.  A direction whose (u, v) is not finite (zero, NaN) gives 0.
 *
 * The backward is deterministic and writes every element of dL/dtex exactly once (no float atomics): samples are keyed
 * by the 2x2 texel cell of their footprint, stably sorted, and a texel-parallel gather sums the runs of the cells that
 * touch each texel in a fixed order.  Cell keys are 32-bit: Bt * 6 * (R + 1)^2 must stay below 2^32 - 1
 * (SGR_E_INVALID otherwise, in both directions).  Nothing synchronises with the host. */
#ifndef SGR_TEXTURE_H
#define SGR_TEXTURE_H
#include <stddef.h>
#include <stdint.h>
#include "sgr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the backward's workspace (0 when the arguments are invalid) */
size_t sgr_texture_cube_workspace_bytes(int Bt, int B, int R, int C, int64_t n);

/* out[b, i, :] = bilinear cube lookup of tex[Bt == 1 ? 0 : b] at direction uv[b, i]. */
int sgr_texture_cube_forward(int Bt, int B, int R, int C, int64_t n, const float* tex, const float* uv, float* out,
                             void* stream);

/* dL/dtex[t] = sum over the samples whose footprint holds t of (bilinear weight of t) * dL/dout (all B batches when
 * Bt == 1).  Every element of dL_dtex is written, untouched texels with 0.  workspace: sgr_texture_cube_workspace_bytes. */
int sgr_texture_cube_backward(int Bt, int B, int R, int C, int64_t n, const float* uv, const float* dL_dout,
                              float* dL_dtex, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
