"""`-m gpu` parity tests at the frame sizes where the rasterizer changes how it indexes (csrc/sgr_api.hip,
csrc/sgr_preprocess.hip), above the 9 600 tiles of the largest frame elsewhere in the suite:

  * sgr_pack_camera_kernel zeroes the tile ranges with at most 64 workgroups of 256 lanes: its loop wraps above 16 384 tiles;
  * sgr_pack_rect packs a tile rect's x0, y0 and width into 10-bit fields (SGR_MAX_GRID_DIM = 1023 tiles per axis);
  * Switches::key16 takes 16-bit tile keys below 65 535 tiles (the all-ones key is padding) and 32-bit keys from there on;
  * frames of more than 16 368 pixels per side are refused.

Each case runs like test_gpu_parity.test_edge_sizes, whose helpers it uses: mode "default" (the oracle's lists restricted to
the emitted rects, images, same-state gradients), mode "strict" (EXACT | REF_RECT: point_list, keys, ranges and n_contrib
entry for entry against the C oracle, and against the reference's kernels where oracle/_ref travelled) and mode "exact" (the
parity mode against the reference's kernels).  Semantics stay on (S = 2), so the wide blend instantiation runs.  Every case
asserts FROM THE ORACLE that its scene reaches what it is named after."""
import numpy as np
import pytest
import torch

from gpu_utils import (SAME_STATE_GATE, dev, exact_mode_against_reference_kernels, grad_close, image_close, npy,
                       oracle_backward_same_state, raw_backward, raw_forward, restrict_oracle, settings)
from helpers import oracle_kwargs
from oracle import oracle
from street_gaussians_amd import synthetic as syn
from test_gpu_parity import GRAD_KEYS, _ref, _strict_legs

pytestmark = pytest.mark.gpu

S = 2
MODES = ["default", "exact", "strict"]


def _tiles(fw):
    """The tile id of every instance of the oracle's sorted list (the high word of its key)."""
    return (fw.keys >> np.uint64(32)).astype(np.int64)


def _concat(a, b):
    return syn.Scene(*[torch.cat([getattr(a, k), getattr(b, k)]).contiguous()
                       for k in ("means3D", "scales", "rotations", "opacities", "shs", "semantics")])


def _run(cam, sc, mode, label, occupancy, oracle_sum=False):
    """One scene in one mode.  `occupancy(fw)` asserts on the C oracle's forward what the scene is there for.  `oracle_sum`:
    how the C oracle's backward accumulates (oracle.backward's `parallel`)."""
    kw = oracle_kwargs(cam, sc, deg=3)
    wts = syn.loss_weights(cam, S=S)
    fw = oracle.forward(**kw)
    occupancy(fw)
    if mode == "exact":
        fw.free()
        _ref()
        exact_mode_against_reference_kernels(kw, wts, S, label)
        return
    if mode == "strict":
        fw.free()
        _strict_legs(kw, wts, S, label, oracle_sum=oracle_sum)
        return
    res, internal = raw_forward(kw)
    b = restrict_oracle(internal, fw, kw)
    assert res["R"] == b.num_rendered and b.num_rendered > 0
    assert (npy(res["radii"]) == fw.radii).all()
    assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
    assert (npy(internal("keys")).view(np.uint64) == b.keys).all()
    assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
    image_close(npy(res["color"]), fw.color, name="color")
    image_close(npy(res["depth"]), fw.depth, name="depth")
    image_close(npy(res["alpha"]), fw.alpha, name="alpha")
    image_close(npy(res["semantic"]), fw.semantic, name="semantic")
    g = raw_backward(kw, res, wts)
    same = oracle_backward_same_state(oracle, fw, res, wts, S, parallel=oracle_sum)
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"same-state {label}:{k}", **SAME_STATE_GATE)
    fw.free()
    return b


@pytest.mark.parametrize("mode", MODES)
def test_widest_frame_full_width_rect_then_sparse_ranges(mode):
    """16368 x 272: 1023 x 17 = 17 391 tiles, the widest grid there is and more tiles than one trip of the range-zeroing loop.
    Two scenes on the same frame size, in this order, so that the second is likely to get the first one's ranges buffer back
    from the allocator:
      1. two giant Gaussians over a few small ones -- a rect of width 1023, x0 + w at the limit of the 10-bit fields, and
         every tile's range written;
      2. a few hundred small Gaussians -- most tiles past 16 384 are empty, and their ranges must read (0, 0)."""
    W, H, gx = 16368, 272, 1023
    cam = syn.make_camera(W, H, fx=8000.0)
    assert (W + 15) // 16 == gx and gx * ((H + 15) // 16) > 16384
    giants = syn.make_scene(2, cam, S=S, seed=302, scale_px=0.75, zmin=2.0, zmax=4.0, margin=0.5)
    giants.opacities.fill_(0.6)  # (so that the alpha >= 1/255 box the default rects are cut to is as wide as the frame too)
    small = syn.make_scene(40, cam, S=S, seed=312, scale_px=0.0005, zmin=2.0, zmax=4.0, margin=1.0)

    def full_width(fw):
        t = _tiles(fw)
        columns = [np.unique(t[fw.point_list == i] % gx).size for i in range(2)]
        assert max(columns) == gx, columns          # some Gaussian's tiles span all 1023 columns
        assert (t % gx == gx - 1).any()             # tile column 1022 is occupied

    # Each giant gets a gradient term from every one of the frame's 4.45 M pixels.  The C oracle adds them one after the other
    # into a float32 (its default), and for dL/dmeans2D's third column -- the sum of the terms' magnitudes, all of one sign --
    # that running sum stops taking in the terms below half an ulp of it: measured on MI355X it ends at 316 178 where the
    # library and the reference's own kernels (mode "exact" below, no element outside) end at 317 146, 3e-3 apart, the oracle's
    # own error.  So the oracle sums the same float32 terms in double here ("exact"), as it does at the full benchmark sizes.
    b = _run(cam, _concat(giants, small), mode, "wide_giant", full_width, oracle_sum="exact")
    if b is not None:  # the rect the library packed for it: x0 = 0, w = 1023
        assert ((b.rect[:2, 0] == 0) & (b.rect[:2, 2] == gx)).any(), b.rect[:2]

    def sparse(fw):
        n = fw.ranges[16384:, 1].astype(np.int64) - fw.ranges[16384:, 0]
        assert (n == 0).any() and (n > 0).any()     # tiles past the zeroing loop's first trip: some empty, some occupied

    _run(cam, syn.make_scene(300, cam, S=S, seed=320, scale_px=0.0005, zmin=2.0, zmax=40.0, margin=1.1), mode, "wide_sparse",
         sparse)


@pytest.mark.parametrize("mode", MODES)
def test_last_frame_with_16_bit_tile_keys(mode):
    """6944 x 2416: 434 x 151 = 65 534 tiles, the most a frame can have and keep 16-bit tile keys.  Its highest tile id,
    65 533, is one below the key reserved as padding; the tile ids of the exported keys are the oracle's."""
    W, H = 6944, 2416
    cam = syn.make_camera(W, H, fx=7000.0)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert T == 65534

    def last_tile(fw):
        assert int(_tiles(fw).max()) == T - 1 == 65533

    _run(cam, syn.make_scene(3000, cam, S=S, seed=330, scale_px=0.002), mode, "keys16_last", last_tile)


@pytest.mark.parametrize("mode", MODES)
def test_first_frame_with_32_bit_tile_keys(mode):
    """4080 x 4112: 255 x 257 = 65 535 tiles, the first frame that takes 32-bit tile keys without the switch.  A tile whose id
    does not fit a 16-bit key next to the padding value holds an instance, so a truncated key could not go unnoticed."""
    W, H = 4080, 4112
    cam = syn.make_camera(W, H, fx=4200.0)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert T == 65535

    def beyond_16_bits(fw):
        assert int(_tiles(fw).max()) >= 65534

    _run(cam, syn.make_scene(3000, cam, S=S, seed=340, scale_px=0.002), mode, "keys32_first", beyond_16_bits)


@pytest.mark.parametrize("W,H", [(16369, 16), (16, 16369)])
def test_frames_beyond_the_packed_rect_are_refused(W, H):
    from diff_gaussian_rasterization import GaussianRasterizer
    from street_gaussians_amd._native import SgrError
    cam = syn.make_camera(W, H, fx=float(max(W, H)))
    sc = syn.make_scene(2, cam, S=S, seed=350, scale_px=0.01, zmin=2.0, zmax=4.0, margin=0.5)
    rast = GaussianRasterizer(raster_settings=settings(cam))
    with pytest.raises(SgrError, match="16368"):
        rast(dev(sc.means3D), None, dev(sc.opacities), shs=dev(sc.shs), scales=dev(sc.scales), rotations=dev(sc.rotations),
             semantics=dev(sc.semantics))


@pytest.mark.parametrize("mode", ["default", "strict"])
def test_widest_accepted_frame_renders(mode):
    """16368 x 16, the last width that is accepted: two Gaussians render and match the oracle."""
    cam = syn.make_camera(16368, 16, fx=16368.0)
    sc = syn.make_scene(2, cam, S=S, seed=350, scale_px=0.01, zmin=2.0, zmax=4.0, margin=0.5)

    def both_visible(fw):
        assert (fw.radii > 0).all() and fw.num_rendered > 0

    _run(cam, sc, mode, "widest_accepted", both_visible)
