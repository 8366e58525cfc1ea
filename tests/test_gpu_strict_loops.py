"""`-m gpu` tests of the parity-mode blend loops after their per-visit trims (csrc/sgr_blend_bwd.hip, sgr_blend_fwd.hip,
sgr_tile_walk.h): the background branch of the backward and the one-select blend weight of the forward.

Scene: 300 Gaussians (every second one at opacity 0.9, sigma about 5 % of the image: tile lists of 107-218 entries, so the
backward takes two 128-entry rounds per tile; the C oracle has 82 % of the pixels past alpha 0.999, i.e. stopped by the
T < 1e-4 test, and the rest down to alpha 0.84) on a 48 x 32 image -- six whole tiles -- and on 44 x 30, where the six
tiles are ragged: two rows and four columns of pixels lie outside the image.

Backward.  The parity mode forms dL/dalpha's background term (backward.cu:611-614) behind a wave-uniform branch on "the
background is black" (all three components compare equal to zero).  Four backgrounds put both sides of it under test:
(0, 0, 0) and (-0.0, 0, 0) skip the term; (0.3, 0, 0.7) and (0, 0, 1e-30) form it.  Every gradient is held against the C
oracle's backward on the same forward state under SAME_STATE_GATE -- the comparison and the tolerance of
gpu_utils.strict_mode_against_reference's oracle leg.  Black and (-0.0, 0, 0) must give the same bytes: -0.0 == 0.0f takes
the same side of the branch, and on the forward side T * (-0.0) only changes the sign of a zero that is added to C >= 0.
(The parent commit, which selected between the two arms instead of branching, gives equal bytes there as well: checked on
MI355X when this test was written, tests/golden/strict_loops/README.md.)

Forward.  S = 0 and S = 5 (the S = 0 parity forward also keeps its LDS address register across the step).  No file under
tests/golden holds this scene, so the pins are of two kinds: tests/golden/strict_loops/pins.npz -- the images, n_contrib and
the hit record the PARENT commit's kernels produced for these very calls on MI355X (tests/golden/make_strict_loops_fixture.py) --
which this build must reproduce byte for byte; and the reference kernels' own files the suite already holds for these
channel counts, g2 (S = 0) and g3 (S = 5): alpha, depth, semantic image and n_contrib bit-identical, the hit list what
check_hit_list defines.  forward_layers over the full subset (split = 0: the second layer is every Gaussian) must give the
forward's colour and alpha bit for bit -- the rule of sgr_tile_walk.h."""
import functools
import os

import numpy as np
import pytest
import torch

from street_gaussians_amd import _C
from street_gaussians_amd import synthetic as syn

from golden import make_strict_loops_fixture as mk
from golden.make_golden import load_case
from gpu_utils import (SAME_STATE_GATE, _strict_mask, check_hit_list, grad_close, npy, oracle_backward_same_state, raw_backward,
                       raw_forward, switches)
from helpers import oracle_kwargs
from oracle import oracle
from test_gpu_layers import _check
from test_gpu_parity import GRAD_KEYS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BACKGROUNDS = {"black": (0.0, 0.0, 0.0), "colour": (0.3, 0.0, 0.7), "tiny": (0.0, 0.0, 1e-30), "negzero": (-0.0, 0.0, 0.0)}


def _mask(mode):
    return _strict_mask() if mode == "strict" else (_C.test_switches(-1) | _C.EXACT)


@functools.lru_cache(maxsize=None)
def _oracle(size, S, bg_name):
    """The C oracle's forward, once per call signature (kept for both modes)."""
    cam, sc = mk.scene(size, S)
    return oracle.forward(**oracle_kwargs(cam, sc, bg=torch.tensor(BACKGROUNDS[bg_name])))


@functools.lru_cache(maxsize=None)
def _run(size, mode, bg_name):
    """Forward + backward of the S = 0 scene in `mode` under background `bg_name` -> (res, {gradient name: numpy})."""
    cam, sc = mk.scene(size, 0)
    kw = oracle_kwargs(cam, sc, bg=torch.tensor(BACKGROUNDS[bg_name]))
    with switches(_mask(mode)):
        res, _ = raw_forward(kw)
        g = raw_backward(kw, res, syn.loss_weights(cam, S=0))
        torch.cuda.synchronize()
    return res, {k: npy(v).copy() for k, v in g.items()}


@pytest.mark.parametrize("bg_name", list(BACKGROUNDS))
@pytest.mark.parametrize("mode", ["strict", "exact"])
@pytest.mark.parametrize("size", mk.SIZES, ids=[f"{w}x{h}" for w, h in mk.SIZES])
def test_backward_on_both_sides_of_the_background_branch(size, mode, bg_name):
    cam, sc = mk.scene(size, 0)
    fw = _oracle(size, 0, bg_name)
    assert (fw.alpha > 0.999).mean() > 0.5 and fw.alpha.min() < 0.9, "the scene's premise: saturated and open pixels"
    res, g = _run(size, mode, bg_name)
    same = oracle_backward_same_state(oracle, fw, res, syn.loss_weights(cam, S=0), 0)
    for k in GRAD_KEYS:
        if k == "semantics":  # S = 0: empty
            continue
        assert np.abs(same[k]).max() > 0, k
        grad_close(g[k].reshape(same[k].shape), same[k], name=f"strict loops {size}/{mode}/{bg_name}: same-state {k}", **SAME_STATE_GATE)


@pytest.mark.parametrize("mode", ["strict", "exact"])
@pytest.mark.parametrize("size", mk.SIZES, ids=[f"{w}x{h}" for w, h in mk.SIZES])
def test_black_and_negative_zero_backgrounds_give_the_same_bytes(size, mode):
    (res_a, ga), (res_b, gb) = _run(size, mode, "black"), _run(size, mode, "negzero")
    for k in ("color", "depth", "alpha"):
        assert np.array_equal(npy(res_a[k]).view(np.uint32), npy(res_b[k]).view(np.uint32)), k
    for k in ga:
        assert np.array_equal(ga[k].view(np.uint32), gb[k].view(np.uint32)), f"{k}: -0.0 took another path than 0.0"
    # ... and the other side of the branch is another result: the term is not dead
    _, gc = _run(size, mode, "colour")
    assert not np.array_equal(ga["opacity"], gc["opacity"])


@pytest.mark.parametrize("S", mk.CHANNELS)
@pytest.mark.parametrize("mode", ["strict", "exact"])
@pytest.mark.parametrize("size", mk.SIZES, ids=[f"{w}x{h}" for w, h in mk.SIZES])
def test_forward_reproduces_the_parent_commits_bits_and_the_layer_kernel_agrees(size, mode, S):
    cam, sc = mk.scene(size, S)
    pins = np.load(mk.PINS)
    with switches(_mask(mode)):
        got = mk.forward_arrays(cam, sc)
        _check(cam, sc, 0, f"strict loops {size}/{mode}/S={S}")  # layer 1 = every Gaussian: the forward's bits
    assert got["alpha"].max() > 0.999 and got["n_contrib"].max() > 128
    for k, v in got.items():
        want = pins[mk.key(size, mode, S, k)]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), f"{k} differs from the parent commit's"


@pytest.mark.parametrize("mode", ["strict", "exact"])
@pytest.mark.parametrize("name", ["g2_dense_clamped_offscreen", "g3_deg0_sem5_whitebg"], ids=["S0", "S5"])
def test_forward_holds_the_reference_kernels_pins(name, mode):
    kw, _, gold = load_case(os.path.join(HERE, "golden", name + ".npz"))
    S = int(gold["semantics"].shape[1])
    H, W = int(kw["image_height"]), int(kw["image_width"])
    with switches(_mask(mode) | _C.HLIST_ALWAYS):  # (by default only the reference's rects, i.e. strict, write the compact list)
        res, internal = raw_forward(kw)
        torch.cuda.synchronize()
        arr = {k: npy(internal(k)).copy() for k in ["ranges", "n_contrib", "hits", "hit_list", "n_contrib_k"]}
    for k in ["alpha", "depth"] + (["semantic"] if S else []):
        assert np.array_equal(npy(res[k]).reshape(-1), np.asarray(gold[k]).reshape(-1)), f"{name}: {k} image not bit-identical"
    if mode == "strict":  # the reference's own lists: n_contrib counts the same entries
        assert np.array_equal(arr["n_contrib"].view(np.uint32).reshape(-1), np.asarray(gold["n_contrib"]).view(np.uint32).reshape(-1))
    assert check_hit_list(arr, H, W, name) > 0
