"""`-m gpu` tests of the shared tile walk (csrc/sgr_tile_walk.h) at its loop boundaries.

Every blend kernel -- forward, layers, object alpha forward and backward, blend backward -- takes its survivor loop from
sgr_walk_pairs: the odd survivor first, then pairs, per 64-entry chunk of a 256-entry (backward: 128-entry) batch.  One
scene per list length N around those boundaries: a 16 x 16 image (ONE tile), N wide, faint Gaussians centred in it at
distinct depths, so that every pixel blends every Gaussian and none terminates -- the walk visits all N entries in all four
quadrants.  That premise is asserted (n_contrib == N in every pixel, from the C oracle alone and from the kernel); the
numbers behind it: sigma 18-22 px with the centres within 2 px of the image centre puts every pixel within 14.2 px, G >= 0.73,
alpha = opacity * G in [0.011, 0.02] -- almost three times the 1/255 cut -- and T >= 0.98^257 = 5.5e-3, fifty times the 1e-4 stop.

Per N and mode: the forward against the C oracle (gpu_utils.image_close at its defaults, the comparison of
test_gpu_parity.test_forward_matches_oracle) and the blend backward against the oracle's backward on the same forward state
(SAME_STATE_GATE, as test_gpu_parity.test_backward_matches_oracle); forward_layers bit for bit against the forwards over
the two subsets (test_gpu_layers._check); forward_with_object_alpha's image bit for bit against the subset forward's alpha and
its gradients against the subset render's backward, compared as
test_gpu_object_alpha.test_small_case_equals_the_subset_render_and_its_backward compares them (grad_close at its defaults and
exact zeros in rows [0, split): the two backwards sum the same terms in different orders).  The split is N // 2 by index;
depths are shuffled, so the two layers interleave in the tile's list."""

import functools

import numpy as np
import pytest
import torch

from street_gaussians_amd import _C
from street_gaussians_amd import synthetic as syn

from gpu_utils import SAME_STATE_GATE, grad_close, image_close, npy, oracle_backward_same_state, raw_backward, raw_forward, switches
from helpers import oracle_kwargs
from oracle import oracle
from test_gpu_layers import _check
from test_gpu_object_alpha import FRAME_BG, _compare, _head, _weight, _yardstick
from test_gpu_parity import GRAD_KEYS

pytestmark = pytest.mark.gpu

SIDE = 16
NS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def _scene(N):
    """-> (cam, scene, split)"""
    fx = 20.0
    cam = syn.make_camera(SIDE, SIDE, fx=fx)
    g = torch.Generator().manual_seed(N)
    z = torch.linspace(2.0, 6.0, N + 1)[:N][torch.randperm(N, generator=g)]
    off = (torch.rand(N, 2, generator=g) * 4.0 - 2.0) / fx  # +-2 px around the principal point
    means = torch.stack([off[:, 0] * z, off[:, 1] * z, z], 1)
    # mildly anisotropic: the rotation gradient of a sphere is analytically zero (tests/test_gpu_object_alpha.py)
    scales = (20.0 * z / fx)[:, None] * torch.tensor([0.9, 1.0, 1.1])
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(N, 1)
    opac = 0.015 + 0.005 * torch.rand(N, 1, generator=g)
    shs = torch.zeros(N, 16, 3)
    shs[:, 0] = torch.rand(N, 3, generator=g) * 2.0 - 1.0
    sc = syn.Scene(means.contiguous(), scales.contiguous(), rot, opac, shs, torch.zeros(N, 0))
    return cam, sc, N // 2


@functools.lru_cache(maxsize=None)
def _oracle(N):
    """The C oracle's forward of scene N, computed once and kept for both modes."""
    cam, sc, _ = _scene(N)
    return oracle.forward(**oracle_kwargs(cam, sc, bg=FRAME_BG))


@pytest.mark.parametrize("mask", [0, _C.EXACT], ids=["default", "exact"])
@pytest.mark.parametrize("N", NS)
def test_forward_and_backward_against_the_oracle(N, mask):
    cam, sc, _ = _scene(N)
    fw = _oracle(N)
    assert (fw.n_contrib == N).all(), "the scene's premise: every pixel blends every Gaussian (oracle)"
    assert fw.alpha.max() < 1.0 - 1e-3, "... and no pixel comes near the T < 1e-4 stop"
    kw = oracle_kwargs(cam, sc, bg=FRAME_BG)
    wts = syn.loss_weights(cam, S=0)
    with switches(mask):
        res, internal = raw_forward(kw)
        nc = npy(internal("n_contrib")).view(np.uint32).reshape(SIDE, SIDE)
        g = raw_backward(kw, res, wts)
        torch.cuda.synchronize()
    assert (nc == N).all(), "every pixel blends every Gaussian (kernel)"
    for k in ("color", "depth", "alpha"):
        image_close(npy(res[k]), getattr(fw, k), name=f"tile walk N={N}/{mask}: {k}")
    same = oracle_backward_same_state(oracle, fw, res, wts, 0)
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"tile walk N={N}/{mask}: same-state {k}", **SAME_STATE_GATE)


@pytest.mark.parametrize("mask", [0, _C.EXACT], ids=["default", "exact"])
@pytest.mark.parametrize("N", NS)
def test_layers_and_object_alpha_equal_the_subset_renders(N, mask):
    cam, sc, split = _scene(N)
    w = _weight(cam)
    with switches(mask):
        _check(cam, sc, split, f"tile walk N={N}/{mask}")
        want_alpha, want = _yardstick(cam, sc, split, w)
        got, grads = _head(cam, sc, split, w)
    assert np.array_equal(got["acc"], want_alpha), "acc_object differs from the subset forward's alpha"
    assert want_alpha.min() > 0.0
    _compare(grads, want, split, f"tile walk N={N}/{mask}")
