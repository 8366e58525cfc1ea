"""`-m gpu` tests of per-Gaussian loads that are requested for EVERY Gaussian, in front of the test that decides whether
the Gaussian is used: the per-Gaussian backward (csrc/sgr_gauss_bwd.hip, stage 2) asks for the row sums, scales + rotation
and the clamp word together with the radius instead of behind `radius > 0`.  (The same was built for the preprocess --
opacity, scales + rotation next to the means -- and did not pay: DESIGN.md section 10; the forward checks below hold for
either schedule.)  What such a load can get wrong is a pointer that is not there (cov3D_precomp / colors_precomp calls have
no scales / rotations / SH), a lane past P, and a culled Gaussian whose value must not reach any output.  So:

  * a scene with every Gaussian behind the camera, and a mixed scene (a third behind the camera, some off screen) with
    P = 1, 255, 256, 257, 513 -- around the 256-lane workgroup;
  * each with scales + rotations, with cov3D_precomp only, and with colors_precomp only; SH degrees 0 and 3;
  * forward: radii, num_rendered and the lists identical to the C oracle's, images inside the parity gates;
  * a backward through each, against the oracle on the same forward state; culled Gaussians get zeros."""
import numpy as np
import pytest
import torch

from gpu_utils import (GRAD_NAMES, SAME_STATE_GATE, grad_close, image_close, npy, oracle_backward_same_state, raw_backward,
                       raw_forward, restrict_oracle)
from helpers import oracle_kwargs
from oracle import oracle
from street_gaussians_amd import synthetic as syn

pytestmark = pytest.mark.gpu

S = 0
FORMS = ["scales_rotations", "cov3D_precomp", "colors_precomp"]


def _scene(P, all_culled):
    cam = syn.make_camera(200, 120, fx=150.0)
    sc = syn.make_scene(P, cam, S=S, seed=900 + P, scale_px=0.02, zmin=2.0, zmax=6.0, margin=1.4)
    if all_culled:
        sc.means3D[:, 2] = -sc.means3D[:, 2]
    else:
        sc.means3D[::3, 2] = -sc.means3D[::3, 2]  # every third one behind the camera (P = 1: that one is in front, below)
        if P == 1:
            sc.means3D[:, 2] = sc.means3D[:, 2].abs()
    return cam, sc


def _kwargs(cam, sc, form, deg):
    if form == "scales_rotations":
        return oracle_kwargs(cam, sc, deg=deg, semantics=False)
    g = torch.Generator().manual_seed(5)
    if form == "colors_precomp":
        return oracle_kwargs(cam, sc, deg=deg, use_sh=False, colors=torch.rand(sc.P, 3, generator=g), semantics=False)
    fw0 = oracle.forward(**oracle_kwargs(cam, sc, deg=deg, semantics=False))
    cov6 = torch.from_numpy(fw0.cov3D.copy())
    fw0.free()
    return oracle_kwargs(cam, sc, deg=deg, use_cov_precomp=True, cov3D=cov6, semantics=False)


def _check(P, all_culled, form, deg):
    cam, sc = _scene(P, all_culled)
    kw = _kwargs(cam, sc, form, deg)
    wts = syn.loss_weights(cam, S=S)
    label = f"hoist P{P}{' culled' if all_culled else ''} {form} deg{deg}"
    fw = oracle.forward(**kw)
    res, internal = raw_forward(kw)
    b = restrict_oracle(internal, fw, kw)
    culled = fw.radii == 0
    assert culled.all() if all_culled else (culled.any() or P == 1) and not culled.all(), label
    assert res["R"] == b.num_rendered, label
    assert (npy(res["radii"]) == fw.radii).all(), label
    assert (npy(internal("tiles_touched")).view(np.uint32) == b.tiles_touched).all(), label
    if b.num_rendered:
        assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all(), label
        assert (npy(internal("keys")).view(np.uint64) == b.keys).all(), label
    assert (npy(internal("ranges")).view(np.uint32).reshape(-1) == b.ranges.reshape(-1)).all(), label
    for k in ("color", "depth", "alpha"):
        image_close(npy(res[k]), getattr(fw, k), name=f"{label}: {k}")
    g = raw_backward(kw, res, wts)
    torch.cuda.synchronize()
    same = oracle_backward_same_state(oracle, fw, res, wts, S)
    cm = torch.from_numpy(culled)
    for k in GRAD_NAMES:
        if g[k] is None or g[k].numel() == 0:
            continue
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"same-state {label}:{k}", **SAME_STATE_GATE)
        rows = g[k].reshape(P, -1).cpu()[cm]
        assert (rows == 0).all(), f"{label}: {k}: a culled Gaussian got a gradient"
    fw.free()


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("P", [1, 255, 256, 257, 513])
def test_mixed_scene(P, form, deg):
    _check(P, False, form, deg)


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("form", FORMS)
def test_every_gaussian_behind_the_camera(form, deg):
    _check(257, True, form, deg)
