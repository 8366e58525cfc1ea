"""CPU premises of the general-camera tests (tests/cameras.py): conditions on the matrices and on the scenes the -m gpu camera
tests use, computed from the matrices in numpy and the C oracle's radii -- not measurements of any kernel.  No GPU needed."""
import numpy as np
import pytest

import cameras
from helpers import oracle_kwargs
from oracle import oracle


@pytest.mark.parametrize("name", cameras.NAMES)
@pytest.mark.parametrize("size", [(150, 100), (48, 40), (200, 120)])
def test_named_entries_are_in_play(name, size):
    cameras.check_premises(name, *size)


def test_yaw_only_family_has_the_zero_pattern_the_table_breaks():
    """What every other rasterizer test's camera looks like, so that the table above is known to differ from it."""
    from street_gaussians_amd import synthetic as syn
    cam = syn.make_camera(150, 100, fx=165.0, yaw_deg=7.0, translation=(0.1, -0.05, 0.3))
    view, proj = cam.viewmatrix.reshape(-1).numpy(), cam.projmatrix.reshape(-1).numpy()
    assert not view[[1, 4, 6, 9]].any() and view[5] == 1.0 and not proj[[1, 4, 7, 9]].any()
    assert np.abs(proj[0::4] - 2.0 * 165.0 / 150 * view[0::4]).max() < 1e-6


@pytest.mark.parametrize("name", cameras.NAMES)
def test_gpu_scene_premises(name):
    """The scene of tests/test_gpu_cameras.py under each camera: at least 500 Gaussians with a radius, at least 20 visible
    ones past the tan-fov clamp in x and 20 in y (the clamp branch and its zeroed gradient factor run with non-zero
    off-diagonal view entries), at least 20 behind tz <= 0.2."""
    cam, sc = cameras.gpu_scene(name)
    fw = oracle.forward(**oracle_kwargs(cam, sc), internals=False)
    n_vis, n_cx, n_cy, n_behind = cameras.scene_premises(cam, sc, fw.radii)
    fw.free()
    assert n_vis >= 500 and n_cx >= 20 and n_cy >= 20 and n_behind >= 20, (n_vis, n_cx, n_cy, n_behind)
    assert n_vis < sc.P  # ... and some are culled


def test_multiview_scene_premises():
    """Every view of the multiview camera test sees a good part of the shared scene, and no view sees all of it."""
    cams, sc = cameras.multiview_scene()
    for name, cam in zip(cameras.MULTIVIEW, cams):
        fw = oracle.forward(**oracle_kwargs(cam, sc, semantics=False), internals=False)
        n_vis = int((fw.radii > 0).sum())
        fw.free()
        assert 500 <= n_vis < sc.P, (name, n_vis)
