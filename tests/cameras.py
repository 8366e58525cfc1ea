"""Named general cameras for the rasterizer tests: pitch, roll, an off-centre K, a z-up world basis, skew, and a camera
tens of metres from the origin -- what the reference's ``Camera`` hands over for a real frame, and what
``synthetic.make_camera`` (yaw about y, a symmetric frustum) never produces.

The world-to-camera rotation is ``Rz(roll) @ Rx(pitch) @ Ry(yaw) @ B`` with Ry as in make_camera; B is the identity unless
stated.  In the transposed layout the kernels read (flat index ``m[4*r+c]`` = element (c, r)):

  name        what it isolates
  pitch       pitch -12 deg, centred K, fx = fy: view[6], view[9], proj[7], proj[9]
  roll        roll 8 deg: view[1], view[4], proj[1], proj[4]
  offcentre   yaw 3 deg only, cx = 0.56 W, cy = 0.452 H, fy = 1.07 fx: the x / y rows of proj are no multiple of the rows of
              view, and the tan-fov clamp is asymmetric on the screen
  general     yaw 140, pitch -12, roll 8 deg, the off-centre K, t = (3, -1, 5)
  zup         general with B = (x forward, z up) -> OpenCV: a different zero pattern, view[5] near 0
  skewed      general with K[0, 1] = 0.02 fx
  far         zup at t = (30, -4, 55): float32 cancellation in view . p + t, as at Waymo's scale

The premises these names promise are asserted at import (conditions on the matrices, not measurements of any kernel)."""
import math

import numpy as np
import torch

from street_gaussians_amd import synthetic as syn

Z_UP = [[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]  # world (x forward, y left, z up) -> camera (x right, y down, z forward)
NEAR_T = (0.05, -0.02, 0.1)

#            yaw    pitch  roll  off-centre K  skew/fx  basis   translation
TABLE = {
    "pitch":     (0.0, -12.0, 0.0, False, 0.0, None, NEAR_T),
    "roll":      (0.0, 0.0, 8.0, False, 0.0, None, NEAR_T),
    "offcentre": (3.0, 0.0, 0.0, True, 0.0, None, NEAR_T),
    "general":   (140.0, -12.0, 8.0, True, 0.0, None, (3.0, -1.0, 5.0)),
    "zup":       (140.0, -12.0, 8.0, True, 0.0, Z_UP, (3.0, -1.0, 5.0)),
    "skewed":    (140.0, -12.0, 8.0, True, 0.02, None, (3.0, -1.0, 5.0)),
    "far":       (140.0, -12.0, 8.0, True, 0.0, Z_UP, (30.0, -4.0, 55.0)),
}
NAMES = list(TABLE)
OFF_CENTRE = [n for n in NAMES if TABLE[n][3]]
# the entries each camera is named for (|entry| >= 0.05); the composed ones exercise them together.  With yaw 140, pitch -12
# and roll 8 degrees the two terms of R[1][0] = sin(roll) cos(yaw) - cos(roll) sin(pitch) sin(yaw) nearly cancel: view[1] is
# 0.026 for `general` and `skewed` -- present, but under the bar, so it is held to 0.02 there, and proj[1] (view[1] scaled by
# 2 fy / H, less the cy share of view[2]) to being non-zero; `roll` (0.139) and `zup` (0.247) carry view[1] / proj[1] at full size
NAMED_ENTRIES = {
    "pitch": dict(view=[6, 9], proj=[7, 9]),
    "roll": dict(view=[1, 4], proj=[1, 4]),
    "general": dict(view=[4, 6, 9], proj=[4, 7, 9]),
    "zup": dict(view=[1, 4, 6, 9], proj=[1, 4, 7, 9]),
    "skewed": dict(view=[4, 6, 9], proj=[4, 7, 9]),
}
WEAK_ENTRIES = {"general": dict(view=[1]), "skewed": dict(view=[1])}


def rotation(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0, basis=None):
    """Rz(roll) @ Rx(pitch) @ Ry(yaw) @ B, float64; Ry is make_camera's rotation about the camera's y axis."""
    a, p, r = math.radians(yaw_deg), math.radians(pitch_deg), math.radians(roll_deg)
    Ry = torch.tensor([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]], dtype=torch.float64)
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(p), -math.sin(p)], [0.0, math.sin(p), math.cos(p)]], dtype=torch.float64)
    Rz = torch.tensor([[math.cos(r), -math.sin(r), 0.0], [math.sin(r), math.cos(r), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    R = Rz @ Rx @ Ry
    if basis is not None:
        R = R @ torch.tensor(basis, dtype=torch.float64)
    return R + 0.0  # (-0.0 -> 0.0: a yaw-only rotation is make_camera's matrix bit for bit)


def intrinsics(W, H, fx, off_centre=False, skew=0.0):
    if off_centre:
        return torch.tensor([[fx, skew * fx, 0.56 * W], [0.0, 1.07 * fx, 0.452 * H], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return torch.tensor([[fx, 0.0, 0.5 * W], [0.0, fx, 0.5 * H], [0.0, 0.0, 1.0]], dtype=torch.float64)


def pose(name, W, H, fx=None):
    """-> (K, R_w2c, t_w2c) of the named camera for a W x H image, float64."""
    yaw, pitch, roll, off, skew, basis, t = TABLE[name]
    fx = 1.1 * W if fx is None else fx
    return intrinsics(W, H, fx, off, skew), rotation(yaw, pitch, roll, basis), torch.tensor(t, dtype=torch.float64)


def camera(name, W, H, fx=None):
    K, R, t = pose(name, W, H, fx)
    return syn.make_camera_general(W, H, K, R, t)


def scene(name, P, W, H, fx=None, **kw):
    """-> (camera, scene placed in its view by synthetic.make_scene_in_view)."""
    K, R, t = pose(name, W, H, fx)
    cam = syn.make_camera_general(W, H, K, R, t)
    return cam, syn.make_scene_in_view(P, cam, K, R, t, **kw)


# The scene of the -m gpu camera tests: 150 x 100 px (ragged in both directions, 10 x 7 tiles), 3000 Gaussians about 2.5 px
# wide (sigma), SH degree 3, two semantic channels; pixel positions out to 1.6 times the image about the principal point
# (the tan-fov clamp is at 1.3), depths from 0.5 (some under the 0.2 cut once the splat is moved) and every 15th Gaussian
# behind the camera.  tests/test_cameras_cpu.py holds the counts this must reach, per camera.
GPU_W, GPU_H, GPU_P, GPU_S = 150, 100, 3000, 2
GPU_SCENE = dict(seed=7, scale_px=0.015, zmin=0.5, zmax=40.0, margin=1.6, behind_every=15)


def gpu_scene(name, P=GPU_P, S=GPU_S):
    return scene(name, P, GPU_W, GPU_H, S=S, **GPU_SCENE)


MULTIVIEW = ["general", "zup", "offcentre"]


def multiview_scene(per_view=1000):
    """-> ([camera per name in MULTIVIEW], one scene: `per_view` Gaussians placed in each camera's view, concatenated)."""
    pairs = [scene(n, per_view, GPU_W, GPU_H, S=0, **{**GPU_SCENE, "seed": 11 + i}) for i, n in enumerate(MULTIVIEW)]
    fields = ("means3D", "scales", "rotations", "opacities", "shs", "semantics")
    sc = syn.Scene(*[torch.cat([getattr(s, f) for _, s in pairs], 0).contiguous() for f in fields])
    return [c for c, _ in pairs], sc


def check_premises(name, W=150, H=100, fx=None):
    """The conditions the table promises, on the float32 matrices the kernels are given."""
    K, _, _ = pose(name, W, H, fx)
    cam = camera(name, W, H, fx)
    view, proj = cam.viewmatrix.reshape(-1).numpy(), cam.projmatrix.reshape(-1).numpy()
    for which, m in (("view", view), ("proj", proj)):
        for i in NAMED_ENTRIES.get(name, {}).get(which, []):
            assert abs(m[i]) >= 0.05, f"{name}: {which}[{i}] = {m[i]}"
        for i in WEAK_ENTRIES.get(name, {}).get(which, []):
            assert abs(m[i]) >= 0.02, f"{name}: {which}[{i}] = {m[i]}"
    if name in WEAK_ENTRIES:
        assert proj[1] != 0.0
    if name in OFF_CENTRE:
        # x row of proj (flat 0, 4, 8, 12) against 2 fx / W times the x row of view: the cx term mixes the z row in
        d = np.abs(proj[0::4] - 2.0 * float(K[0, 0]) / W * view[0::4])
        assert d.max() >= 0.05, f"{name}: proj x-row is proportional to view's ({d})"
        d = np.abs(proj[1::4] - 2.0 * float(K[1, 1]) / H * view[1::4])
        assert d.max() >= 0.05, f"{name}: proj y-row is proportional to view's ({d})"
    if name in ("zup", "far"):
        assert abs(view[5]) < 0.5, f"{name}: view[5] = {view[5]}"


def scene_premises(cam, sc, radii):
    """Counts the GPU tests' scenes must reach, from the matrices alone (numpy, float64) and the oracle's radii:
    -> (Gaussians with a radius, visible ones past the x clamp, past the y clamp, ones behind tz <= 0.2)."""
    m = sc.means3D.double().numpy()
    V = cam.viewmatrix.double().numpy()
    t = np.concatenate([m, np.ones((m.shape[0], 1))], 1) @ V
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    vis = np.asarray(radii) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        cx = vis & (np.abs(tx / tz) > 1.3 * cam.tanfovx)
        cy = vis & (np.abs(ty / tz) > 1.3 * cam.tanfovy)
    return int(vis.sum()), int(cx.sum()), int(cy.sum()), int((tz <= 0.2).sum())


for _n in NAMES:
    check_premises(_n)
