"""The reference leg of tests/train_step_ref.py alone, on the CPU: the conditions the `-m gpu` tests of the whole iteration
(tests/test_gpu_train_step.py) rest on, frame by frame, and a wiring check of the leg itself -- central finite differences
of its loss against its analytic gradient.  A condition that fails here means the SCENARIO has to change, not the
condition."""
import numpy as np
import pytest
import torch

import torch_ref_sky as rs
import train_step_ref as tsr

SC = tsr.scenario()
_STEPS = {}


def step(i):
    """The reference iteration of frame i, computed once and shared (nothing reads it for writing)."""
    if i not in _STEPS:
        _STEPS[i] = tsr.reference_step(SC, tsr.FRAMES[i])
    return _STEPS[i]


FRAME_IDS = [f["name"] for f in tsr.FRAMES]
GEOM_AND_COLOUR = tuple(k for k in tsr.RAW if k != "semantic")


@pytest.mark.parametrize("i", range(3), ids=FRAME_IDS)
def test_sky_share_and_terms(i):
    frame, r = tsr.FRAMES[i], step(i)
    share = float(rs.sky_mask_of(r.alpha.detach(), SC.sky_mask, True).float().mean())
    assert 0.2 <= share <= 0.8, share
    on = ["l1", "ssim", "sky", "lidar", "mse", "loss"] + (["obj"] if tsr.object_head_on(frame) else [])
    for k in on:
        v = float(r.terms[k].detach())
        assert np.isfinite(v) and v > 0, (k, v)
    if not tsr.object_head_on(frame):
        assert float(r.terms["obj"]) == 0.0 and r.fw_obj is None and r.acc_obj is None
    assert SC.H > 50 and not SC.sky_mask[:, 50:].any()  # rows below the 50 the sky-mask rule forces on, none of them sky


def test_f1_one_actor_on_screen_one_behind_the_camera():
    frame, r = tsr.FRAMES[1], step(1)
    rows = tsr.model_rows(SC, frame)
    assert float(r.fw_obj.alpha.max()) > 0.05
    assert (r.fw.radii[slice(*rows[1])] > 0).any()
    assert not r.fw.radii[slice(*rows[2])].any()
    assert not r.fw_obj.radii[rows[2][0] - rows[1][0]:].any()
    # ... while in F0 both are in view
    r0 = step(0)
    assert (r0.fw.radii[slice(*rows[1])] > 0).any() and (r0.fw.radii[slice(*rows[2])] > 0).any()


def test_f2_has_no_actor_and_no_object_head():
    frame, r = tsr.FRAMES[2], step(2)
    assert r.poses.shape == (0, 7) and tsr.split_of(SC, frame) == r.outs[0].shape[0] == tsr.COUNTS[0]
    assert not tsr.object_head_on(frame)


@pytest.mark.parametrize("i", range(3), ids=FRAME_IDS)
def test_every_gradient_block_is_alive(i):
    frame, r = tsr.FRAMES[i], step(i)
    rows = tsr.model_rows(SC, frame)
    L = r.leaves
    for m, model in enumerate(L.models):
        if m not in rows:  # absent from the frame: no gradient at all
            assert all(model[k].grad is None for k in tsr.RAW), m
            continue
        on_screen = bool((r.fw.radii[slice(*rows[m])] > 0).any())
        for k in GEOM_AND_COLOUR:
            assert bool(model[k].grad.any()) == on_screen, (m, k)
        # no term of the iteration reads the semantic image: its upstream gradient is None, the parameters get zeros
        assert not model["semantic"].grad.any(), m
    for k in ("cube", "affine", "correction"):
        assert getattr(L, k).grad.any(), k
    for k in ("opt_trans", "opt_rots"):
        g = getattr(L, k).grad
        assert (g is None) if not frame["ids"] else bool(g.any()), k
    assert np.abs(r.d_alpha_sky).max() > 0 and np.abs(r.d_alpha_loss).max() > 0  # alpha: both consumers
    assert r.g_comp["means2D"].any()
    if tsr.object_head_on(frame):
        a, b = rows[1]
        assert all(r.g_obj[k][a:b].any() and not r.g_obj[k][:a].any() for k in r.g_obj)


@pytest.mark.parametrize("i", range(3), ids=FRAME_IDS)
def test_lidar_selection_keeps_95_percent(i):
    r = step(i)
    n = int(((SC.lidar > 0) & SC.mask).sum())
    assert n >= 100 and int((r.d_depth != 0).sum()) == int(0.95 * n) < n


# ---- the wiring of the reference leg: finite differences ---------------------------------------------------------------
AFTER_STEP = 1e-7
BEFORE_STEP = 2e-3


def _head_loss(r, frame, cube, affine):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    acc_obj = t(r.fw_obj.alpha) if r.fw_obj is not None else None
    _, terms = tsr.head(SC, frame, t(r.fw.color), t(r.fw.depth), t(r.fw.alpha), t(r.fw.alpha), acc_obj, cube, affine)
    return float(terms["loss"])


def _central(f, base, idx, h):
    out = []
    for s in (+1.0, -1.0):
        v = base.detach().double().clone()
        v[idx] += s * h
        out.append(f(v))
    return (out[0] - out[1]) / (2.0 * h)


def test_finite_differences_after_the_rasterizer():
    """F1, on the oracle's fixed images, float64 throughout: the 12 entries of `affine` and the 8 cube texels with the
    largest gradients, central differences with h = 1e-7.  Measured: worst |fd - analytic| = 1.0e-8 x max |analytic| for
    affine, 7.7e-8 x for the texels (the rounding of a loss near 0.9 in double, 1e-16 / h = 1e-9, against gradients of
    0.04 and 0.012); the gate is 1e-6 x."""
    frame, r = tsr.FRAMES[1], step(1)
    L = r.leaves
    ga, gc = L.affine.grad, L.cube.grad
    worst = 0.0
    for i in range(3):
        for j in range(4):
            fd = _central(lambda v: _head_loss(r, frame, L.cube.detach(), v), L.affine, (i, j), AFTER_STEP)
            worst = max(worst, abs(fd - float(ga[i, j])) / float(ga.abs().max()))
    print(f"affine: worst |fd - analytic| / max |analytic| = {worst:.3e}")
    assert worst <= 1e-6
    top = torch.topk(gc.abs().reshape(-1), 8).indices
    worst = 0.0
    for flat in top.tolist():
        idx = tuple(int(x) for x in np.unravel_index(flat, tuple(gc.shape)))
        fd = _central(lambda v: _head_loss(r, frame, v, L.affine.detach()), L.cube, idx, AFTER_STEP)
        worst = max(worst, abs(fd - float(gc[idx])) / float(gc.abs().max()))
    print(f"cube: worst |fd - analytic| / max |analytic| = {worst:.3e}")
    assert worst <= 1e-6


def test_finite_differences_before_the_rasterizer():
    """F1, through the float32 oracle: the 7 entries of `correction` and the `opt_trans` row of the on-screen actor's
    first tracklet cell, central differences against the analytic gradient, gated at 5 % of the largest analytic entry
    -- a dropped consumer or a missing factor is an error of 50 % or more.

    The step was chosen by measuring on the reference leg itself.  The rasterizer's forward is only piecewise smooth (a
    Gaussian is dropped from a pixel below alpha = 1 / 255 and outside its 3-sigma rect), so small steps read the jumps
    (h = 3e-4: up to 10 %) and large ones the curvature (h = 1e-2: up to 17 %).  In between the worst entry reads, for
    correction / opt_trans: 5.0 / 5.2 % at h = 1e-3, 4.5 / 4.0 % at 2e-3, 4.8 / 5.3 % at 3e-3, 4.5 / 4.1 % at 5e-3.  What is
    left there does not fall with h: the analytic gradient of the reference algorithm leaves out the movement of those
    cut-off edges, which does not cancel where the background ends against the sky and at an actor's outline (the
    scenario's splats are opaque for that reason: with translucent ones the same comparison reads 8 to 15 %).
    h = 2e-3."""
    frame, r = tsr.FRAMES[1], step(1)
    loss = lambda name: (lambda v: tsr.reference_step(SC, frame, {name: v}, backward=False).loss)
    gc = r.leaves.correction.grad.numpy()
    fd = np.array([_central(loss("correction"), SC.correction, (i,), BEFORE_STEP) for i in range(7)])
    worst_c = np.abs(fd - gc).max() / np.abs(gc).max()
    ot = torch.from_numpy(SC.tracklets["opt_trans"])
    cell = (2, 0)  # frame 2, column 0: the nearer sample of actor 0 at F1's timestamp
    gt = r.leaves.opt_trans.grad.numpy()[cell]
    fd_t = np.array([_central(loss("opt_trans"), ot, cell + (j,), BEFORE_STEP) for j in range(3)])
    worst_t = np.abs(fd_t - gt).max() / np.abs(gt).max()
    print(f"correction: worst {worst_c:.4f}, opt_trans{list(cell)}: worst {worst_t:.4f} of the largest analytic entry")
    assert np.abs(gc).max() > 0 and np.abs(gt).max() > 0
    assert worst_c <= 0.05 and worst_t <= 0.05, (worst_c, worst_t)
