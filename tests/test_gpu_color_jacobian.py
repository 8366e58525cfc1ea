"""The colour Jacobian handed from the preprocess to the per-Gaussian backward (sgr_forward_extras.color_jacobian).

A forward that asks stores J = d rgb / d dir (9 floats per visible Gaussian) in the geometry buffer and says so in its
header; the backward over such a frame forms dL/ddir = J . dL/dRGB and does not read the SH rows.  A frame that did not ask
is served by the row-reading backward.  Checked here, on the smallest scenes that reach every path (P = 1000 and 1027:
the second is no multiple of 64 or 256, so the last wave has dead lanes and the dL/dSH staging runs on a partial block;
160 x 96 pixels; SH degree 0..3 at M = 16 -- the rows the backward stages through LDS --, degree 1 at M = 4 -- float4 rows
read per lane --, and degree 1 and 2 at M = 9: 108-byte rows, not 16-byte aligned, the scalar path of both kernels; default,
exact and strict mode, and the default mode with the preprocess's LDS-staged SH copy forced):

  * the forward's outputs and exported internals are bit-identical with and without the request;
  * on one forward state, every gradient except dL/dmeans3D is bit-identical between the two backward paths, and
    dL/dmeans3D too at degree 0 (J = 0);
  * dL/dmeans3D of BOTH paths passes the gate of tests/test_gpu_parity.py::test_backward_matches_oracle against the C oracle
    on identical inputs (SAME_STATE_GATE, imported); the measured errors of both go to the parity log;
  * a frame that did not ask never reads `jac`: its region is filled with NaN bit patterns before the backward, and the
    gradients are finite and bit-identical to those from before the poisoning;
  * skip_sh_grad / masked_color_out leave dL/dmeans3D of the J path as it is; two runs with J are bit-identical."""
import functools

import numpy as np
import pytest
import torch

from gpu_utils import GRAD_NAMES, SAME_STATE_GATE, _log, dev, grad_close, npy, oracle_backward_same_state, raw_backward, raw_forward, switches
from helpers import oracle_kwargs
from jacobian_utils import asking_for_jacobian, backward_with, jacobian_flag
from oracle import oracle
from street_gaussians_amd import _C
from street_gaussians_amd import synthetic as syn

pytestmark = pytest.mark.gpu

W, H = 160, 96
AXIS = 3  # the Gaussian placed on the camera's z axis
# "staged": the preprocess form that copies the SH rows through LDS (chosen by P from 3 M Gaussians on): J is formed from
# the staged row there
MODES = {"default": lambda: 0, "exact": lambda: _C.EXACT, "strict": lambda: _C.EXACT | _C.REF_RECT,
         "staged": lambda: _C.PRE_STAGE_SH}
SHAPES = [(deg, 16) for deg in (0, 1, 2, 3)] + [(1, 4), (1, 9), (2, 9)]


@pytest.fixture(scope="module", autouse=True)
def _free_oracle_states():
    yield
    while _FORWARDS:
        _FORWARDS.pop().free()
    _case.cache_clear()


_FORWARDS = []


@functools.lru_cache(maxsize=None)
def _case(P, deg, M):
    """Scene, loss weights and the C oracle's forward (computed once, shared, left unchanged; freed with the module)."""
    cam = syn.make_camera(W, H, fx=170.0, yaw_deg=3.0, translation=(0.05, -0.02, 0.1))
    sc = syn.make_scene(P, cam, sh_degree_max={16: 3, 9: 2, 4: 1}[M], S=0, seed=7 + P + deg, margin=1.6, zmin=1.0, zmax=20.0,
                        scale_px=0.01)
    sc.shs[::5, 0, 1] -= 2.5  # one channel negative before the clamp
    sc.shs[::7, 0, :] -= 2.5  # all three
    sc.means3D[AXIS] = cam.campos + torch.tensor([2e-4, -3e-4, 4.0])  # direction within 1e-3 of the z axis
    kw = oracle_kwargs(cam, sc, deg=deg)
    fw = oracle.forward(**kw)
    _FORWARDS.append(fw)
    # ---- the scene holds what the test is about (CPU side)
    vis = fw.radii > 0
    assert (~vis).sum() >= 20 and vis.sum() >= P // 3, (int(vis.sum()), P)
    cl = np.asarray(fw.clamped).reshape(P, 3).astype(bool)
    assert (cl[vis].any(axis=1)).sum() >= 20 and (cl[vis].sum(axis=1) == 1).sum() >= 5
    d = (sc.means3D[AXIS] - cam.campos).double()
    d = d / d.norm()
    assert float((d - torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).norm()) < 1e-3 and vis[AXIS]
    return cam, sc, kw, syn.loss_weights(cam, S=0), fw, vis


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("deg,M", SHAPES)
@pytest.mark.parametrize("P", [1000, 1027])
def test_color_jacobian(P, deg, M, mode):
    cam, sc, kw, wts, fw, vis = _case(P, deg, M)
    label = f"P{P} deg{deg} M{M} {mode}"
    v = torch.from_numpy(vis).cuda()
    with switches(_C.test_switches(-1) | MODES[mode]()):
        res0, int0 = raw_forward(kw)  # did not ask
        with asking_for_jacobian():
            res1, int1 = raw_forward(kw)
        torch.cuda.synchronize()
        assert jacobian_flag(res0["geom"]) == 0 and jacobian_flag(res1["geom"]) == 1, label
        # ---- forward unchanged
        assert res0["R"] == res1["R"], label
        for k in ("color", "depth", "alpha", "radii"):
            assert torch.equal(res0[k], res1[k]), f"{label}: forward output {k} changed"
        assert np.array_equal(npy(res1["radii"]) > 0, vis), label
        for k in ("rgb", "clamped", "conic_opacity", "means2D", "depths"):  # (rows of culled Gaussians are not written)
            assert torch.equal(int0(k)[v], int1(k)[v]), f"{label}: internal {k} changed"
        for k in ("tiles_touched", "point_list", "ranges", "n_contrib"):
            assert torch.equal(int0(k), int1(k)), f"{label}: internal {k} changed"
        jac = _C.color_jacobian_view(res1["geom"], P)
        assert torch.isfinite(jac[v]).all(), label
        if deg == 0:
            assert (jac[v] == 0).all(), label
        else:
            assert (jac[v] != 0).any(), label
        if mode == "staged":  # the same J as the form that reads the rows per lane
            with switches(_C.test_switches(-1) & ~_C.PRE_STAGE_SH), asking_for_jacobian():
                res2, _ = raw_forward(kw)
            assert torch.equal(_C.color_jacobian_view(res2["geom"], P)[v], jac[v]), f"{label}: J differs from the direct form's"
        # ---- the two backward paths on their own frames (identical forward state)
        g_rows = raw_backward(kw, res0, wts)
        g_jac = raw_backward(kw, res1, wts)
        g_jac2 = raw_backward(kw, res1, wts)
        # ---- the frame that did not ask: `jac` poisoned, then the same backward again
        _C.color_jacobian_view(res0["geom"], P).view(torch.int32).fill_(0x7FC00001)
        g_rows2 = raw_backward(kw, res0, wts)
        # ---- extras on the J path
        masked = torch.full((P, 3), float("nan"), device="cuda")
        g_ex = backward_with(kw, res1, wts, skip_sh_grad=True, masked_color_out=masked)
        torch.cuda.synchronize()
    for k in GRAD_NAMES:
        assert torch.isfinite(g_rows2[k]).all(), f"{label}: {k} not finite after `jac` was poisoned"
        assert torch.equal(g_rows[k], g_rows2[k]), f"{label}: {k}: the row-reading backward looked at `jac`"
        assert torch.equal(g_jac[k], g_jac2[k]), f"{label}: {k} not deterministic with J"
        if k != "means3D" or deg == 0:
            assert torch.equal(g_rows[k], g_jac[k]), f"{label}: {k} differs between the two paths"
    assert g_ex["sh"] is None and torch.equal(g_ex["means3D"], g_jac["means3D"]), f"{label}: extras changed dL/dmeans3D"
    cl = torch.from_numpy(np.asarray(fw.clamped).reshape(P, 3).astype(bool)).cuda()
    want = torch.where(cl & v[:, None], torch.zeros_like(g_jac["colors"]), g_jac["colors"])
    assert torch.equal(masked, want), f"{label}: masked_color_out"
    # ---- dL/dmeans3D of both paths against the C oracle on identical inputs, by the parity test's gate
    same = oracle_backward_same_state(oracle, fw, res1, wts, 0)
    ref = np.asarray(same["means3D"], np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    for path, g in (("jacobian", g_jac), ("rows", g_rows)):
        a = npy(g["means3D"]).astype(np.float64).reshape(ref.shape)
        err = np.abs(a - ref)
        rec = dict(kind="color_jacobian_means3D", name=label, path=path, worst_abs_over_scale=float(err.max() / scale),
                   rms_abs_over_scale=float(np.sqrt((err ** 2).mean()) / scale))
        print(rec)
        _log(rec)
        grad_close(a, ref, name=f"color jacobian {label} ({path}): means3D", **SAME_STATE_GATE)
