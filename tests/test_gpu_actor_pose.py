"""`-m gpu` tests of the per-frame actor poses (street_gaussians_amd/actor_pose.py, include/sgr_actor_pose.h): values and
gradients against the reference's executed text (tests/golden/actor_pose/pins.npz: float64 outputs, the gate
|x - ref_f64| <= 4 e_ref scale of tests/golden/actor_pose/README.md), the op-by-op parts bit for bit against the float32 restatement
(tests/torch_ref_actor_pose.py), the fixed-order gradient sum, the chain into FlatScene.compose, no host sync, the cached
plan."""
import types

import numpy as np
import pytest
import torch

import torch_ref_actor_pose as rp
from golden import make_actor_pose_fixture as mk
from street_gaussians_amd.actor_pose import ActorPoses

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
D = mk.load()
NAMES = [str(n) for n in D["names"]]
E_REF = {k: float(D["e_ref_" + k]) for k in mk.KINDS}


def _actor_poses(c, dev=DEV):
    t = lambda k: torch.from_numpy(c[k].copy()).to(dev)
    opt = bool(c["opt_track"])
    ot = torch.nn.Parameter(t("opt_trans")) if opt else None
    orr = torch.nn.Parameter(t("opt_rots")) if opt else None
    info = {int(i): dict(start_timestamp=float(s), end_timestamp=float(e))
            for i, s, e in zip(c["obj_ids"], c["obj_start"], c["obj_end"])}
    return ActorPoses(torch.from_numpy(c["track_ids"]).to(dev), t("input_trans"), t("input_rots"), c["timestamps"],
                      {0: {"train_timestamps": list(c["cam_ts"])}}, info, opt_trans=ot, opt_rots=orr)


def _plan(ap, c, key=None):
    return ap.plan([int(i) for i in c["ids"]], float(c["timestamp"]), 0, is_val=bool(c["is_val"]), key=key)


def _run(c):
    ap = _actor_poses(c)
    plan = _plan(ap, c)
    out = ap.poses(plan, torch.from_numpy(c["ego"]).to(DEV))
    res = {"rot": out[:, :4].detach().cpu().numpy(), "trans": out[:, 4:].detach().cpu().numpy()}
    if ap.opt_track:
        out.backward(torch.from_numpy(c["g"]).to(DEV))
        res["dtrans"], res["drots"] = ap.opt_trans.grad.cpu().numpy(), ap.opt_rots.grad.cpu().numpy()
    return ap, plan, res


@pytest.mark.parametrize("name", NAMES)
def test_values_and_gradients_within_the_gate(name):
    """Every case of the fixture: poses and, with opt_track, both dense gradients within 4 e_ref scale of the reference's
    float64; gradient elements that are exactly 0 in the reference are exactly 0.  The factor each case needs (of the 4
    allowed) is printed; tests/golden/actor_pose/README.md records what was measured and where."""
    c = mk.case(D, name)
    ap, plan, res = _run(c)
    assert set(res) == {k for k in mk.KINDS if k + "64" in c}
    bad = []
    for k, v in res.items():
        assert v.shape == c[k + "64"].shape and np.isfinite(v).all(), k
        ok, need = mk.gate(k, v, c[k + "64"], E_REF[k], c[k + "32"] if k[0] == "d" else None)
        print(f"actor_pose gate {name} {k}: needs {need:.3f} x e_ref")
        if not ok:
            bad.append((k, need))
    assert not bad, bad


@pytest.mark.parametrize("name", ["mid_opt", "mid_noopt", "theta_zero", "theta_flip", "offset", "before", "ego_w", "ego_x",
                                  "ego_y", "ego_z", "k65"])
def test_declared_parts_are_bitwise(name):
    """What the header declares op by op, against the float32 restatement with torch.equal: the lerp, mul_theta (on the
    kernel's own cos / sin), matrix_to_quaternion, and the ego composition (on the kernel's own Q)."""
    c = mk.case(D, name)
    ap = _actor_poses(c)
    plan = _plan(ap, c)
    assert (plan.records["n_samples"] == 1).all()
    K = len(plan)
    ego = torch.from_numpy(c["ego"]).to(DEV)
    out, parts = ap._forward(plan.on(DEV), K, ego, ap.opt_trans, ap.opt_rots, parts=True)
    out, parts = out.cpu(), parts.cpu()
    T, qa, qb, cs, qe, Q = parts[:, 0:3], parts[:, 3:7], parts[:, 7:11], parts[:, 11:15], parts[:, 15:19], parts[:, 19:23]
    f32 = torch.float32
    t = lambda k: torch.from_numpy(c[k].copy())
    ot, orr = (t("opt_trans"), t("opt_rots")) if ap.opt_track else (None, None)
    _, want = rp.poses(plan.records, t("input_trans"), t("input_rots"), ot, orr, t("ego"), f32, parts=True,
                       cs=tuple(cs[:, i] for i in range(4)))
    assert torch.equal(T, want["T"])
    assert torch.equal(qa, want["qa"]) and torch.equal(qb, want["qb"])
    assert torch.equal(qe, want["qe"].expand_as(qe))
    E = t("ego")
    rot, trans = rp.world(want["qe"], E[:3, :3], E[:3, 3], Q, T)
    assert torch.equal(out[:, :4], rot) and torch.equal(out[:, 4:], trans)
    winner = {"ego_w": 0, "ego_x": 1, "ego_y": 2, "ego_z": 3}.get(name)
    if winner is not None:  # the case is there for this candidate of matrix_to_quaternion
        assert int(qe[0].abs().argmax()) == winner


def test_k0_returns_empty_without_a_launch():
    c = mk.case(D, "mid_opt")
    ap = _actor_poses(c)
    plan = ap.plan([], float(c["timestamp"]), 0)
    out = ap.poses(plan, torch.from_numpy(c["ego"]).to(DEV))
    assert out.shape == (0, 7) and out.dtype == torch.float32 and out.is_cuda and plan.copies == 0


def test_invalid_input_raises():
    c = mk.case(D, "mid_opt")
    ap = _actor_poses(c)
    with pytest.raises(ValueError):
        ap.plan([0, 99], float(c["timestamp"]), 0)
    plan = _plan(ap, c)
    with pytest.raises(ValueError):
        ap.poses(plan, torch.eye(4, dtype=torch.float64, device=DEV))
    from street_gaussians_amd._native import SgrError
    with pytest.raises(SgrError):
        ap.poses(plan, torch.eye(4))


def test_colliding_cells_sum_in_a_fixed_order():
    """mid_opt: every actor's (frame1, column2) angle cell is another actor's own angle cell.  Two backward runs are
    bitwise equal, and the sum is the float64 sum within the gate."""
    c = mk.case(D, "mid_opt")
    cells = None
    runs = []
    for _ in range(2):
        ap, plan, res = _run(c)
        cells = plan.cells()[:, 0]
        runs.append(res)
    th1, th2 = cells[:, 2], cells[:, 3]
    assert set(th2.tolist()) & set(th1.tolist()), "the case must have coinciding cells"
    for k in ("dtrans", "drots"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
        assert mk.gate(k, runs[0][k], c[k + "64"], E_REF[k], c[k + "32"])[0], k
    # the k65 case: theta1 and theta2 of every actor share one cell, 65 actors, more than one wave in the first launch
    c = mk.case(D, "k65")
    a, b = _run(c)[2], _run(c)[2]
    for k in ("dtrans", "drots"):
        assert np.array_equal(a[k], b[k]), k


def test_gradient_writes_every_element():
    """The dense gradients are written in full: freed NaN blocks that torch.empty_like reuses do not show through."""
    c = mk.case(D, "late_opt")
    ap = _actor_poses(c)
    plan = _plan(ap, c)
    out = ap.poses(plan, torch.from_numpy(c["ego"]).to(DEV))
    junk = [torch.full_like(ap.opt_trans, float("nan")), torch.full_like(ap.opt_rots, float("nan"))]
    del junk
    out.backward(torch.from_numpy(c["g"]).to(DEV))
    assert ap.opt_trans.grad.shape == ap.opt_trans.shape and ap.opt_rots.grad.shape == ap.opt_rots.shape
    assert torch.isfinite(ap.opt_trans.grad).all() and torch.isfinite(ap.opt_rots.grad).all()
    # the (frame1, column2) cell of track 1 is an empty cell of the table and still gets its gradient
    k = [int(i) for i in c["ids"]].index(1)
    f, col = divmod(int(plan.cells()[k, 0, 3]), ap.O)
    assert c["track_ids"][f, col] == -1 and float(ap.opt_rots.grad[f, col, 0]) != 0.0


def test_chain_into_flat_compose():
    """flat.compose(poses=ap.poses(...)) on a background and two actors: the gradients that arrive in opt_trans / opt_rots
    against the float64 chain restatement -> torch_ref_scene_frame.compose_frame, within the gate."""
    import torch_ref_scene_frame as fref
    from street_gaussians_amd import scene
    from test_gpu_scene import _make, _to_gpu
    M, S = 4, 3
    c = mk.case(D, "mid_opt")
    ids = [0, 1]
    models = _make((40, 9, 7), M, S, seed=6)
    gsegs, _ = _to_gpu(models)
    flat = scene.FlatScene.from_segments(gsegs)
    ap = _actor_poses(c)
    plan = ap.plan(ids, float(c["timestamp"]), 0)
    ego = torch.from_numpy(c["ego"])
    outs = flat.compose(M, S, flip_masks=[s.flip_mask for s in gsegs], poses=ap.poses(plan, ego.to(DEV)))
    t64 = lambda k: torch.from_numpy(c[k].copy()).double()
    ot, orr = t64("opt_trans").requires_grad_(True), t64("opt_rots").requires_grad_(True)
    p64 = rp.poses(plan.records, t64("input_trans"), t64("input_rots"), ot, orr, ego, torch.float64)
    routs = fref.compose_frame(models, M, S, poses=p64)
    g = torch.Generator().manual_seed(21)
    ups = [torch.randn(r.shape, generator=g, dtype=torch.float64) for r in routs]
    torch.autograd.backward([r for r in routs if r.requires_grad], [u for r, u in zip(routs, ups) if r.requires_grad])
    torch.autograd.backward([o for o in outs if o.requires_grad], [u.float().to(DEV) for o, u in zip(outs, ups) if o.requires_grad])
    for k, got, want in (("dtrans", ap.opt_trans.grad, ot.grad), ("drots", ap.opt_rots.grad, orr.grad)):
        ok, need = mk.gate(k, got.cpu().numpy(), want.numpy(), E_REF[k])
        print(f"actor_pose chain {k}: needs {need:.3f} x e_ref")
        assert ok, (k, need)
        assert not got.cpu().numpy()[want.numpy() == 0].any(), k


def test_no_host_sync_on_a_side_stream():
    """plan + poses + backward under torch's sync debug mode, on a non-default stream; validation frame included."""
    for name in ("mid_opt", "val_two"):
        c = mk.case(D, name)
        ap = _actor_poses(c)
        ego, g = torch.from_numpy(c["ego"]).to(DEV), torch.from_numpy(c["g"]).to(DEV)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with torch.cuda.stream(side):
                plan = _plan(ap, c, key=7)
                out = ap.poses(plan, ego)
                out.backward(g)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        ok, _ = mk.gate("drots", ap.opt_rots.grad.cpu().numpy(), c["drots64"], E_REF["drots"], c["drots32"])
        assert ok


def test_cached_plan_is_not_copied_again():
    c = mk.case(D, "mid_opt")
    ap = _actor_poses(c)
    ego = torch.from_numpy(c["ego"]).to(DEV)
    plan = _plan(ap, c, key="cam3")
    assert plan.copies == 0
    a = ap.poses(plan, ego)
    assert plan.copies == 1
    again = _plan(ap, c, key="cam3")
    assert again is plan
    b = ap.poses(again, ego)
    assert plan.copies == 1 and torch.equal(a, b)
    # the same key with other arguments is a new plan
    other = ap.plan([0], float(c["timestamp"]), 0, key="cam3")
    assert other is not plan and len(other) == 1 and other.copies == 0
    # without a key nothing is kept
    assert _plan(ap, c) is not _plan(ap, c)


def test_from_reference_shares_the_parameters():
    """from_reference keeps the module's own Parameters: gradients land in them, an optimiser that holds them steps them."""
    c = mk.case(D, "mid_opt")
    t = lambda k: torch.from_numpy(c[k].copy()).to(DEV)
    tracklets_ids = torch.from_numpy(c["track_ids"]).float().to(DEV)
    module = types.SimpleNamespace(
        track_ids=tracklets_ids, input_trans=t("input_trans"), input_rots=t("input_rots"), timestamps=c["timestamps"],
        camera_timestamps={0: {"train_timestamps": []}}, opt_track=True, opt_trans=torch.nn.Parameter(t("opt_trans")),
        opt_rots=torch.nn.Parameter(t("opt_rots")),
        obj_info={int(i): dict(start_timestamp=float(s), end_timestamp=float(e))
                  for i, s, e in zip(c["obj_ids"], c["obj_start"], c["obj_end"])})
    ap = ActorPoses.from_reference(module)
    assert ap.opt_trans is module.opt_trans and ap.opt_rots is module.opt_rots
    optim = torch.optim.Adam([module.opt_trans, module.opt_rots], lr=1e-3, eps=1e-15)
    before = module.opt_rots.detach().clone()
    ap.poses(_plan(ap, c), t("ego")).backward(t("g"))
    assert mk.gate("drots", module.opt_rots.grad.cpu().numpy(), c["drots64"], E_REF["drots"], c["drots32"])[0]
    optim.step()
    assert not torch.equal(before, module.opt_rots.detach())


def _embedded(c, frames):
    """The case as the LAST rows of a table of ``frames`` frames: the rows before them are padding no track lives in
    (track_ids -1, timestamps well before the case's first), with values of their own in every tensor."""
    F0, O = c["track_ids"].shape
    pad = frames - F0
    rng = np.random.default_rng(pad)
    big = dict(c)
    big["track_ids"] = np.concatenate([np.full((pad, O), -1, np.int32), c["track_ids"]])
    for k in ("input_trans", "input_rots", "opt_trans", "opt_rots"):
        big[k] = np.concatenate([rng.standard_normal((pad,) + c[k].shape[1:]).astype(np.float32), c[k]])
    big["timestamps"] = np.concatenate([c["timestamps"][0] - 1000.0 - 0.125 * np.arange(pad, 0, -1), c["timestamps"]])
    return big, pad


@pytest.mark.parametrize("name,frames", [("mid_opt", 60_000), ("k65", 2_604)])
def test_gradient_of_a_table_past_the_zeroing_grid(name, frames):
    """A drive-length table (450 frames x 200 objects is past the cap too): the backward's first launch zeroes d_opt_trans
    grid-stride, here in two full trips and a ragged third, and the case's cells are in the third.  The plan, the poses
    and the case's gradient rows are those of the small table bit for bit (the per-address add order does not depend on the
    cell index), inside the fixture's gate; every padding row of both gradients is exactly 0.0 although the blocks
    torch.empty_like hands out were NaN.  The cap is the library's: were it raised, this fails instead of passing for
    nothing."""
    from street_gaussians_amd import _native
    c = mk.case(D, name)
    big, pad = _embedded(c, frames)
    F0, O = c["track_ids"].shape
    stride = _native.lib().sgr_actor_pose_backward_max_blocks() * 256
    assert stride > 0 and 2 * stride < 3 * frames * O < 3 * stride, \
        f"3 x {frames * O} cells no longer reach two full trips and a ragged third of {stride} threads"
    assert 3 * pad * O > 2 * stride                         # the case's own cells are zeroed by the third trip
    _, plan0, small = _run(c)

    ap = _actor_poses(big)
    plan = _plan(ap, big)
    assert np.array_equal(plan.cells(), plan0.cells() + pad * O)
    for f in ("wa", "wb", "wd", "r"):
        assert np.array_equal(plan.records["s"][f].view(np.int32), plan0.records["s"][f].view(np.int32)), f
    assert np.array_equal(plan.records["n_samples"], plan0.records["n_samples"])
    out = ap.poses(plan, torch.from_numpy(big["ego"]).to(DEV))
    junk = [torch.full_like(ap.opt_trans, float("nan")), torch.full_like(ap.opt_rots, float("nan"))]
    del junk
    out.backward(torch.from_numpy(big["g"]).to(DEV))
    got = {"rot": out[:, :4].detach().cpu().numpy(), "trans": out[:, 4:].detach().cpu().numpy()}
    for k in ("rot", "trans"):
        assert np.array_equal(got[k].view(np.int32), small[k].view(np.int32)), k
    for k, grad in (("dtrans", ap.opt_trans.grad), ("drots", ap.opt_rots.grad)):
        assert grad.shape == (frames, O, 3 if k == "dtrans" else 1)
        not_zero = int(grad[:pad].contiguous().view(torch.int32).count_nonzero())
        assert not_zero == 0, f"{k}: {not_zero} elements of the padding rows are not exactly 0.0"
        tail = grad[pad:].cpu().numpy()
        ok, need = mk.gate(k, tail, c[k + "64"], E_REF[k], c[k + "32"])
        print(f"actor_pose gate {name} in {frames} frames {k}: needs {need:.3f} x e_ref")
        assert ok, (k, need)
        assert np.array_equal(tail.view(np.int32), small[k].view(np.int32)), k
