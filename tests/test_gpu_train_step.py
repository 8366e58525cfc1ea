"""`-m gpu` tests of one whole training iteration (tests/train_step_gpu.py: the call site of INTEGRATION.md sections 4, 5,
9 and 11 on the scenario of tests/train_step_ref.py), in the default switch mask and in strict mode:

(a) op by op on the chain's own state: every tensor that crosses an op boundary is captured with retain_grad(), and each
    op's reference is fed the captured inputs and the captured upstream gradients of THAT op and held to the gate the op's
    own test file uses (the idea of gpu_utils.oracle_backward_same_state, applied to every stage);
(b) the three sinks (SegmentedAdam.sink, SkyAdam.sink, FlatStats.sink) against the two-step path over three iterations
    (F0, F1, F2), byte for byte;
(c) path A twice from fresh state, and once on a side stream, byte for byte;
(d) no host wait in an F1 iteration outside the rasterizer forward's one documented wait.

Every measured error goes through gpu_utils._log (committed copy: profiles/train_step/parity_measured.jsonl)."""
import contextlib

import numpy as np
import pytest
import torch

import torch_ref_frame_loss as rl
import torch_ref_sky as rs
import train_step_ref as tsr
from golden import make_actor_pose_fixture as mk
from gpu_utils import _log, grad_close, image_close, npy, oracle_backward_same_state, switches
from oracle import oracle
from test_gpu_frame_loss import GRAD, check_grad, check_scalar
from test_gpu_scene import _close
from test_gpu_sky import _op_rays
from train_step_gpu import DEV, MODES, Chain, bytes_equal, mode_mask, numpy_record

pytestmark = pytest.mark.gpu
SC = tsr.scenario()
_D = mk.load()
E_REF = {k: float(_D["e_ref_" + k]) for k in mk.KINDS}
CALLSITE = dict(rel=2e-4, abs_frac=3e-4)  # tests/test_gpu_callsite.py
FRAME_IDS = [f["name"] for f in tsr.FRAMES]


def _used(stage, name, err, bound, mode, frame):
    """Logs the largest fraction of its gate a comparison used, and returns it."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    _log(dict(kind="train_step", stage=stage, name=name, mode=mode, frame=frame, worst_over_gate=frac))
    return frac


def _f64(t):
    return t.detach().cpu().double()


# ---- (a) op by op -----------------------------------------------------------------------------------------------------
def _stage_poses(ch, frame, t, mode):
    if not frame["ids"]:
        assert t["poses"].shape == (0, 7) and t["poses"].grad_fn is None
        assert ch.ap.opt_trans.grad is None and ch.ap.opt_rots.grad is None
        return
    ot, orr = _f64(ch.ap.opt_trans).requires_grad_(True), _f64(ch.ap.opt_rots).requires_grad_(True)
    want = tsr.ref_poses(SC, frame, ot, orr)
    want.backward(_f64(t["poses"].grad))
    got = npy(t["poses"])
    for kind, x, w in (("rot", got[:, :4], want.detach().numpy()[:, :4]), ("trans", got[:, 4:], want.detach().numpy()[:, 4:]),
                       ("dtrans", npy(ch.ap.opt_trans.grad), ot.grad.numpy()), ("drots", npy(ch.ap.opt_rots.grad), orr.grad.numpy())):
        ok, need = mk.gate(kind, x, w, E_REF[kind])
        _log(dict(kind="train_step", stage="poses", name=kind, mode=mode, frame=frame["name"], worst_over_gate=need / mk.FACTOR))
        assert ok, (kind, need)
        if kind[0] == "d":
            assert not x[w == 0].any(), kind


def _model_blocks(flat, grads):
    """Per persistent model, {attribute: its block of the flat tensor `grads[attribute]`}."""
    out = []
    for m, o in zip(flat.meta, flat._offsets()):
        n = m["count"]
        d = {k: grads[k][o["row"]:o["row"] + n] for k in ("xyz", "rotation", "scaling", "opacity", "features_rest")}
        d["features_dc"] = grads["features_dc"][o["dc"]:o["dc"] + n * m["fourier_dim"] * 3]
        d["semantic"] = grads["semantic"][o["sem"]:o["sem"] + n * m["sem_width"]]
        out.append(d)
    return out


def _stage_compose(ch, frame, t, mode):
    """The bounds of tests/test_gpu_scene_frame.py (test_correction_forward_and_gradients): outputs 3e-6, leaf and pose
    gradients 2e-5, the correction's gradient 1e-4, each of the tensor's largest reference entry."""
    L = tsr.leaves64(SC, dict(correction=ch.correction))
    values = _model_blocks(ch.flat, {k: _f64(v) for k, v in ch.flat.tensors.items()})
    for model, vals in zip(L.models, values):
        for k in tsr.RAW:
            model[k] = vals[k].reshape(model[k].shape).clone().requires_grad_(True)
    poses = _f64(t["poses"]).requires_grad_(True)
    routs = tsr.ref_compose(SC, frame, L.models, poses, L.correction)
    for k, r in zip(tsr.OUT_NAMES, routs):
        _close(npy(t[k]), r.detach().numpy(), 3e-6, f"compose {k}")
    pairs = [(r, _f64(t[k].grad)) for k, r in zip(tsr.OUT_NAMES, routs) if t[k].grad is not None and r.requires_grad]
    torch.autograd.backward([r for r, _ in pairs], [u for _, u in pairs])
    got = _model_blocks(ch.flat, {k: _f64(v.grad) for k, v in ch.flat.tensors.items()})
    worst = 0.0
    for i, (model, g) in enumerate(zip(L.models, got)):
        for k in tsr.RAW:
            w = model[k].grad if model[k].grad is not None else torch.zeros_like(model[k])  # absent: zeros by the same backward
            _close(g[k].numpy().reshape(-1), w.numpy().reshape(-1), 2e-5, f"compose model {i} d_{k}")
            if w.any():
                worst = max(worst, float((g[k].reshape(-1) - w.reshape(-1)).abs().max() / w.abs().max()) / 2e-5)
    _log(dict(kind="train_step", stage="compose", name="leaf gradients", mode=mode, frame=frame["name"], worst_over_gate=worst))
    if frame["ids"]:
        _close(npy(t["poses"].grad), poses.grad.numpy(), 2e-5, "compose d_poses")
        _used("compose", "d_poses", np.abs(npy(t["poses"].grad) - poses.grad.numpy()).max(), 2e-5 * poses.grad.abs().max(), mode, frame["name"])
    _close(npy(ch.correction.grad), L.correction.grad.numpy(), 1e-4, "compose d_correction")
    _used("compose", "d_correction", np.abs(npy(ch.correction.grad) - L.correction.grad.numpy()).max(),
          1e-4 * L.correction.grad.abs().max(), mode, frame["name"])


def _summed_close(got, parts, gates, name, fracs=(2e-3, 2e-3), caps=(2e-2, 2e-2)):
    """A tensor with two producers of its gradient: `got` is autograd's sum, `parts` the references of the two, `gates` the
    (rel, abs_frac) of the owner of each.  The bound is the sum of the two bounds, element by element; so are the
    allowances for alpha-threshold flips (gpu_utils.grad_close)."""
    got = np.asarray(got, np.float64)
    want = sum(np.asarray(p, np.float64).reshape(got.shape) for p in parts)
    tol = sum(g["rel"] * np.abs(np.asarray(p, np.float64).reshape(got.shape)) + g["abs_frac"] * max(np.abs(p).max(), 1e-30)
              for p, g in zip(parts, gates))
    err = np.abs(got - want)
    bad = err > tol
    _log(dict(kind="train_step_sum", name=name, n=int(got.size), outside=int(bad.sum()), worst_over_tol=float((err / tol).max())))
    assert bad.mean() <= sum(fracs), f"{name}: {int(bad.sum())}/{got.size} outside the summed bound"
    assert err.max() <= sum(c * max(np.abs(p).max(), 1e-30) for c, p in zip(caps, parts)), name


def _stage_raster(ch, frame, t, mode):
    """Images, radii and num_rendered against the C oracle on the captured compose outputs (image_close); the composite
    head's gradients against the oracle's backward fed the captured upstream gradients and the product's own alpha image
    (oracle_backward_same_state) under test_gpu_callsite's gate; the object head against the subset forward."""
    from diff_gaussian_rasterization import GaussianRasterizer
    outs = [t[k].detach() for k in tsr.OUT_NAMES]
    captured = {k: npy(t[k].grad).copy() for k in tsr.OUT_NAMES}  # (a later backward through one head adds to .grad)
    fw = oracle.forward(**tsr.oracle_kwargs(SC, outs))
    label = f"{mode} {frame['name']}"
    assert np.array_equal(npy(t["radii"]), fw.radii)
    if mode == "strict":
        assert t["num_rendered"] == fw.num_rendered
    else:
        assert 0 < t["num_rendered"] <= fw.num_rendered
    for k in ("color", "depth", "alpha", "semantic"):
        image_close(npy(t[k]), getattr(fw, k), name=f"train step {label}: {k}")
    assert t["semantic"].grad is None  # nobody reads the semantic image: its upstream gradient is None
    H, W = SC.H, SC.W
    wts = dict(color=npy(t["color"].grad), depth=npy(t["depth"].grad), alpha=npy(t["alpha"].grad), semantic=np.zeros((SC.S, H, W), np.float32))
    g = oracle_backward_same_state(oracle, fw, dict(alpha=t["alpha"]), wts, SC.S)
    fw.free()
    comp = {k: np.asarray(g[tsr.ORACLE_OF[k]], np.float64) for k in tsr.OUT_NAMES}
    grad_close(npy(t["means2D"].grad), g["means2D"], name=f"train step {label}: means2D", **CALLSITE)
    if t["acc_obj"] is None:
        for k in tsr.OUT_NAMES:
            grad_close(captured[k].reshape(comp[k].shape), comp[k], name=f"train step {label}: d_{k}", **CALLSITE)
        return
    # ---- the object head
    split = tsr.split_of(SC, frame)
    sub = {k: t[k].detach()[split:].contiguous() for k in tsr.OUT_NAMES}
    with torch.no_grad():
        alone = GaussianRasterizer(ch.settings)(sub["means3D"], torch.zeros_like(sub["means3D"]), sub["opacities"], shs=sub["shs"], scales=sub["scales"],
                                                rotations=sub["rotations"], semantics=sub["semantics"])
    assert np.array_equal(npy(t["acc_obj"]), npy(alone[3])), "acc_obj differs from the subset forward's alpha"
    fwo = oracle.forward(**tsr.oracle_kwargs(SC, outs, lo=split))
    wo = dict(color=np.zeros((3, H, W), np.float32), depth=np.zeros((1, H, W), np.float32), alpha=npy(t["acc_obj"].grad), semantic=None)
    go = oracle_backward_same_state(oracle, fwo, dict(alpha=t["acc_obj"]), wo, 0)
    fwo.free()
    geom = ("means3D", "opacities", "scales", "rotations")
    # the head alone: a second backward through it only, with the upstream gradient the chain gave it
    alone_g = torch.autograd.grad(t["acc_obj"], [t[k] for k in geom], grad_outputs=t["acc_obj"].grad.clone(), retain_graph=True)
    obj = {}
    for k, a in zip(geom, alone_g):
        a = npy(a)
        assert not a[:split].any(), f"object head: {k} rows [0, split) are not zero"
        want = np.asarray(go[tsr.ORACLE_OF[k]], np.float64).reshape(a[split:].shape)
        grad_close(a[split:], want, name=f"train step {label}: object head d_{k}")
        obj[k] = np.zeros(a.shape)
        obj[k][split:] = want
    # both heads: the captured gradient is autograd's sum
    for k in tsr.OUT_NAMES:
        got = captured[k].reshape(comp[k].shape)
        if k in obj:
            _summed_close(got, [comp[k], obj[k].reshape(comp[k].shape)], [CALLSITE, dict(rel=1e-4, abs_frac=2e-6)],
                          f"train step {label}: both heads d_{k}")
        else:
            grad_close(got, comp[k], name=f"train step {label}: d_{k}", **CALLSITE)


def _stage_sky(ch, frame, t, mode):
    """The gs / S bounds of tests/test_gpu_sky.py::test_gradients_against_the_float64_restatement, on the op's own rays."""
    H, W = SC.H, SC.W
    rays, _ = _op_rays(H, W, ch.K, ch.w2c, ch.perturb)
    ins = [t["color"].detach().double().requires_grad_(True), t["alpha"].detach().double().requires_grad_(True),
           ch.affine.detach().double().requires_grad_(True)]
    ref = rs.render_step2(ins[0], ins[1], ch.cube.detach().double(), ch.K, ch.w2c, sky_mask=ch.sky_mask, affine=ins[2],
                          perturb=ch.perturb, d=rays.double())
    frac = {"image": _used("sky", "image", (t["image"].double() - ref).abs().max().item(), 1e-5, mode, frame["name"])}
    g = t["image"].grad.double()
    ref.backward(g)
    A = ch.affine.detach().double()
    gs = (A[:, :3].abs().T @ g.abs().reshape(3, -1)).reshape(3, H, W)  # |A|^T |g|
    rgb = t["color"].detach().double()
    c = (rgb + 1.5).abs()
    Sb = torch.einsum("ihw,jhw->ij", g.abs(), torch.cat([c, torch.ones(1, H, W, device=DEV).double()], 0))
    checks = (("d_rgb", t["color"].grad, ins[0].grad, 1e-6 * gs + 1e-30), ("d_acc", t["alpha_sky"].grad, ins[1].grad, 1e-5 * gs.sum(0, keepdim=True) + 1e-30),
              ("d_affine", ch.affine.grad, ins[2].grad, 1e-6 * Sb))
    for name, got, want, bound in checks:
        err = (got.double() - want).abs()
        frac[name] = _used("sky", name, npy(err), npy(bound), mode, frame["name"])
    assert all(v <= 1.0 for v in frac.values()), frac
    return ins[1].grad, 1e-5 * gs.sum(0, keepdim=True) + 1e-30


def _stage_loss(ch, frame, t, mode, d_acc_sky, sky_bound):
    """REL, SSIM_ABS, GRAD, PSNR_DB of tests/test_gpu_frame_loss.py against the float64 restatement on the captured images;
    then alpha, the tensor with two consumers: the captured gradient is their sum, the bound the sum of the two bounds."""
    c = lambda k: t[k].detach().cpu().double().requires_grad_(True)
    image, acc, depth = c("image"), c("alpha"), c("depth")
    acc_obj = c("acc_obj") if t["acc_obj"] is not None else None
    kw = dict(tsr.LAMBDAS, acc=acc, sky_mask=SC.sky_mask, sky_scale=tsr.SKY_SCALE, depth=depth, lidar_depth=SC.lidar.double())
    if acc_obj is not None:
        kw.update(acc_obj=acc_obj, obj_bound=SC.obj_bound)
    want = rl.frame_loss(image, SC.gt.double(), SC.mask, **kw)
    want["loss"].backward()
    vals = t["terms"].values.tolist()
    for i, k in enumerate(rl.NAMES):
        check_scalar(k, vals[i], want[k])
        bound = {"ssim": 5e-6, "psnr": 5e-5}.get(k, 5e-6 * abs(float(want[k].detach())))
        if bound:
            _used("frame_loss", k, abs(vals[i] - float(want[k].detach())), bound, mode, frame["name"])
    pairs = [("image", t["image"].grad, image.grad), ("acc", t["alpha_loss"].grad, acc.grad), ("depth", t["depth"].grad, depth.grad)]
    if acc_obj is not None:
        pairs.append(("acc_obj", t["acc_obj"].grad, acc_obj.grad))
    for k, got, w in pairs:
        check_grad(k, got, w)
        _used("frame_loss", "d_" + k, (got.cpu().double() - w).abs().max().item(), GRAD * float(w.abs().max()), mode, frame["name"])
    assert float(t["image"].grad[:, ~ch.mask[0]].abs().max()) == 0.0
    # alpha: sky composite + frame loss
    total = d_acc_sky.cpu() + acc.grad
    bound = sky_bound.cpu() + GRAD * float(acc.grad.abs().max())
    err = (t["alpha"].grad.cpu().double() - total).abs()
    assert _used("alpha", "d_alpha (two consumers)", err.numpy(), bound.numpy(), mode, frame["name"]) <= 1.0
    # autograd's sum of the two parts it was given
    assert torch.equal(t["alpha"].grad, t["alpha_sky"].grad + t["alpha_loss"].grad)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("i", range(3), ids=FRAME_IDS)
def test_op_by_op_on_the_chains_own_state(i, mode):
    frame = tsr.FRAMES[i]
    with switches(mode_mask(mode)):
        ch = Chain()
        t = ch.forward(frame, sinks=False, capture=True)
        t["loss"].backward(retain_graph=True)
        torch.cuda.synchronize()
        _stage_poses(ch, frame, t, mode)
        _stage_compose(ch, frame, t, mode)
        d_acc_sky, sky_bound = _stage_sky(ch, frame, t, mode)
        _stage_loss(ch, frame, t, mode, d_acc_sky, sky_bound)
        _stage_raster(ch, frame, t, mode)  # last: its backward through the object head alone adds to the retained .grad
        torch.cuda.synchronize()


# ---- (b) sinks against the two-step path --------------------------------------------------------------------------------
def _run(sinks, frames=tsr.FRAMES):
    """Three iterations from fresh state -> per iteration (state, step counts, record), and the chain."""
    ch = Chain()
    out = [(ch.state(), ch.counts(), None)]
    for it, frame in enumerate(frames):
        rec = ch.iterate(it, frame, sinks)
        out.append((ch.state(), ch.counts(), (numpy_record(rec), rec["flat_grads"])))
    return out, ch


def _assert_same(a, b, what):
    for it, ((sa, ca, ra), (sb, cb, rb)) in enumerate(zip(a, b)):
        assert ca == cb, f"{what}: step counts after iteration {it}"
        for k in sa:
            assert bytes_equal(sa[k], sb[k]), f"{what}: {k} after iteration {it}"
        if ra is not None:
            for k in ra[0]:
                assert bytes_equal(ra[0][k], rb[0][k]), f"{what}: {k} of iteration {it}"


@pytest.mark.parametrize("mode", list(MODES))
def test_sinks_equal_the_two_step_path_byte_for_byte(mode):
    from street_gaussians_amd.optim import ATTR, GROUPS
    with switches(mode_mask(mode)):
        A, ch = _run(True)
        B, _ = _run(False)
        torch.cuda.synchronize()
    _assert_same(A, B, "sinks vs two-step")
    layout = ch.opt.layout

    def block(state, s, g, kind):
        off, cnt, _ = layout[s][g]
        return state[f"{kind}.{ATTR[g]}"].reshape(-1)[off:off + cnt]

    for path in (A, B):
        (s0, (c0, k0), _), (s1, (c1, k1), r1), (s2, (c2, k2), r2), (s3, (c3, k3), r3) = path
        assert k3 == k0 + 3  # the cube map is stepped every iteration
        for g in GROUPS:
            # every model is in F0 and F1; the actor behind the camera in F1 is stepped all the same -- with a zero gradient,
            # so its elements move by their decaying moments
            for s in range(3):
                assert c1[s][g] == c0[s][g] + 1 and c2[s][g] == c1[s][g] + 1, (s, g)
            assert not bytes_equal(block(s1, 2, g, "p"), block(s2, 2, g, "p")), g
            # F2 renders the background only: nothing of the actors changes
            assert c3[0][g] == c2[0][g] + 1
            for s in (1, 2):
                assert c3[s][g] == c2[s][g], (s, g)
                for kind in "pmv":
                    assert bytes_equal(block(s2, s, g, kind), block(s3, s, g, kind)), (s, g, kind)
            assert not bytes_equal(block(s2, 0, g, "p"), block(s3, 0, g, "p")), g
        for k in ("opt_trans", "opt_rots"):
            assert bytes_equal(s2[k], s3[k]) and r3[0][f"grad.{k}"] is None and r2[0][f"grad.{k}"].any(), k
        assert not bytes_equal(s2["correction"], s3["correction"]) and not bytes_equal(s2["cube"], s3["cube"])
        assert not r3[0]["img.acc_obj"].any() and r2[0]["img.acc_obj"].max() > 0.05 and not r1[0]["img.acc_obj"].any()
        assert s3["denom"].sum() > 0 and s3["max_radii"].max() > 0
    # path B shows the gradient the off-screen actor was stepped with in F1: exact zeros
    grads = B[2][2][1]
    for g in GROUPS:
        off, cnt, _ = layout[2][g]
        assert not grads[ATTR[g]].reshape(-1)[off:off + cnt].any(), g
        off, cnt, _ = layout[1][g]
        assert g == "semantic" or grads[ATTR[g]].reshape(-1)[off:off + cnt].any(), g


# ---- (c) reproducibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_sink_path_is_reproducible_and_stream_independent(mode):
    with switches(mode_mask(mode)):
        first, _ = _run(True)
        again, _ = _run(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other, _ = _run(True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    _assert_same(first, again, "second run")
    _assert_same(first, other, "side stream")


# ---- (d) no host wait ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_no_host_wait_outside_the_rasterizer_forward(mode):
    @contextlib.contextmanager
    def the_one_documented_wait():
        torch.cuda.set_sync_debug_mode("default")
        try:
            yield
        finally:
            torch.cuda.set_sync_debug_mode("error")

    with switches(mode_mask(mode)):
        ch = Chain()
        ch.iterate(0, tsr.FRAMES[1], True)  # warms the allocator, the pinned staging buffers and the plan's device copy
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            rec = ch.iterate(1, tsr.FRAMES[1], True, around_raster=the_one_documented_wait, torch_adam=False)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        torch.cuda.synchronize()
    assert float(rec["values"][7]) > 0 and ch.flat.xyz.grad is None
