"""`-m gpu` tests of the per-frame compose (include/sgr_scene_frame.h, scene.FlatScene.compose(segments=, correction=),
scene.compose(correction=)): frame subsets against the per-model path, the camera pose correction against the torch
restatement of the reference (tests/torch_ref_scene_frame.py), its deterministic two-level reduction, and a short
flat-mode training loop against the per-model path with torch.optim.Adam."""
import pytest
import torch

import torch_ref_scene_frame as fref
from street_gaussians_amd import scene
from test_gpu_scene import _close, _make, _to_gpu

pytestmark = pytest.mark.gpu
M, S = 16, 5
COUNTS = (700, 300, 0, 257, 129, 64)  # background, then actors (one empty)


def _flat_and_masks(seed=2):
    gsegs, _ = _to_gpu(_make(COUNTS, M, S, seed))
    return scene.FlatScene.from_segments(gsegs), [s.flip_mask for s in gsegs]


def _pose_rows(flat):
    rows, a = {}, 0
    for i, m in enumerate(flat.meta):
        if m["kind"] == scene.SEG_ACTOR:
            rows[i] = a
            a += 1
    return rows


def _per_model(flat, idx, masks):
    """scene.Segment leaves of the models `idx`, cloned from flat.views() (independent autograd leaves)."""
    views, rows = flat.views(), _pose_rows(flat)
    out = []
    for i in idx:
        v, m = views[i], flat.meta[i]
        leaf = lambda t: t.detach().clone().requires_grad_(True)
        out.append(scene.Segment(
            xyz=leaf(v["xyz"]), rotation=leaf(v["rotation"]), scaling=leaf(v["scaling"]), opacity=leaf(v["opacity"]),
            features_dc=leaf(v["features_dc"]), features_rest=leaf(v["features_rest"]),
            semantic=leaf(v["semantic"]) if m["sem_width"] else None,
            pose=leaf(flat.poses[rows[i]]) if m["kind"] == scene.SEG_ACTOR else None, idft=m["idft"],
            flip_mask=masks[i], class_label=m["class_label"], semantic_mode=m["semantic_mode"],
            flip_axis=m["flip_axis"], flip_quat=m["flip_quat"]))
    return out


def _backward(outs, seed):
    g = torch.Generator().manual_seed(seed)
    ups = [torch.randn(o.shape, generator=g).cuda() for o in outs]
    torch.autograd.backward([o for o in outs if o.requires_grad], [u for o, u in zip(outs, ups) if o.requires_grad])


def _zero_grads(flat):
    for t in list(flat.tensors.values()) + [flat.poses]:
        t.grad = None


def _check_blocks(flat, idx, segs, want_pose_rows=True):
    """Present blocks of the flat gradients equal the per-model leaves' gradients bit for bit; absent blocks are 0."""
    offs, rows = flat._offsets(), _pose_rows(flat)
    fg = {k: flat.tensors[k].grad for k in scene._FLAT}
    seen = set()
    for i, seg in zip(idx, segs):
        seen.add(i)
        m, o = flat.meta[i], offs[i]
        n = m["count"]
        for name in ("xyz", "rotation", "scaling", "opacity"):
            assert torch.equal(getattr(seg, name).grad, fg[name][o["row"]:o["row"] + n]), (i, name)
        assert torch.equal(seg.features_rest.grad.flatten(1), fg["features_rest"][o["row"]:o["row"] + n]), i
        assert torch.equal(seg.features_dc.grad.reshape(-1), fg["features_dc"][o["dc"]:o["dc"] + n * m["fourier_dim"] * 3]), i
        if seg.semantic is not None:
            assert torch.equal(seg.semantic.grad.reshape(-1), fg["semantic"][o["sem"]:o["sem"] + n * m["sem_width"]]), i
        if seg.pose is not None and want_pose_rows:
            assert torch.equal(seg.pose.grad, flat.poses.grad[rows[i]]), i
    for i, (m, o) in enumerate(zip(flat.meta, offs)):
        if i in seen:
            continue
        n = m["count"]
        for name in ("xyz", "rotation", "scaling", "opacity", "features_rest"):
            assert not fg[name][o["row"]:o["row"] + n].any(), (i, name)
        assert not fg["features_dc"][o["dc"]:o["dc"] + n * m["fourier_dim"] * 3].any(), i
        assert not fg["semantic"][o["sem"]:o["sem"] + n * m["sem_width"]].any(), i
        if i in rows and want_pose_rows:
            assert not flat.poses.grad[rows[i]].any(), i


@pytest.mark.parametrize("idx", [[0, 4, 1, 3], [3, 0, 5], [5, 1, 3], [0], [4], [0, 2], [2, 4]],
                         ids=["reordered", "background-inside", "actors-only", "background-only", "single-actor",
                              "empty-actor", "empty-actor-first"])
def test_subset_equals_per_model_compose(idx):
    """(a) FlatScene.compose(segments=idx) == scene.compose on the per-model leaves of the same subset, bit for bit,
    outputs and present gradient blocks; absent blocks and absent pose rows exactly 0."""
    flat, masks = _flat_and_masks()
    segs = _per_model(flat, idx, masks)
    outs = scene.compose(segs, M, S)
    fouts = flat.compose(M, S, flip_masks=[masks[i] for i in idx], segments=idx)
    for a, b in zip(outs, fouts):
        assert torch.equal(a, b)
    _backward(outs, 7)
    # NaN-filled blocks freed just before the backward: its torch.empty_like gradients reuse them, so an element the
    # kernels or the zero spans miss shows up
    junk = [torch.full_like(t, float("nan")) for t in list(flat.tensors.values()) + [flat.poses]]
    del junk
    _backward(fouts, 7)
    _check_blocks(flat, idx, segs)
    for t in flat.tensors.values():
        assert t.grad.shape == t.shape and torch.isfinite(t.grad).all()


def test_subset_with_frame_poses_and_idfts():
    """(a) poses given in frame order (a non-leaf) and explicit IDFT rows for a subset: the held leaf gets no gradient."""
    flat, masks = _flat_and_masks(seed=3)
    idx, rows = [0, 5, 3], _pose_rows(flat)
    raw = torch.stack([flat.poses[rows[5]], flat.poses[rows[3]]]).detach().clone().requires_grad_(True)
    idfts = [None, flat.meta[5]["idft"], flat.meta[3]["idft"]]
    fouts = flat.compose(M, S, flip_masks=[masks[i] for i in idx], poses=raw * 1.0, idfts=idfts, segments=idx)
    segs = _per_model(flat, idx, masks)
    outs = scene.compose(segs, M, S)
    for a, b in zip(outs, fouts):
        assert torch.equal(a, b)
    _backward(outs, 8)
    _backward(fouts, 8)
    _check_blocks(flat, idx, segs, want_pose_rows=False)
    assert flat.poses.grad is None
    assert torch.equal(raw.grad[0], segs[1].pose.grad) and torch.equal(raw.grad[1], segs[2].pose.grad)


def test_full_segment_list_equals_default():
    """(b) segments=list(range(K)) is the default call, bit for bit."""
    flat, masks = _flat_and_masks(seed=4)
    outs = flat.compose(M, S, flip_masks=masks)
    _backward(outs, 9)
    want = [t.grad.clone() for t in list(flat.tensors.values()) + [flat.poses]]
    _zero_grads(flat)
    fouts = flat.compose(M, S, flip_masks=masks, segments=list(range(len(COUNTS))))
    for a, b in zip(outs, fouts):
        assert torch.equal(a, b)
    _backward(fouts, 9)
    for a, t in zip(want, list(flat.tensors.values()) + [flat.poses]):
        assert torch.equal(a, t.grad)


def _correction(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randn(4, generator=g, dtype=torch.float64) * scale, torch.randn(3, generator=g, dtype=torch.float64)])


@pytest.mark.parametrize("cscale", [1.0, 0.01, 30.0])
def test_correction_forward_and_gradients(cscale):
    """(c) forward within a few ulp of the reference's torch formulation on the GPU; every gradient, the correction's
    included, within tolerance of the float64 restatement; the flat path equals the per-model path bit for bit."""
    counts = (20_000, 700, 300)
    models = _make(counts, M, S, seed=5)
    gsegs, gleaves = _to_gpu(models)
    c64 = _correction(11, cscale)
    corr_rots = c64[:4].float().cuda().requires_grad_(True)
    corr_trans = c64[4:].float().cuda().requires_grad_(True)
    corr = torch.cat([corr_rots, corr_trans])  # the per-image leaves behind a cat, as the caller builds it
    outs = scene.compose(gsegs, M, S, correction=corr)
    plain = scene.compose(gsegs, M, S)
    # forward: the torch formulation of correct_gaussian_xyz / _rotation (float32, GPU) applied to the uncorrected rows
    n0 = counts[0]
    c32 = corr.detach()
    want_x = fref.correct_xyz(c32, plain[0][:n0].detach())
    want_q = fref.correct_rotation(c32, plain[1][:n0].detach())
    eps = 2.0 ** -23
    x0 = plain[0][:n0].detach()
    bound_x = 8 * eps * (x0.abs().sum(1, keepdim=True) + c32[4:].abs()[None])
    assert bool(((outs[0][:n0] - want_x).abs() <= bound_x).all())
    assert float((outs[1][:n0].detach() - want_q).abs().max()) <= 8 * eps
    for k in range(2, 6):
        assert torch.equal(outs[k], plain[k])
    assert torch.equal(outs[0][n0:], plain[0][n0:]) and torch.equal(outs[1][n0:], plain[1][n0:])
    # gradients against float64
    rleaves = []
    for d in models:
        for n in ("xyz", "rotation", "scaling", "opacity", "features_dc", "features_rest", "semantic", "pose"):
            if d.get(n) is not None:
                d[n] = d[n].clone().requires_grad_(True)
                rleaves.append(d[n])
    c64 = c64.clone().requires_grad_(True)
    routs = fref.compose_frame(models, M, S, correction=c64)
    for o, r, name in zip(outs, routs, ["means3D", "rotations", "scales", "opacities", "shs", "semantics"]):
        _close(o.detach().cpu().numpy(), r.detach().numpy(), 3e-6, name)
    g = torch.Generator().manual_seed(12)
    ups = [torch.randn(r.shape, generator=g, dtype=torch.float64) for r in routs]
    torch.autograd.backward(list(routs), ups)
    torch.autograd.backward(list(outs), [u.float().cuda() for u in ups])
    for i, (a, b) in enumerate(zip(gleaves, rleaves)):
        _close(a.grad.cpu().numpy(), b.grad.numpy(), 2e-5, f"grad[{i}] shape {tuple(b.shape)}")
    got = torch.cat([corr_rots.grad, corr_trans.grad]).cpu().numpy()
    _close(got, c64.grad.numpy(), 1e-4, "correction grad")
    # flat path, background + a subset, against the per-model path with the same correction
    flat = scene.FlatScene.from_segments(gsegs)
    idx = [0, 2]
    segs = _per_model(flat, idx, [s.flip_mask for s in gsegs])
    cf = corr.detach().clone().requires_grad_(True)
    cp = corr.detach().clone().requires_grad_(True)
    fouts = flat.compose(M, S, flip_masks=[gsegs[i].flip_mask for i in idx], segments=idx, correction=cf)
    pouts = scene.compose(segs, M, S, correction=cp)
    for a, b in zip(fouts, pouts):
        assert torch.equal(a, b)
    _backward(fouts, 13)
    _backward(pouts, 13)
    _check_blocks(flat, idx, segs)
    assert torch.equal(cf.grad, cp.grad)
    # actors only: the correction does not apply and its gradient is 0
    ca = corr.detach().clone().requires_grad_(True)
    aouts = flat.compose(M, S, flip_masks=[gsegs[i].flip_mask for i in (1, 2)], segments=[1, 2], correction=ca)
    bouts = flat.compose(M, S, flip_masks=[gsegs[i].flip_mask for i in (1, 2)], segments=[1, 2])
    for a, b in zip(aouts, bouts):
        assert torch.equal(a, b)
    _backward(aouts, 14)
    assert not ca.grad.any()


@pytest.mark.parametrize("n_bg", [70_001, 5_000_000])
def test_correction_gradient_is_bitwise_reproducible(n_bg):
    """(d) the two-level reduction: the same bits on every run and on another stream, up to 5 M background Gaussians."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen, device="cuda")
    bk = scene.Segment(xyz=r(n_bg, 3) * 10, rotation=r(n_bg, 4), scaling=r(n_bg, 3), opacity=r(n_bg, 1),
                       features_dc=r(n_bg, 1, 3), features_rest=r(n_bg, 0, 3))
    act = scene.Segment(xyz=r(1000, 3), rotation=r(1000, 4), scaling=r(1000, 3), opacity=r(1000, 1),
                        features_dc=r(1000, 1, 3), features_rest=r(1000, 0, 3), pose=r(7))
    ups = [r(n_bg + 1000, 3), r(n_bg + 1000, 4)]
    c = torch.tensor([0.9, 0.1, -0.2, 0.05, 0.3, -0.1, 0.2], device="cuda")

    def run():
        cc = c.clone().requires_grad_(True)
        outs = scene.compose([bk, act], 1, 0, correction=cc)
        torch.autograd.backward(list(outs[:2]), ups)
        return cc.grad
    first = run()
    assert torch.isfinite(first).all() and first.abs().max() > 0
    for _ in range(2):
        assert torch.equal(run(), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(other, first)
    # against float64 sums of the same terms
    with torch.no_grad():
        c64 = c.double().requires_grad_(True)
    with torch.enable_grad():
        xb = bk.xyz.detach().double()
        qb = torch.nn.functional.normalize(bk.rotation.detach().double())
        x2, q2 = fref.correct_xyz(c64, xb), fref.correct_rotation(c64, qb)
        torch.autograd.backward([x2, q2], [ups[0][:n_bg].double(), ups[1][:n_bg].double()])
    _close(first.cpu().numpy(), c64.grad.cpu().numpy(), 1e-4, "correction grad")


def test_repeated_segment_index_raises():
    """(f)"""
    flat, masks = _flat_and_masks()
    with pytest.raises(ValueError, match="at most once"):
        flat.compose(M, S, segments=[0, 3, 0])


# ---- (e) a short flat-mode training loop against the per-model path ---------------------------------------------
def test_flat_mode_loop_with_frame_subsets_matches_per_model_path():
    """Frames with different in_frame, each with a full render (stats sink, colour loss) and an actors-only render with
    the object-accumulation loss (train.py:114-122); FlatScene + FlatStats.sink(models=) + SegmentedAdam.step(segments=)
    against scene.compose + densification_stats + one torch.optim.Adam per model.  The first step's images are equal bit
    for bit; parameters and moments agree within test_gpu_optim's tolerance."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gpu_utils import settings
    from street_gaussians_amd import losses, synthetic as syn
    from street_gaussians_amd.optim import ATTR, GROUPS, SegmentedAdam
    from test_gpu_optim import _compare, _torch_models
    cam = syn.make_camera(320, 200, fx=300.0)
    sc = syn.make_scene(3000, cam, S=0, seed=4)
    g = torch.Generator().manual_seed(8)
    r = lambda *s: torch.randn(*s, generator=g)
    Sx = 2
    segs = [scene.Segment(xyz=sc.means3D.cuda(), rotation=sc.rotations.cuda(), scaling=sc.scales.log().cuda(),
                          opacity=torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)).cuda(), features_dc=sc.shs[:, :1].cuda(),
                          features_rest=sc.shs[:, 1:].cuda(), semantic=r(3000, Sx).cuda())]
    for k, n in enumerate((400, 250, 300)):
        segs.append(scene.Segment(
            xyz=(r(n, 3) * 0.4).cuda(), rotation=r(n, 4).cuda(), scaling=torch.full((n, 3), -3.0).cuda(),
            opacity=r(n, 1).cuda(), features_dc=(r(n, 3, 3) * 0.3).cuda(), features_rest=(r(n, 15, 3) * 0.05).cuda(),
            semantic=r(n, 1).cuda(), pose=torch.tensor([0.9, 0.1 * k, -0.2, 0.3, 0.8 * (k - 1), -0.2, 6.0 + k]).cuda(),
            idft=torch.tensor([0.7, -0.4, 0.2]).cuda(), class_label=k % Sx))
    flat = scene.FlatScene.from_segments(segs)
    flat.poses.requires_grad_(False)
    K = len(segs)
    lrs = [{gr: 1e-6 * (1 + s) for gr in GROUPS} for s in range(K)]
    opt = SegmentedAdam(flat, lrs)
    models = _torch_models(flat, lrs)
    stats = scene.FlatStats([m["count"] for m in flat.meta], "cuda")
    pstats = [{k: torch.zeros_like(v) for k, v in m.items()} for m in stats.views()]
    rows = _pose_rows(flat)
    obj_bound = torch.zeros(cam.image_height, cam.image_width, dtype=torch.bool, device="cuda")
    obj_bound[60:140, 100:220] = True
    w = syn.loss_weights(cam, seed=3)["color"].cuda()
    frames = [[0, 1, 2, 3], [0, 3, 1], [0, 2], [0, 1, 3]]

    def per_model_segments(idx):
        out = []
        for i in idx:
            ps, m = models[i][0], flat.meta[i]
            out.append(scene.Segment(
                xyz=ps["xyz"], rotation=ps["rotation"], scaling=ps["scaling"], opacity=ps["opacity"],
                features_dc=ps["f_dc"], features_rest=ps["f_rest"], semantic=ps["semantic"],
                pose=flat.poses[rows[i]].detach() if i in rows else None, idft=m["idft"], class_label=m["class_label"],
                semantic_mode=m["semantic_mode"]))
        return out

    def render(compose_fn, idx, sink=None):
        means3D, rot, scales, opac, shs, sem = compose_fn(idx)
        rast = GaussianRasterizer(settings(cam))
        m2d = torch.zeros(means3D.shape[0], 3, device="cuda", requires_grad=True)
        if sink is not None:
            rast.stats_sink = sink
        color, radii, depth, alpha, semo = rast(means3D, m2d, opac, shs=shs, scales=scales, rotations=rot, semantics=sem)
        return color, radii, alpha, m2d

    for it, in_frame in enumerate(frames):
        actors = [i for i in in_frame if i in rows]
        # flat mode
        fc = lambda idx: flat.compose(M, Sx, segments=idx)
        color_f, _, _, _ = render(fc, in_frame, sink=stats.sink(models=in_frame))
        obj_f, _, acc_f, _ = render(fc, actors)
        loss_f = (color_f * w).sum() + 0.1 * losses.obj_acc_loss(acc_f, obj_bound)
        loss_f.backward()
        opt.step(segments=in_frame)
        for t in flat.tensors.values():
            t.grad = None
        # per-model path
        pc = lambda idx: scene.compose(per_model_segments(idx), M, Sx)
        color_p, radii_p, _, m2d_p = render(pc, in_frame)
        obj_p, _, acc_p, _ = render(pc, actors)
        loss_p = (color_p * w).sum() + 0.1 * losses.obj_acc_loss(acc_p, obj_bound)
        loss_p.backward()
        scene.densification_stats([pstats[i] for i in in_frame], m2d_p.grad, radii_p)
        for ps, topt in models:
            topt.step()
            topt.zero_grad(set_to_none=True)
        if it == 0:
            assert torch.equal(color_f, color_p) and torch.equal(obj_f, obj_p) and torch.equal(acc_f, acc_p)
            assert float(acc_p.detach().max()) > 0.05  # the actors are in view
    torch.cuda.synchronize()
    bitwise = []
    _compare(opt, flat, models, K=64, bitwise=bitwise)
    # statistics: the paths' parameters differ in the last bits after the first step, so a radius may round apart
    for a, b in zip(stats.views(), pstats):
        assert float((a["denom"] != b["denom"]).float().mean()) < 2e-3
        assert float((a["max_radii2D"] != b["max_radii2D"]).float().mean()) < 2e-3
        same = (a["denom"] == b["denom"]).squeeze(1)
        assert torch.allclose(a["xyz_gradient_accum"][same], b["xyz_gradient_accum"][same], rtol=1e-3, atol=1e-9)
    assert float(stats.denom.sum()) > 0
    assert opt.steps[2]["xyz"] == 2 and opt.steps[0]["xyz"] == len(frames)
