"""`-m gpu` test of densify.densify_scene (include/sgr_densify_scene.h): density control of a whole FlatScene in one pass.

The yardstick is the per-model loop on the same GPU -- densify.densify_and_prune on every model's views with that
model's rule and its own block of the pre-drawn normals, FlatScene.from_segments, SegmentedAdam.rebuild -- and every
comparison is torch.equal: both paths run the same device functions (csrc/sgr_densify_rules.h) on the same inputs."""
import pytest
import torch

from street_gaussians_amd import densify, multiview, scene
from street_gaussians_amd.optim import ATTR, GROUPS, SegmentedAdam, segment_layout
from test_gpu_densify import KW, _setup

pytestmark = pytest.mark.gpu

M, S = 16, 3
FLAT = ("xyz", "rotation", "scaling", "opacity", "features_dc", "features_rest", "semantic")
SPHERE = dict(sphere_center=torch.tensor([0.5, -1.0, 0.3]), sphere_radius=2.5)   # of test_background_model_prune_rule
BOX = dict(box_min=torch.tensor([-1.2, -0.9, -1.5]), box_max=torch.tensor([1.1, 1.0, 1.4]))  # of test_actor_model_prune_rule
LRS = {g: 1e-3 * (i + 1) for i, g in enumerate(GROUPS)}


def _bkgd_rule(prune_big=True, **kw):
    return dict(KW, prune_big=prune_big, variant="bkgd", grad_column=1, **SPHERE, **kw)


def _actor_rule(prune_big=True, **kw):
    return dict(KW, prune_big=prune_big, variant="actor", **BOX, **kw)


def _model(n, fourier_dim, sem_width, seed, actor, sh=M):
    """One model with `_setup`'s inputs (denom has zeros: 0/0 -> NaN -> 0 and x/0 -> inf): (Segment fields, moments of its
    seven groups, xyz_gradient_accum, denom)."""
    p, states, accum, denom, _ = _setup(n, fourier_dim, sh, sem_width, seed)
    if actor:
        p["xyz"] *= 0.3  # most of the actor inside its tracking box
    else:
        p["scaling"][::7] += 3.0  # big points, near and far from the sphere
    seg = dict(xyz=p["xyz"], rotation=p["rotation"], scaling=p["scaling"], opacity=p["opacity"], features_dc=p["f_dc"],
               features_rest=p["f_rest"], semantic=p["semantic"] if sem_width else None)
    if actor:
        seg.update(pose=torch.tensor([1.0, 0.0, 0.0, 0.0, 0.5 * seed, 0.0, 8.0]), idft=torch.ones(fourier_dim) / fourier_dim,
                   class_label=seed % S)
    return seg, states, accum, denom


class _Scene:
    """A FlatScene on the GPU with its statistics and an optimiser whose moments are random."""

    def __init__(self, models):
        dev = "cuda"
        self.flat = scene.FlatScene.from_segments([scene.Segment(**{k: (v.to(dev) if torch.is_tensor(v) else v)
                                                                    for k, v in seg.items()}) for seg, _, _, _ in models])
        self.acc = torch.cat([a for _, _, a, _ in models]).to(dev)
        self.den = torch.cat([d for _, _, _, d in models]).to(dev)
        self.states = [st for _, st, _, _ in models]

    def optimiser(self, flat=None):
        opt = SegmentedAdam(flat or self.flat, [dict(LRS, xyz=LRS["xyz"] * (i + 1)) for i in range(len(self.states))])
        for i, st in enumerate(self.states):
            opt.steps[i] = {g: 3 + i for g in GROUPS}
            for g, (m, v) in opt.state_views(i).items():
                m.copy_(st[g][0].reshape(m.shape))
                v.copy_(st[g][1].reshape(v.shape))
        return opt


class _Recorder:
    """A normal source that draws from a seeded generator and keeps what it handed out."""

    def __init__(self, seed):
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.calls, self.blocks = [], []

    def __call__(self, rows, device, cols=3):
        t = torch.randn(int(rows), cols, generator=self.g, device=device)
        self.calls.append((int(rows), cols))
        self.blocks.append(t)
        return t


def _loop(sc, opt, rules, normal_source):
    """Today's loop (INTEGRATION section 6 per model).  Returns the new flat scene (opt rebuilt onto it), the per-model
    scalars, the kinds and flat source rows of the result, and per model which normal requests it made."""
    flat = sc.flat
    views, segs, states, scalars, kinds, srcs, asked = flat.views(), [], [], [], [], [], []
    row = 0
    n_calls = lambda: len(normal_source.calls) if isinstance(normal_source, _Recorder) else 0
    for i, m in enumerate(flat.meta):
        n = m["count"]
        before = n_calls()
        new, new_states, scal, index = densify.densify_and_prune(
            {g: views[i][a].detach() for g, a in ATTR.items()}, sc.acc[row:row + n], sc.den[row:row + n],
            states=opt.state_views(i), normal_source=normal_source, **rules[i])
        asked.append(n_calls() - before)
        segs.append(scene.Segment(new["xyz"], new["rotation"], new["scaling"], new["opacity"], new["f_dc"], new["f_rest"],
                                  semantic=new["semantic"] if m["sem_width"] else None, pose=views[i].get("pose"),
                                  idft=m["idft"], class_label=m["class_label"], semantic_mode=m["semantic_mode"]))
        states.append(new_states)
        scalars.append(scal)
        kinds.append(index["kind"])
        srcs.append(index["src"] + row)
        row += n
    new_flat = scene.FlatScene.from_segments(segs)
    opt.rebuild(new_flat, states)
    return new_flat, scalars, torch.cat(kinds), torch.cat(srcs), asked


def _split_blocks(rec, rules, asked):
    """The recorded blocks as the scene's two tensors: per model its split block (if it asked for one), then its box block
    (the actor rule with prune_big always asks)."""
    split, box, it = [], [], iter(rec.blocks)
    for rule, n in zip(rules, asked):
        has_box = rule.get("variant") == "actor" and rule["prune_big"]
        assert n in ((1, 2) if has_box else (0, 1))
        if n - int(has_box):
            split.append(next(it))
        if has_box:
            box.append(next(it))
    dev = "cuda"
    return (torch.cat(split) if split else torch.zeros(0, 3, device=dev),
            torch.cat(box).view(-1, 2, 3) if box else torch.zeros(0, 2, 3, device=dev))


def _assert_same(got, want_flat, want_opt, want_scalars, want_kind, want_src):
    new_flat, new_moments, scalars, index = got
    assert index["counts"] == [m["count"] for m in want_flat.meta] == [m["count"] for m in new_flat.meta]
    assert scalars == want_scalars
    for a in FLAT:
        assert new_flat.tensors[a].shape == want_flat.tensors[a].shape, a
        assert torch.equal(new_flat.tensors[a], want_flat.tensors[a]), a
        assert torch.equal(new_moments[0][a], want_opt.exp_avg[a]), a
        assert torch.equal(new_moments[1][a], want_opt.exp_avg_sq[a]), a
        assert new_flat.tensors[a].requires_grad
    assert torch.equal(index["kind"], want_kind)
    assert torch.equal(index["src"], want_src)


def _run_both(models, rules, seed=5):
    """The loop with a recording source, then densify_scene with the recorded normals as its two tensors."""
    sc = _Scene(models)
    rec = _Recorder(seed)
    opt_loop = sc.optimiser()
    want_flat, want_scalars, want_kind, want_src, asked = _loop(sc, opt_loop, rules, rec)
    normals, box_normals = _split_blocks(rec, rules, asked)
    opt = sc.optimiser()
    got = densify.densify_scene(sc.flat, sc.acc, sc.den, rules, moments=(opt.exp_avg, opt.exp_avg_sq), normals=normals,
                                box_normals=box_normals)
    _assert_same(got, want_flat, opt_loop, want_scalars, want_kind, want_src)
    assert got[0].poses is sc.flat.poses
    return sc, opt, got, (want_flat, opt_loop, want_scalars)


def _mixed_models():
    """Background of 2500 rows (S = 3), actors of 0, 1, 255, 257 and 700 rows (fourier_dim 5, semantic width 1, the
    257-row one without semantics): counts on both sides of the 256-row workgroups, the 128-row gather blocks and -- the
    background and the cumulated rows -- the 2048-element scan blocks."""
    models = [_model(2500, 1, S, 101, actor=False)]
    for i, (n, sw) in enumerate([(0, 1), (1, 1), (255, 1), (257, 0), (700, 1)]):
        models.append(_model(n, 5, sw, 110 + i, actor=True))
    return models


@pytest.mark.parametrize("prune_big", [True, False])
def test_mixed_scene_at_block_boundaries(prune_big):
    models = _mixed_models()
    rules = [_bkgd_rule(prune_big)] + [_actor_rule(prune_big) for _ in models[1:]]
    sc, opt, (new_flat, _, scalars, index), _ = _run_both(models, rules)
    kinds = index["kind"]
    assert all(int((kinds == k).sum()) > 0 for k in (0, 1, 2))  # keep, clone, split child
    assert scalars[0]["points_below_min_opacity"] > 0
    assert all(s["points_clone"] > 0 and s["points_split"] > 0 and s["points_pruned"] > 0 for s in (scalars[0], scalars[5]))
    if prune_big:
        assert scalars[0]["points_big_ws"] > 0
        # outside the box: the 700-row actor loses more points to its own box than to one nothing can leave (same normals)
        n = models[5][0]["xyz"].shape[0]
        views, row = sc.flat.views()[5], sum(m["count"] for m in sc.flat.meta[:5])
        rec = _Recorder(77)
        kw = dict(states=None, normal_source=rec)
        args = ({g: views[a].detach() for g, a in ATTR.items()}, sc.acc[row:row + n], sc.den[row:row + n])
        tight = densify.densify_and_prune(*args, **kw, **rules[5])[2]["points_pruned"]
        rec2 = _Recorder(77)
        wide = dict(rules[5], box_min=torch.full((3,), -1e9), box_max=torch.full((3,), 1e9))
        loose = densify.densify_and_prune(*args, states=None, normal_source=rec2, **wide)[2]["points_pruned"]
        assert tight > loose > 0


def test_degenerate_results():
    # model 1: every row pruned; model 2: nothing cloned, split or pruned; model 3 behind them is still right
    seg, st, acc, den = _model(130, 5, 1, 203, actor=True)
    still = (seg, st, acc, torch.ones_like(den))  # finite gradients: none reaches max_grad = 1e30
    models = [_model(300, 1, S, 201, actor=False), _model(200, 5, 1, 202, actor=True), still, _model(500, 5, 1, 204, actor=True)]
    rules = [_bkgd_rule(), _actor_rule(min_opacity=2.0), _actor_rule(False, max_grad=1e30, min_opacity=-1.0), _actor_rule()]
    sc, opt, (new_flat, new_moments, scalars, index), _ = _run_both(models, rules)
    assert index["counts"][1] == 0 and scalars[1]["points_pruned"] > 0
    assert index["counts"][2] == 130 and scalars[2] == dict(points_total=130, points_clone=0, points_split=0, points_pruned=0)
    old, new = sc.flat.views()[2], new_flat.views()[2]
    for a in FLAT:
        assert torch.equal(new[a], old[a].detach()), a
    lay_old, lay_new = opt.layout[2], segment_layout(new_flat.meta, new_flat.features_rest.shape[1])[2]
    for g in GROUPS:  # its moments are kept
        (o0, c0, _), (o1, c1, _) = lay_old[g], lay_new[g]
        assert c0 == c1
        assert torch.equal(new_moments[0][ATTR[g]].reshape(-1)[o1:o1 + c1], opt.exp_avg[ATTR[g]].reshape(-1)[o0:o0 + c0])
    # a scene of one model is the per-model call
    _run_both([_model(1500, 1, S, 205, actor=False)], [_bkgd_rule()])
    _run_both([_model(900, 5, 1, 206, actor=True)], [_actor_rule()])
    _run_both([_model(900, 1, 0, 207, actor=False, sh=4)], [dict(KW, prune_big=True)])  # the base rule


def test_different_thresholds_per_segment():
    """Two actors with identical tensors and different thresholds: each equals ITS per-model call, so they differ."""
    twin = _model(600, 5, 1, 301, actor=True)
    models = [_model(400, 1, S, 300, actor=False), twin, twin]
    rules = [_bkgd_rule(), _actor_rule(), _actor_rule(extent=1.0, max_grad=0.0008)]
    _, _, (new_flat, _, scalars, index), _ = _run_both(models, rules)
    assert scalars[1] != scalars[2] and index["counts"][1] != index["counts"][2]


def test_stateful_normal_source():
    models = _mixed_models()
    rules = [_bkgd_rule()] + [_actor_rule() for _ in models[1:]]
    sc = _Scene(models)
    rec_loop, rec_scene = _Recorder(9), _Recorder(9)
    _loop(sc, sc.optimiser(), rules, rec_loop)
    densify.densify_scene(sc.flat, sc.acc, sc.den, rules, normal_source=rec_scene)
    assert rec_scene.calls == rec_loop.calls and len(rec_loop.calls) > len(models)
    assert (0, 3) in rec_loop.calls  # the empty actor's box block is asked for as well
    # the library's replicated source: consumed call by call, so the results are equal
    opt_loop = sc.optimiser()
    want_flat, want_scalars, want_kind, want_src, _ = _loop(sc, opt_loop, rules,
                                                             multiview.ReplicatedNormals(seed=4, mode="seeded"))
    opt = sc.optimiser()
    got = densify.densify_scene(sc.flat, sc.acc, sc.den, rules, moments=(opt.exp_avg, opt.exp_avg_sq),
                                normal_source=multiview.ReplicatedNormals(seed=4, mode="seeded"))
    _assert_same(got, want_flat, opt_loop, want_scalars, want_kind, want_src)


def test_round_trip_into_training_state():
    models = [_model(2500, 1, S, 401, actor=False), _model(255, 5, 1, 402, actor=True), _model(700, 5, 1, 403, actor=True)]
    rules = [_bkgd_rule(), _actor_rule(), _actor_rule()]
    sc, opt, (new_flat, new_moments, _, index), (want_flat, opt_loop, _) = _run_both(models, rules)
    opt.rebuild_flat(new_flat, new_moments)
    assert opt.exp_avg["xyz"] is new_moments[0]["xyz"] and opt.flat is new_flat  # adopted, not copied
    assert opt.steps == opt_loop.steps and opt.lrs == opt_loop.lrs
    g = torch.Generator(device="cuda").manual_seed(1)
    for a in FLAT:
        grad = torch.randn(new_flat.tensors[a].shape, generator=g, device="cuda")
        new_flat.tensors[a].grad, want_flat.tensors[a].grad = grad, grad.clone()
    opt.step()
    opt_loop.step()
    for a in FLAT:
        assert torch.equal(new_flat.tensors[a], want_flat.tensors[a]), a
        assert torch.equal(opt.exp_avg_sq[a], opt_loop.exp_avg_sq[a]), a
    stats = scene.FlatStats(index["counts"], "cuda")
    out = new_flat.compose(M, S)
    assert out[0].shape[0] == sum(index["counts"]) == stats.denom.shape[0] and out[5].shape == (sum(index["counts"]), S)


def test_past_the_block_caps():
    """600 000 background rows + 3 actors: more than 2048 workgroups of 256 rows, so the prune kernel's grid-stride tail
    runs (its grid is capped at 2048 workgroups; the per-model clone count at 1024)."""
    models = [_model(600000, 1, 1, 501, actor=False, sh=4)] + [_model(n, 2, 1, 502 + i, actor=True, sh=4)
                                                                for i, n in enumerate((3000, 257, 4000))]
    rules = [_bkgd_rule()] + [_actor_rule() for _ in range(3)]
    _, _, (_, _, scalars, index), _ = _run_both(models, rules)
    n_cand = sum(s["points_total"] + s["points_clone"] + s["points_split"] for s in scalars)
    assert n_cand > 2048 * 256 and all(s["points_pruned"] > 0 for s in scalars)
