"""`-m gpu` tests of the SegmentedAdam sink (include/sgr_scene_step.h; optim.SegmentedAdam.sink,
FlatScene.compose(grad_sink=)): the Adam step applied inside the compose backward against the shipped two-step path of
the same tree -- the plain compose backward makes the gradients, SegmentedAdam.step applies them -- which the existing
tests pin to the numpy restatements.  The criterion is byte equality: after three iterations with changing learning
rates the seven flat leaves, both moment sets and all step counts are equal, and so are the poses and correction
gradients of every iteration.

Shapes: a chunk is 256 Gaussians -- a background of 257 (two chunks, odd: every later block starts at an odd element
offset, so the plain path's Adam kernel takes its scalar head and its float4 body), actors of 1, 255, 256 and 300, one
empty model; M in {1, 4, 16} (no features_rest, the runtime-M path, the <16> instantiation); fourier_dim 1 and 3; S = 0
and S = 3 in both semantic modes.  An actor with fourier_dim 3 and NO idft row (the `k > 0` zeros of the kernel) is
refused by the library's segment check in both paths before anything is launched: that case is pinned as a refusal."""
import copy

import numpy as np
import pytest
import torch

from street_gaussians_amd import densify, scene
from street_gaussians_amd._native import SgrError
from street_gaussians_amd.optim import ATTR, GROUPS, SegmentedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = (257, 1, 255, 256, 300, 0)  # background, actors (the last one empty)
LABELS = (0, 1, 2, 0, 5, 1)          # actor class columns; 5 is outside S = 3: no column, a zero gradient
FLIPPED = 4                          # the actor that carries a flip mask


def _segments(M, sem, fd, order, seed, sem_params=True, idft=True):
    """sem = (S, mode); with S == 0 the actors still carry their semantic column when `sem_params` (its gradient is the
    zeros of the `S <= 0` branch); a static model's semantic block is [n, S] wide, so the background then has none."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    S, mode = sem
    segs = []
    for k, n in enumerate(COUNTS):
        actor = k > 0
        C = fd if actor else 1
        semantic = None
        if sem_params and (actor or S):
            semantic = r(n, 1 if actor else S)
        segs.append(scene.Segment(
            xyz=r(n, 3), rotation=r(n, 4), scaling=r(n, 3) * 0.3, opacity=r(n, 1), features_dc=r(n, C, 3),
            features_rest=r(n, M - 1, 3), semantic=semantic, pose=r(7) if actor else None,
            idft=(r(C) if idft or C == 1 else None) if actor else None, class_label=LABELS[k], semantic_mode=mode))
    return [segs[i] for i in order]


class _Path:
    """One of the two paths: its own FlatScene, optimiser (random moments, uneven step counts) and correction leaf."""

    def __init__(self, M, sem, fd, order, frozen=(), seed=3, **kw):
        self.M, self.S = M, sem[0]
        self.flat = scene.FlatScene.from_segments(_segments(M, sem, fd, order, seed, **kw))
        for a in frozen:
            self.flat.tensors[a].requires_grad_(False)
        K = len(COUNTS)
        rng = np.random.default_rng(seed)
        self.opt = SegmentedAdam(self.flat, [{g: float(10 ** rng.uniform(-4, -2)) for g in GROUPS} for _ in range(K)])
        for a in self.opt.exp_avg:
            gen = torch.Generator().manual_seed(seed + len(a))
            self.opt.exp_avg[a].copy_(torch.randn(self.opt.exp_avg[a].shape, generator=gen).to(DEV) * 1e-2)
            self.opt.exp_avg_sq[a].copy_(torch.rand(self.opt.exp_avg_sq[a].shape, generator=gen).to(DEV) * 1e-4)
        for st in self.opt.steps:
            for g in GROUPS:
                st[g] = int(rng.integers(0, 50))
        self.corr = torch.tensor([0.98, 0.05, -0.1, 0.02, 0.3, -0.2, 0.1], device=DEV, requires_grad=True)
        self.order = list(order)

    def state(self):
        torch.cuda.synchronize()
        out = {f"p.{a}": t.detach().cpu().numpy().copy() for a, t in self.flat.tensors.items()}
        out.update({f"m.{a}": t.cpu().numpy().copy() for a, t in self.opt.exp_avg.items()})
        out.update({f"v.{a}": t.cpu().numpy().copy() for a, t in self.opt.exp_avg_sq.items()})
        return out

    def compose(self, frame, use_corr, sink=None, flips=True):
        masks = None
        if flips:
            masks = []
            for i in frame:
                n = self.flat.meta[i]["count"]
                on = self.order[i] == FLIPPED
                masks.append((torch.arange(n, device=DEV) % 3 == 1) if on else None)
        return self.flat.compose(self.M, self.S, flip_masks=masks, segments=frame, correction=self.corr if use_corr else None,
                                 grad_sink=sink)


def _bytes_equal(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _loss(outs, seed, ignore=()):
    """A fixed linear functional of the compose outputs (the weights depend only on the seed and the shapes)."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for name, o in zip(("means", "rot", "scale", "opac", "shs", "sem"), outs):
        w = torch.randn(o.shape, generator=g).to(DEV)
        if name not in ignore and o.numel():
            total = total + (o * w).sum()
    return total


def _frames(order):
    """Persistent indices of: every model; a frame that omits two actors (255 and 256); the actors only."""
    at = {k: i for i, k in enumerate(order)}
    return [None, [at[0], at[4], at[1], at[5]], [at[k] for k in (3, 1, 2, 5, 4)]]


def _iterate(path, use_sink, use_corr, ignore=(), iters=3):
    """Three iterations with changing learning rates.  Returns the per-iteration poses / correction gradients and checks
    that a model absent from a frame keeps its bytes."""
    grads = []
    K = len(COUNTS)
    for it, frame in enumerate(_frames(path.order)[:iters]):
        for s in range(K):  # the schedule: every model's xyz rate decays, one group of one model jumps
            path.opt.lrs[s]["xyz"] *= 0.7
        path.opt.lrs[it % K]["opacity"] *= 3.0
        segs = list(range(K)) if frame is None else frame
        before = path.state()
        steps0 = copy.deepcopy(path.opt.steps)
        sink = path.opt.sink(segs) if use_sink else None
        outs = path.compose(segs, use_corr, sink)
        _loss(outs, 100 + it, ignore).backward()
        path.opt.step(segs)
        for t in path.flat.tensors.values():
            if not use_sink:
                assert t.grad is not None or not t.requires_grad
            else:
                assert t.grad is None
            t.grad = None
        grads.append((path.flat.poses.grad.cpu().numpy().copy(),
                      path.corr.grad.cpu().numpy().copy() if use_corr else np.zeros(0, np.float32)))
        path.flat.poses.grad = None
        path.corr.grad = None
        after = path.state()
        for s in set(range(K)) - set(segs):  # an absent model: bytes and counts unchanged
            assert path.opt.steps[s] == steps0[s], (it, s)
            for g in GROUPS:
                off, cnt, _ = path.opt.layout[s][g]
                for kind in "pmv":
                    key = f"{kind}.{ATTR[g]}"
                    assert _bytes_equal(before[key].reshape(-1)[off:off + cnt], after[key].reshape(-1)[off:off + cnt]), (it, s, key)
        if use_sink:
            assert path.opt._sink is None and sink.consumed
    return grads


def _run_both(M, sem, fd, order, use_corr, frozen=(), ignore=(), **kw):
    plain, sunk = _Path(M, sem, fd, order, frozen, **kw), _Path(M, sem, fd, order, frozen, **kw)
    start = plain.state()
    g_plain = _iterate(plain, False, use_corr, ignore)
    g_sunk = _iterate(sunk, True, use_corr, ignore)
    a, b = plain.state(), sunk.state()
    for key in a:
        assert _bytes_equal(a[key], b[key]), key
    assert plain.opt.steps == sunk.opt.steps
    for it, ((pp, pc), (sp, sc_)) in enumerate(zip(g_plain, g_sunk)):
        assert _bytes_equal(pp, sp), f"poses gradient, iteration {it}"
        assert _bytes_equal(pc, sc_), f"correction gradient, iteration {it}"
    return start, a, plain


BG_FIRST = (0, 1, 2, 3, 4, 5)
ODD_FIRST = (1, 0, 4, 2, 5, 3)  # the one-Gaussian actor first: the background's blocks start at odd offsets too

CASES = [
    # M, (S, mode), fourier_dim, order, correction
    (16, (3, "logits"), 3, BG_FIRST, True),
    (16, (3, "probabilities"), 1, ODD_FIRST, False),
    (4, (3, "probabilities"), 3, ODD_FIRST, True),
    (4, (3, "logits"), 1, BG_FIRST, False),
    (4, (0, "logits"), 1, BG_FIRST, True),      # S = 0, actors with a semantic column: the zeros of the S <= 0 branch
    (1, (3, "logits"), 3, ODD_FIRST, True),
    (1, (3, "probabilities"), 1, BG_FIRST, False),
    (16, (0, "logits"), 3, ODD_FIRST, False),
]


@pytest.mark.parametrize("M,sem,fd,order,use_corr", CASES,
                         ids=[f"M{c[0]}-S{c[1][0]}{c[1][1][:4]}-fd{c[2]}-{'bg' if c[3] is BG_FIRST else 'odd'}first-corr{int(c[4])}"
                              for c in CASES])
def test_three_iterations_byte_equal_to_the_two_step_path(M, sem, fd, order, use_corr):
    start, end, plain = _run_both(M, sem, fd, order, use_corr)
    # the run did something: every group of the background moved
    lay = plain.opt.layout[order.index(0)]
    for g in GROUPS:
        off, cnt, _ = lay[g]
        if cnt:
            key = f"p.{ATTR[g]}"
            assert not _bytes_equal(start[key].reshape(-1)[off:off + cnt], end[key].reshape(-1)[off:off + cnt]), g


def test_scene_without_semantic_parameters():
    _run_both(4, (0, "logits"), 3, BG_FIRST, True, sem_params=False)


@pytest.mark.parametrize("frozen", ["opacity", "features_rest", "xyz"])
def test_frozen_leaf_stays_untouched_in_both_paths(frozen):
    start, end, plain = _run_both(4, (3, "probabilities"), 3, ODD_FIRST, True, frozen=(frozen,))
    for kind in "pmv":
        assert _bytes_equal(start[f"{kind}.{frozen}"], end[f"{kind}.{frozen}"])
    group = [g for g in GROUPS if ATTR[g] == frozen][0]
    assert all(st[group] == st0[group] for st, st0 in zip(plain.opt.steps, _Path(4, (3, "probabilities"), 3, ODD_FIRST).opt.steps))


def test_loss_that_ignores_shs_and_semantics_steps_them_with_zero():
    """None arrives upstream for shs and semantics: the plain backward writes zero gradients and the step moves the
    elements by their decaying moments; the sink does the same."""
    start, end, plain = _run_both(16, (3, "logits"), 3, BG_FIRST, True, ignore=("shs", "sem"))
    for a in ("features_dc", "features_rest", "semantic"):
        assert not _bytes_equal(start[f"p.{a}"], end[f"p.{a}"]), a
    assert plain.opt.steps[0]["f_rest"] > 0


def test_fourier_actor_without_idft_is_refused_alike():
    """fourier_dim 3 without an idft row (the kernels' `k > 0` zero case) does not pass the library's segment check: both
    paths refuse it before a launch, and the sink stays unconsumed and can be discarded."""
    for use_sink in (False, True):
        p = _Path(4, (3, "logits"), 3, BG_FIRST, idft=False)
        segs = list(range(len(COUNTS)))
        before = p.state()
        sink = p.opt.sink(segs) if use_sink else None
        with pytest.raises(SgrError, match="idft"):
            p.compose(segs, False, sink)
        if use_sink:
            assert not sink.consumed
            sink.discard()
        after = p.state()
        assert all(_bytes_equal(before[k], after[k]) for k in before)


# ---- consumption and errors ---------------------------------------------------------------------------------------
def test_second_backward_raises():
    p = _Path(4, (3, "logits"), 1, BG_FIRST)
    segs = list(range(len(COUNTS)))
    sink = p.opt.sink(segs)
    outs = p.compose(segs, True, sink)
    loss = _loss(outs, 1)
    loss.backward(retain_graph=True)
    once = p.state()
    with pytest.raises(RuntimeError, match="one backward per sink"):
        loss.backward()
    assert all(_bytes_equal(once[k], v) for k, v in p.state().items())
    p.opt.step(segs)
    # a second compose given the same (now disarmed) sink: refused in its backward as well
    outs = p.compose(segs, True, sink)
    with pytest.raises(RuntimeError, match="consumed"):
        _loss(outs, 2).backward()


def test_step_with_a_stray_grad_raises_and_changes_nothing():
    p = _Path(4, (3, "logits"), 1, BG_FIRST)
    segs = [0, 1, 4]
    sink = p.opt.sink(segs)
    _loss(p.compose(segs, False, sink), 1).backward()
    p.flat.tensors["scaling"].grad = torch.ones_like(p.flat.tensors["scaling"])
    before, steps0 = p.state(), copy.deepcopy(p.opt.steps)
    with pytest.raises(ValueError, match="mixed"):
        p.opt.step(segs)
    assert p.opt.steps == steps0 and all(_bytes_equal(before[k], v) for k, v in p.state().items())
    p.flat.tensors["scaling"].grad = None
    p.opt.step(segs)
    assert p.opt.steps[0]["xyz"] == steps0[0]["xyz"] + 1 and p.opt.steps[2]["xyz"] == steps0[2]["xyz"]


def test_armed_sink_whose_backward_never_ran_is_dropped_by_step():
    p = _Path(4, (3, "logits"), 1, BG_FIRST)
    segs = list(range(len(COUNTS)))
    sink = p.opt.sink(segs)
    with torch.no_grad():
        p.compose(segs, False, sink)
    before, steps0 = p.state(), copy.deepcopy(p.opt.steps)
    p.opt.step(segs)  # no gradient anywhere: as today, nothing to step
    assert not sink.armed and not sink.consumed and p.opt.steps == steps0
    assert all(_bytes_equal(before[k], v) for k, v in p.state().items())


def test_lazy_mode_refuses_the_sink():
    from street_gaussians_amd import _native
    p = _Path(4, (0, "logits"), 1, BG_FIRST)
    prev = _native.lib().sgr_set_lazy(1)
    try:
        with pytest.raises(RuntimeError, match="lazy"):
            p.opt.sink()
    finally:
        _native.lib().sgr_set_lazy(prev)


def test_no_host_synchronisation():
    p = _Path(16, (3, "probabilities"), 3, BG_FIRST)
    segs = [0, 1, 4, 5]
    outs = p.compose(segs, True, None)  # warm the allocator and the pinned staging buffers
    _loss(outs, 1).backward()
    p.opt.step(segs)
    for t in list(p.flat.tensors.values()) + [p.flat.poses, p.corr]:
        t.grad = None
    w = [torch.randn(o.shape, device=DEV) for o in p.compose(segs, True, None)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sink = p.opt.sink(segs)
        outs = p.compose(segs, True, sink)
        sum((o * x).sum() for o, x in zip(outs, w)).backward()
        p.opt.step(segs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sink.consumed and p.flat.xyz.grad is None and p.corr.grad is not None


# ---- one iteration through the real chain -------------------------------------------------------------------------
def _chain(use_sink):
    from diff_gaussian_rasterization import GaussianRasterizer
    from gpu_utils import settings
    from street_gaussians_amd import synthetic as syn
    M, S = 16, 3
    cam = syn.make_camera(64, 64, fx=60.0)
    sc = syn.make_scene(600, cam, S=0, seed=4)
    g = torch.Generator().manual_seed(8)
    r = lambda *s: torch.randn(*s, generator=g)
    segs = [scene.Segment(xyz=sc.means3D.cuda(), rotation=sc.rotations.cuda(), scaling=sc.scales.log().cuda(),
                          opacity=torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)).cuda(), features_dc=sc.shs[:, :1].cuda(),
                          features_rest=sc.shs[:, 1:].cuda(), semantic=r(600, S).cuda())]
    for k, n in enumerate((257, 120)):
        segs.append(scene.Segment(
            xyz=(r(n, 3) * 0.4).cuda(), rotation=r(n, 4).cuda(), scaling=torch.full((n, 3), -1.5).cuda(),
            opacity=r(n, 1).cuda(), features_dc=(r(n, 3, 3) * 0.3).cuda(), features_rest=(r(n, 15, 3) * 0.05).cuda(),
            semantic=r(n, 1).cuda(), pose=torch.tensor([0.9, 0.1 * k, -0.2, 0.3, 0.8 * (k - 0.5), -0.2, 6.0 + k]).cuda(),
            idft=torch.tensor([0.7, -0.4, 0.2]).cuda(), class_label=k % S))
    flat = scene.FlatScene.from_segments(segs)
    opt = SegmentedAdam(flat, [{gr: 1e-3 * (1 + s) for gr in GROUPS} for s in range(3)])
    stats = scene.FlatStats([m["count"] for m in flat.meta], DEV)
    frame = [0, 1, 2]
    sink = opt.sink(frame) if use_sink else None
    means3D, rot, scales, opac, shs, sem = flat.compose(M, S, segments=frame, grad_sink=sink)
    rast = GaussianRasterizer(settings(cam))
    rast.stats_sink = stats.sink(models=frame)
    m2d = torch.zeros(means3D.shape[0], 3, device=DEV, requires_grad=True)
    color, radii, depth, alpha, semo, acc = rast.forward_with_object_alpha(
        means3D, m2d, opac, shs=shs, scales=scales, rotations=rot, semantics=sem, split=600)
    wg = torch.Generator().manual_seed(5)
    w = lambda t: torch.randn(t.shape, generator=wg).to(DEV)
    loss = (color * w(color)).abs().sum() + (depth * w(depth)).sum() + (semo * w(semo)).sum() + ((acc - 0.5) ** 2).sum()
    loss.backward()
    opt.step(frame)
    for t in flat.tensors.values():
        t.grad = None
    torch.cuda.synchronize()
    assert float(acc.detach().max()) > 0.05 and float(stats.denom.sum()) > 0  # the actors are in view, Gaussians visible
    out = {f"p.{a}": t.detach().cpu().numpy() for a, t in flat.tensors.items()}
    out.update({f"m.{a}": t.cpu().numpy() for a, t in opt.exp_avg.items()})
    out.update({f"v.{a}": t.cpu().numpy() for a, t in opt.exp_avg_sq.items()})
    out.update(color=color.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(), alpha=alpha.detach().cpu().numpy(),
               sem=semo.detach().cpu().numpy(), acc=acc.detach().cpu().numpy(), radii=radii.cpu().numpy(),
               poses_grad=flat.poses.grad.cpu().numpy(), acc_stat=stats.xyz_gradient_accum.cpu().numpy(),
               denom=stats.denom.cpu().numpy(), max_radii=stats.max_radii2D.cpu().numpy())
    return out, opt.steps


def test_one_iteration_through_the_rasterizer_chain():
    plain, steps_p = _chain(False)
    sunk, steps_s = _chain(True)
    assert steps_p == steps_s
    for k in plain:
        assert _bytes_equal(plain[k], sunk[k]), k
    assert np.abs(plain["poses_grad"]).max() > 0


# ---- densification after sink-stepped iterations -------------------------------------------------------------------
def _densified(use_sink):
    from test_gpu_densify_scene import _Recorder, _actor_rule, _bkgd_rule
    p = _Path(16, (3, "logits"), 3, BG_FIRST)
    _iterate(p, use_sink, True, iters=2)
    N = p.flat.xyz.shape[0]
    g = torch.Generator().manual_seed(21)
    acc = (torch.rand(N, 2, generator=g) * 1e-3).to(DEV)
    den = torch.randint(0, 3, (N, 1), generator=g).float().to(DEV)
    rules = [_bkgd_rule()] + [_actor_rule() for _ in COUNTS[1:]]
    new_flat, new_moments, scalars, index = densify.densify_scene(
        p.flat, acc, den, rules, moments=(p.opt.exp_avg, p.opt.exp_avg_sq), normal_source=_Recorder(9))
    p.opt.rebuild_flat(new_flat, new_moments)
    p.flat = new_flat
    _iterate(p, use_sink, True, iters=1)  # and the rebuilt optimiser steps on, through the same path
    return p.state(), p.opt.steps, scalars


def test_densify_scene_and_rebuild_flat_after_sink_steps():
    a, steps_a, sc_a = _densified(False)
    b, steps_b, sc_b = _densified(True)
    assert steps_a == steps_b and sc_a == sc_b
    for k in a:
        assert _bytes_equal(a[k], b[k]), k
