"""The fused per-segment Adam step (street_gaussians_amd/optim.py, include/sgr_optim.h) on the GPU: bitwise against the
float32 restatement of its declared arithmetic (torch_ref_optim.py), against one torch.optim.Adam(eps=1e-15) per model
over 50 steps with schedules, lr = 0 and absent models, untouched absent chunks, densification, reproducibility, no
host synchronisation and a non-default stream; and past its loop bounds: more spans than the grid has workgroups, as many
records as the table takes and one more, chunks that end on a span, every head length of the float4 path."""
import copy
import math

import numpy as np
import pytest
import torch

import torch_ref_optim as tr
from street_gaussians_amd import densify, optim
from street_gaussians_amd.optim import ATTR, GROUPS, SegmentedAdam
from street_gaussians_amd.scene import FlatScene, Segment

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# background (SH3, 19 classes) + actors: odd counts (unaligned blocks), fourier_dim > 1, sem_width 0, several spans
SPECS = [(10_001, 1, 19, False), (7, 5, 1, True), (4_099, 1, 1, True), (13, 3, 0, True), (1, 1, 1, True),
         (2_049, 5, 1, True)]


def _segments(specs, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    out = []
    for n, fd, sw, actor in specs:
        out.append(Segment(r(n, 3), r(n, 4), r(n, 3), r(n, 1), r(n, fd, 3), r(n, 15, 3),
                           semantic=r(n, sw) if sw else None, pose=r(7) if actor else None,
                           idft=r(fd) if actor else None))
    return out


def _flat(specs=SPECS, seed=0):
    return FlatScene.from_segments(_segments(specs, seed))


def _lrs(n, seed=0):
    rng = np.random.default_rng(seed)
    return [{g: float(10 ** rng.uniform(-5, -1)) for g in GROUPS} for _ in range(n)]


def _wide_grads(shape, seed, specials=True):
    """Gradients from 1e-30 to 1e4 in magnitude (subnormal g*g included), zeros, and NaN / inf at a few places."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(shape, generator=g) * 34 - 30)
    t = mag * torch.randn(shape, generator=g).sign()
    flat = t.view(-1)
    k = flat.numel()
    if specials and k > 40:
        idx = torch.randperm(k, generator=g)
        flat[idx[: k // 10]] = 0.0
        flat[idx[k // 10: k // 10 + 3]] = float("nan")
        flat[idx[k // 10 + 3: k // 10 + 5]] = float("inf")
        flat[idx[k // 10 + 5: k // 10 + 7]] = -float("inf")
    return t.to(DEV)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def _random_state(opt, seed):
    """Random moments (zeros where the gradient will be zero), random step counts."""
    rng = np.random.default_rng(seed)
    for a in opt.exp_avg:
        gen = torch.Generator().manual_seed(seed + len(a))
        opt.exp_avg[a].copy_(torch.randn(opt.exp_avg[a].shape, generator=gen).to(DEV) * 1e-2)
        opt.exp_avg_sq[a].copy_(torch.rand(opt.exp_avg_sq[a].shape, generator=gen).to(DEV) * 1e-4)
    for st in opt.steps:
        for g in GROUPS:
            st[g] = int(rng.integers(0, 200))


@pytest.mark.parametrize("shift_grads", [False, True], ids=["aligned", "grad-shifted"])
def test_one_step_bitwise_against_restatement(shift_grads):
    flat = _flat(seed=1)
    opt = SegmentedAdam(flat, _lrs(len(SPECS), 1))
    _random_state(opt, 3)
    for i, a in enumerate(ATTR[g] for g in GROUPS):
        leaf = flat.tensors[a]
        gr = _wide_grads(leaf.shape, 10 + i)
        if shift_grads:   # the gradient 4 bytes off the parameter's alignment: every chunk takes the scalar path
            buf = torch.empty(gr.numel() + 1, device=DEV)
            buf[1:].copy_(gr.reshape(-1))
            gr = buf[1:].view(leaf.shape)
        z = gr.reshape(-1) == 0                                # zero gradient with zero moments: 0 / eps
        opt.exp_avg[a].view(-1)[z] = 0.0
        opt.exp_avg_sq[a].view(-1)[z] = 0.0
        leaf.grad = gr
    before = {k: (flat.tensors[k].detach().cpu().numpy().copy(), opt.exp_avg[k].cpu().numpy().copy(),
                  opt.exp_avg_sq[k].cpu().numpy().copy(), flat.tensors[k].grad.cpu().numpy().copy()) for k in flat.tensors}
    steps0 = copy.deepcopy(opt.steps)
    opt.step()
    torch.cuda.synchronize()
    for s, lay in enumerate(opt.layout):
        for g in GROUPS:
            off, cnt, _ = lay[g]
            a = ATTR[g]
            assert opt.steps[s][g] == steps0[s][g] + 1
            if not cnt:
                continue
            sl = slice(off, off + cnt)
            p0, m0, v0, g0 = (x.reshape(-1)[sl] for x in before[a])
            p1, m1, v1 = tr.adam_step(p0, g0, m0, v0, opt.lrs[s][g], opt.steps[s][g])
            got = [t.detach().reshape(-1)[sl].cpu().numpy() for t in (flat.tensors[a], opt.exp_avg[a], opt.exp_avg_sq[a])]
            for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), got, (p1, m1, v1)):
                assert _bits_equal(x, y), (s, g, name)
    # the special values were there and propagated
    assert np.isnan(flat.xyz.detach().cpu().numpy()).any()


def _expon_lr(lr_init, lr_final, max_steps):
    """get_expon_lr_func's log-linear schedule (lr_delay_steps = 0)."""
    def f(step):
        t = np.clip(step / max_steps, 0, 1)
        return float(np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))
    return f


def _torch_models(flat, lrs):
    models = []
    for s, v in enumerate(flat.views()):
        ps = {g: torch.nn.Parameter(v[ATTR[g]].detach().clone()) for g in GROUPS}
        opt = torch.optim.Adam([{"params": [ps[g]], "lr": lrs[s][g], "name": g} for g in GROUPS], lr=0.0, eps=1e-15)
        models.append((ps, opt))
    return models


def _set_flat_grads(flat, layout, model_grads, present, seed, none=()):
    """Flat gradients whose blocks of the present segments hold the models' gradients; garbage elsewhere."""
    gen = torch.Generator().manual_seed(seed)
    for g in GROUPS:
        a = ATTR[g]
        if g in none:
            flat.tensors[a].grad = None
            continue
        G = (torch.randn(flat.tensors[a].shape, generator=gen) * 1e3).to(DEV)
        for s in present:
            off, cnt, _ = layout[s][g]
            G.view(-1)[off:off + cnt] = model_grads[s][g].reshape(-1)
        flat.tensors[a].grad = G


def _close(got, ref, lr, K, what):
    scale = 2.0 ** -23 * float(ref.abs().max()) + 2.0 ** -20 * lr
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    assert err <= K * scale, f"{what}: max error {err:.3e} > {K} x {scale:.3e}"
    return err == 0.0


def _compare(opt, flat, models, K, bitwise):
    views = flat.views()
    for s, (ps, topt) in enumerate(models):
        sv = opt.state_views(s)
        for g in GROUPS:
            p = ps[g]
            st = topt.state.get(p)
            assert opt.steps[s][g] == (int(st["step"]) if st else 0), (s, g)
            lr = opt.lrs[s][g]
            bitwise.append(_close(views[s][ATTR[g]].detach(), p.detach(), lr, K, f"seg {s} {g} p"))
            if st:
                bitwise.append(_close(sv[g][0], st["exp_avg"], 0.0, K, f"seg {s} {g} exp_avg"))
                bitwise.append(_close(sv[g][1], st["exp_avg_sq"], 0.0, K, f"seg {s} {g} exp_avg_sq"))


def _run_steps(opt, flat, models, n_steps, seed, schedules):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    for it in range(n_steps):
        present = [0] + [s for s in range(1, len(models)) if rng.random() < 0.7]
        for s, f in enumerate(schedules):
            opt.lrs[s]["xyz"] = f(it)
            for pg in models[s][1].param_groups:
                if pg["name"] == "xyz":
                    pg["lr"] = f(it)
        mg = {s: {g: torch.randn_like(models[s][0][g]) * float(10 ** rng.uniform(-4, 1)) for g in GROUPS}
              for s in present}
        _set_flat_grads(flat, opt.layout, mg, present, seed * 1000 + it)
        opt.step(segments=present)
        for s, (ps, topt) in enumerate(models):
            for g in GROUPS:
                ps[g].grad = mg[s][g].clone() if s in present else None
            topt.step()
            topt.zero_grad(set_to_none=True)
        for t in flat.tensors.values():
            t.grad = None


def test_fifty_steps_against_torch_adam_per_model():
    specs = [(10_001, 1, 19, False)] + [(n, fd, 1, True) for n, fd in ((7, 5), (1_001, 1), (13, 3), (2_049, 5), (1, 1))]
    flat = _flat(specs, seed=2)
    lrs = _lrs(len(specs), 2)
    lrs[3]["opacity"] = 0.0                       # an lr = 0 group: moments and step still advance
    opt = SegmentedAdam(flat, lrs)
    models = _torch_models(flat, lrs)
    schedules = [_expon_lr(1.6e-4 * (s + 1), 1.6e-6, 50) for s in range(len(specs))]
    _run_steps(opt, flat, models, 50, seed=5, schedules=schedules)
    torch.cuda.synchronize()
    bitwise = []
    _compare(opt, flat, models, K=64, bitwise=bitwise)
    print(f"bitwise equal to torch.optim.Adam (foreach) in {sum(bitwise)} of {len(bitwise)} tensors")
    # lr = 0: the parameter did not move, its moments and step did
    assert torch.equal(flat.views()[3]["opacity"], models[3][0]["opacity"].detach())
    assert opt.steps[3]["opacity"] > 0
    assert min(min(st.values()) for st in opt.steps[1:]) < 50   # every actor missed some steps


def test_absent_segments_and_none_grads_are_untouched():
    flat = _flat(seed=4)
    opt = SegmentedAdam(flat, _lrs(len(SPECS), 4))
    _random_state(opt, 7)
    present = [0, 2, 5]
    mg = {s: {g: torch.randn(opt.layout[s][g][2], device=DEV) for g in GROUPS} for s in present}
    _set_flat_grads(flat, opt.layout, mg, present, 9, none=("rotation", "semantic"))
    snap = {a: (flat.tensors[a].detach().clone(), opt.exp_avg[a].clone(), opt.exp_avg_sq[a].clone()) for a in flat.tensors}
    steps0 = copy.deepcopy(opt.steps)
    opt.step(segments=present)
    torch.cuda.synchronize()
    for s, lay in enumerate(opt.layout):
        for g in GROUPS:
            off, cnt, _ = lay[g]
            a = ATTR[g]
            moved = s in present and g not in ("rotation", "semantic")
            assert opt.steps[s][g] == steps0[s][g] + int(moved), (s, g)
            now = (flat.tensors[a].detach(), opt.exp_avg[a], opt.exp_avg_sq[a])
            for x, y in zip(now, snap[a]):
                same = torch.equal(x.reshape(-1)[off:off + cnt].view(torch.int32), y.reshape(-1)[off:off + cnt].view(torch.int32))
                assert same != moved or cnt == 0, (s, g)


def _densify_all(params_per_model, states_per_model, seed):
    out = []
    for s, (params, states) in enumerate(zip(params_per_model, states_per_model)):
        n = params["xyz"].shape[0]
        gen = torch.Generator(device=DEV).manual_seed(seed + s)
        acc = torch.rand(n, 2, device=DEV, generator=gen) * 4e-4
        den = torch.ones(n, 1, device=DEV)
        ng = torch.Generator(device=DEV).manual_seed(seed + 100 + s)
        new, new_states, scalars, _ = densify.densify_and_prune(
            {g: params[g].detach() for g in GROUPS}, acc, den, states=states, max_grad=2e-4, min_opacity=0.3,
            extent=3.0, percent_dense=0.3, percent_big_ws=0.1, prune_big=False,
            normal_source=lambda rows, dev, cols=3: torch.randn(rows, cols, device=dev, generator=ng))
        out.append((new, new_states, scalars))
    return out


def test_densify_rebuild_then_step_matches_torch_path():
    specs = [(3_001, 1, 19, False), (101, 5, 1, True), (57, 1, 1, True)]
    flat = _flat(specs, seed=6)
    lrs = _lrs(len(specs), 6)
    opt = SegmentedAdam(flat, lrs)
    models = _torch_models(flat, lrs)
    flat_sched = [lambda it: 1e-3] * len(specs)
    _run_steps(opt, flat, models, 5, seed=8, schedules=flat_sched)
    torch.cuda.synchronize()

    views = flat.views()
    ours = _densify_all([{g: views[s][ATTR[g]] for g in GROUPS} for s in range(len(specs))],
                        [opt.state_views(s) for s in range(len(specs))], seed=40)
    theirs = _densify_all([ps for ps, _ in models],
                          [{g: (topt.state[ps[g]]["exp_avg"], topt.state[ps[g]]["exp_avg_sq"]) for g in GROUPS}
                           for ps, topt in models], seed=40)
    segs = []
    for s, (new, _, sc) in enumerate(ours):
        assert sc == theirs[s][2]
        assert sc["points_clone"] + sc["points_split"] + sc["points_pruned"] > 0
        old = flat.views()[s]
        segs.append(Segment(new["xyz"], new["rotation"], new["scaling"], new["opacity"], new["f_dc"], new["f_rest"],
                            semantic=new["semantic"], pose=old.get("pose"), idft=flat.meta[s]["idft"]))
    new_flat = FlatScene.from_segments(segs)
    opt.rebuild(new_flat, [st for _, st, _ in ours])
    # the torch path's state surgery, as INTEGRATION section 6 does it
    for (ps, topt), (new, new_states, _) in zip(models, theirs):
        for pg in topt.param_groups:
            g = pg["name"]
            old = pg["params"][0]
            st = topt.state.pop(old)
            st["exp_avg"], st["exp_avg_sq"] = new_states[g]
            pg["params"][0] = ps[g] = torch.nn.Parameter(new[g].requires_grad_(True))
            topt.state[ps[g]] = st
    _run_steps(opt, new_flat, models, 5, seed=9, schedules=flat_sched)
    torch.cuda.synchronize()
    _compare(opt, new_flat, models, K=64, bitwise=[])


def test_bit_reproducible_no_sync_and_non_default_stream():
    results = []
    for rep in range(10):
        flat = _flat(seed=11)
        opt = SegmentedAdam(flat, _lrs(len(SPECS), 11))
        for i, a in enumerate(ATTR[g] for g in GROUPS):
            flat.tensors[a].grad = _wide_grads(flat.tensors[a].shape, 50 + i, specials=False)
        torch.cuda.synchronize()
        if rep == 0:
            torch.cuda.set_sync_debug_mode("error")
            try:
                opt.step(segments=[0, 1, 3, 5])
                opt.step()
            finally:
                torch.cuda.set_sync_debug_mode(0)
        elif rep == 1:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                opt.step(segments=[0, 1, 3, 5])
                opt.step()
            torch.cuda.current_stream().wait_stream(s)
        else:
            opt.step(segments=[0, 1, 3, 5])
            opt.step()
        torch.cuda.synchronize()
        results.append(torch.cat([t.detach().reshape(-1) for t in flat.tensors.values()] +
                                 [opt.exp_avg[a].reshape(-1) for a in flat.tensors] +
                                 [opt.exp_avg_sq[a].reshape(-1) for a in flat.tensors]).view(torch.int32).cpu())
    for r in results[1:]:
        assert torch.equal(r, results[0])


def test_state_dict_round_trip_on_device():
    flat = _flat(seed=12)
    opt = SegmentedAdam(flat, _lrs(len(SPECS), 12))
    _random_state(opt, 13)
    for g in GROUPS:     # a group that has taken no step has no state in torch: only stepped groups carry moments
        opt.steps[2][g] = max(opt.steps[2][g], 1)
    opt.steps[2]["opacity"] = 0
    opt.state_views(2)["opacity"][0].zero_()
    opt.state_views(2)["opacity"][1].zero_()
    sd = opt.model_state_dict(2)
    assert 3 not in sd["state"] and len(sd["state"]) == 6
    p = {g: torch.nn.Parameter(torch.zeros(opt.layout[2][g][2], device=DEV)) for g in GROUPS}
    topt = torch.optim.Adam([{"params": [p[g]], "lr": 0.0, "name": g} for g in GROUPS], lr=0.0, eps=1e-15)
    topt.load_state_dict(copy.deepcopy(sd))
    other = SegmentedAdam(_flat(seed=12), _lrs(len(SPECS), 99))
    other.load_model_state_dict(2, topt.state_dict())
    assert other.lrs[2] == opt.lrs[2] and other.steps[2] == opt.steps[2]
    for g in GROUPS:
        for x, y in zip(other.state_views(2)[g], opt.state_views(2)[g]):
            assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# past the loop bounds: the grid-stride walk of the spans, the LDS copy and the search of the record table, the refusal
# of a table that is too long, and the edges of a span.  Every value check is bitwise against the restatement.
def _lib():
    from street_gaussians_amd import _native
    return _native.lib()


def _set_wide_grads(flat, opt, seed):
    """_wide_grads on every leaf; zero moments where the gradient is zero (0 / eps, as the first test has it)."""
    for i, a in enumerate(ATTR[g] for g in GROUPS):
        leaf = flat.tensors[a]
        gr = _wide_grads(leaf.shape, seed + i)
        z = gr.reshape(-1) == 0
        opt.exp_avg[a].view(-1)[z] = 0.0
        opt.exp_avg_sq[a].view(-1)[z] = 0.0
        leaf.grad = gr


def _snapshot(flat, opt):
    """{attr: (p, exp_avg, exp_avg_sq, grad)} as flat host arrays."""
    h = lambda t: t.detach().reshape(-1).cpu().numpy().copy()
    return {a: (h(flat.tensors[a]), h(opt.exp_avg[a]), h(opt.exp_avg_sq[a]), h(flat.tensors[a].grad)) for a in flat.tensors}


def _plan_only(opt, flat, segments=None):
    """The record table and span total the next step will use, planned on a copy of the step counts."""
    grads = {g: flat.tensors[ATTR[g]].grad.data_ptr() for g in GROUPS if flat.tensors[ATTR[g]].grad is not None}
    return optim.plan_step(opt.layout, copy.deepcopy(opt.steps), opt.lrs, segments, grads, opt.betas, opt.eps, opt._span)


def _assert_step_bitwise(flat, opt, before, steps0, present):
    """After one step of the segments ``present``: every element of every flat p, exp_avg and exp_avg_sq is the
    restatement's where a chunk was stepped and its bytes from before the step everywhere else (absent segments, and
    whatever of a flat tensor no chunk covers)."""
    want = {a: [x.copy() for x in before[a][:3]] for a in before}
    for s, lay in enumerate(opt.layout):
        for g in GROUPS:
            off, cnt, _ = lay[g]
            assert opt.steps[s][g] == steps0[s][g] + int(s in present), (s, g)
            if not cnt or s not in present:
                continue
            sl = slice(off, off + cnt)
            p0, m0, v0, g0 = (x[sl] for x in before[ATTR[g]])
            for dst, new in zip(want[ATTR[g]], tr.adam_step(p0, g0, m0, v0, opt.lrs[s][g], opt.steps[s][g])):
                dst[sl] = new
    for a in before:
        got = [t.detach().reshape(-1).cpu().numpy() for t in (flat.tensors[a], opt.exp_avg[a], opt.exp_avg_sq[a])]
        for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), got, want[a]):
            if not _bits_equal(x, y):
                bad = np.flatnonzero(~((x.view(np.int32) == y.view(np.int32)) | (np.isnan(x) & np.isnan(y))))
                raise AssertionError(f"{a} {name}: {bad.size} of {x.size} elements differ, the first at {bad[0]}")


def test_one_step_past_the_grid_cap():
    """A scene of more spans than the grid has workgroups: every workgroup walks two spans and some a third (the real
    size, 1 M Gaussians, makes about 14 trips).  The cap is the library's: were it raised, this fails instead of passing
    without reaching the loop."""
    cap = _lib().sgr_adam_max_blocks()
    specs = [(150_001, 1, 19, False), (7, 5, 1, True), (13, 3, 0, True), (1, 1, 1, True), (4_099, 1, 1, True)]
    flat = _flat(specs, seed=21)
    opt = SegmentedAdam(flat, _lrs(len(specs), 21))
    _random_state(opt, 22)
    _set_wide_grads(flat, opt, 30)
    rec, n_spans = _plan_only(opt, flat)
    assert cap > 0 and 2 * cap < n_spans < 3 * cap and n_spans % cap != 0, \
        f"{n_spans} spans no longer reach two full trips and a ragged third of a grid of {cap}"
    before, steps0 = _snapshot(flat, opt), copy.deepcopy(opt.steps)
    opt.step()
    torch.cuda.synchronize()
    _assert_step_bitwise(flat, opt, before, steps0, set(range(len(specs))))
    assert np.isnan(flat.features_rest.detach().cpu().numpy()).any()


def _actor_specs(n_records):
    """Actors of 1 to 7 points, fourier_dim 1, 3 or 5, that give exactly ``n_records`` records when all are stepped: 7 per
    actor, 6 for one without a semantic column."""
    n_actors = n_records // 7 + 1
    no_sem = 7 * n_actors - n_records                      # 1 to 7 of them, spread over the table
    stride = n_actors // no_sem
    return [(1 + i % 7, (1, 3, 1, 5)[i % 4], 0 if i % stride == 0 and i // stride < no_sem else 1, True)
            for i in range(n_actors)]


def _many_record_scene(n_records, seed):
    specs = _actor_specs(n_records)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    segs = [Segment(r(n, 3), r(n, 4), r(n, 3), r(n, 1), r(n, fd, 3), r(n, 15, 3), semantic=r(n, sw) if sw else None,
                    pose=r(7), idft=r(fd)) for n, fd, sw, _ in specs]
    flat = FlatScene.from_segments(segs)
    opt = SegmentedAdam(flat, _lrs(len(specs), seed))
    _random_state(opt, seed + 1)
    _set_wide_grads(flat, opt, seed + 2)
    return specs, flat, opt


@pytest.mark.parametrize("below", [1, 0], ids=["limit-1", "limit"])
def test_one_step_of_as_many_records_as_the_table_takes(below):
    """As many records as the table takes, and one less (4095 at a limit of 4096), of small actors, some with
    fourier_dim > 1, some without a semantic column: the copy of the span starts into LDS makes 16 trips and the search
    is 12 deep.  Then a subset of the segments, so that the records' chunk indices have gaps."""
    limit = _lib().sgr_adam_max_records()
    n_records = limit - below
    assert n_records > 256 * 2, "the table no longer reaches a second trip of the LDS copy"
    specs, flat, opt = _many_record_scene(n_records, seed=40 + below)
    assert {fd for _, fd, _, _ in specs} >= {1, 3, 5} and {sw for _, _, sw, _ in specs} == {0, 1}
    rec, n_spans = _plan_only(opt, flat)
    assert len(rec) == n_records and n_spans == n_records
    before, steps0 = _snapshot(flat, opt), copy.deepcopy(opt.steps)
    opt.step()
    torch.cuda.synchronize()
    _assert_step_bitwise(flat, opt, before, steps0, set(range(len(specs))))

    present = [s for s in range(len(specs)) if s % 3 != 1 and s % 11 != 0]
    rec, _ = _plan_only(opt, flat, present)
    assert len(rec) > 256 * 2 and (np.diff(rec["chunk"]) > 1).any()
    before, steps0 = _snapshot(flat, opt), copy.deepcopy(opt.steps)
    opt.step(segments=present)
    torch.cuda.synchronize()
    _assert_step_bitwise(flat, opt, before, steps0, set(present))


def test_a_step_of_too_many_records_is_refused_with_nothing_changed():
    """One record more than the table takes: an SgrError that names the limit, and the step counts, the parameters and
    the moments are what they were (the step counts used to advance before the native call refused the table)."""
    limit = _lib().sgr_adam_max_records()
    specs, flat, opt = _many_record_scene(limit + 1, seed=50)
    rec, _ = _plan_only(opt, flat)
    assert len(rec) == limit + 1
    before, steps0 = _snapshot(flat, opt), copy.deepcopy(opt.steps)
    with pytest.raises(optim.SgrError, match=str(limit)):
        opt.step()
    torch.cuda.synchronize()
    assert opt.steps == steps0
    _assert_step_bitwise(flat, opt, before, steps0, set())
    # a subset that fits still steps
    opt.step(segments=range(1, len(specs)))
    torch.cuda.synchronize()
    _assert_step_bitwise(flat, opt, before, steps0, set(range(1, len(specs))))


def test_span_edges_and_every_head_length():
    """Chunks that end exactly on a span (4096 points: opacity is one span, xyz three; 1024 points: rotation is one span),
    aligned and not, and the float4 path's head: every head length 0..3, a chunk shorter than its head, a chunk without
    a single float4.  The coverage is computed from the layout and the addresses, so it holds or fails with them."""
    span = _lib().sgr_adam_span_elems()
    specs = [(span, 1, 19, False), (span // 4, 1, 1, True), (5, 3, 1, True), (1, 1, 1, True), (1, 1, 0, True),
             (1, 5, 1, True), (7, 1, 1, True), (2, 1, 1, True), (span, 1, 1, True)]
    flat = _flat(specs, seed=60)
    opt = SegmentedAdam(flat, _lrs(len(specs), 60))
    _random_state(opt, 61)
    _set_wide_grads(flat, opt, 62)
    heads, shorter, no_vec, exact = set(), 0, 0, set()
    for lay in opt.layout:
        for g in GROUPS:
            off, cnt, _ = lay[g]
            if not cnt:
                continue
            a = ATTR[g]
            addr = [t.data_ptr() + 4 * off for t in (flat.tensors[a], flat.tensors[a].grad, opt.exp_avg[a], opt.exp_avg_sq[a])]
            if len({x & 15 for x in addr}) != 1:
                continue                                  # the scalar path
            h = ((16 - (addr[0] & 15)) & 15) >> 2
            heads.add(h)
            shorter += cnt < h
            last = cnt - (cnt - 1) // span * span         # elements of the chunk's last span
            no_vec += (max(last - h, 0) >> 2) == 0
            if cnt % span == 0:
                exact.add((cnt // span, h))
    assert heads == {0, 1, 2, 3}, heads
    assert shorter > 0 and no_vec > shorter
    assert {n for n, _ in exact} >= {1, 3} and {h for _, h in exact} > {0}, exact
    assert opt.layout[1]["rotation"][1] == span
    before, steps0 = _snapshot(flat, opt), copy.deepcopy(opt.steps)
    opt.step()
    torch.cuda.synchronize()
    _assert_step_bitwise(flat, opt, before, steps0, set(range(len(specs))))
