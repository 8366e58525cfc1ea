"""CPU tests of densify.densify_scene (include/sgr_densify_scene.h): every argument check answers before any HIP call
(a HIP call would answer SGR_E_HIP on a machine without a GPU), and the layout rule -- where a model's candidates, split
normals and box normals start, and in which order a normal source is asked -- stated in numpy against the host function
densify_scene uses."""
import ctypes as C

import numpy as np
import pytest
import torch

from street_gaussians_amd import _native, densify, scene
from street_gaussians_amd._native import SgrError

SGR_E_INVALID = 1  # include/sgr.h
KW = dict(max_grad=0.0004, min_opacity=0.05, extent=3.0, percent_dense=0.01, percent_big_ws=0.1, prune_big=True)
BKGD = dict(KW, variant="bkgd", sphere_center=[0.5, -1.0, 0.3], sphere_radius=2.5, grad_column=1)
ACTOR = dict(KW, variant="actor", box_min=[-1.2, -0.9, -1.5], box_max=[1.1, 1.0, 1.4])
META = [dict(count=5, fourier_dim=1, sem_width=3), dict(count=0, fourier_dim=5, sem_width=1),
        dict(count=7, fourier_dim=5, sem_width=0)]


def _flat(counts=(5, 0, 7)):
    z = torch.zeros
    segs = [scene.Segment(z(counts[0], 3), z(counts[0], 4), z(counts[0], 3), z(counts[0], 1), z(counts[0], 1, 3),
                          z(counts[0], 15, 3), semantic=z(counts[0], 3))]
    for n in counts[1:]:
        segs.append(scene.Segment(z(n, 3), z(n, 4), z(n, 3), z(n, 1), z(n, 5, 3), z(n, 15, 3), semantic=z(n, 1),
                                  pose=z(7), idft=z(5)))
    return scene.FlatScene.from_segments(segs)


@pytest.mark.parametrize("rules", [
    [BKGD, ACTOR],                                                  # one rule short
    [BKGD, ACTOR, dict(ACTOR, max_screen_size=20)],                 # unknown key
    [BKGD, ACTOR, {k: v for k, v in ACTOR.items() if k != "extent"}],  # missing key
    [BKGD, ACTOR, dict(ACTOR, variant="sky")],                      # unknown variant
    [dict(BKGD, sphere_radius=None), ACTOR, ACTOR],                 # the background rule without its sphere
    [BKGD, ACTOR, dict(ACTOR, box_max=None)],                       # the actor rule without its box
    [BKGD, ACTOR, dict(ACTOR, box_min=[0.0, 0.0])],                 # a box of two values
])
def test_malformed_rules_raise_value_error(rules):
    flat = _flat()
    N = flat.xyz.shape[0]
    with pytest.raises(ValueError):
        densify.densify_scene(flat, torch.zeros(N, 2), torch.zeros(N, 1), rules)


def test_cpu_tensors_raise_sgr_error():
    flat = _flat()
    N = flat.xyz.shape[0]
    with pytest.raises(SgrError, match="no CPU path"):
        densify.densify_scene(flat, torch.zeros(N, 2), torch.zeros(N, 1), [BKGD, ACTOR, ACTOR])
    with pytest.raises(ValueError, match="moments"):
        densify.densify_scene(flat, torch.zeros(N, 2), torch.zeros(N, 1), [BKGD, ACTOR, ACTOR], moments=({}, {}))


def test_normals_of_the_wrong_shape_raise_value_error():
    lay = densify.scene_layout(densify.scene_table(META, [BKGD, ACTOR, ACTOR]), 3, [[3, 1, 2, 2], [0, 0, 0, 0], [6, 2, 1, 1]])
    assert int(lay["normals_base"][-1]) == 6 and int(lay["box_base"][-1]) == 10
    ok_n, ok_b = torch.zeros(6, 3), torch.zeros(10, 2, 3)
    densify._scene_normals(lay, ok_n, ok_b, None, "cpu")
    with pytest.raises(ValueError, match="normals"):
        densify._scene_normals(lay, torch.zeros(5, 3), ok_b, None, "cpu")
    with pytest.raises(ValueError, match="box_normals"):
        densify._scene_normals(lay, ok_n, torch.zeros(10, 3, 2), None, "cpu")
    with pytest.raises(ValueError, match="normal_source"):
        densify._scene_normals(lay, None, ok_b, lambda rows, dev: torch.zeros(rows + 1, 3), "cpu")


def _table(rows):
    """rows: (start, count, rule) -> a host table with those starts (scene_table lays the blocks out itself)."""
    tab = densify.scene_table([dict(count=c, fourier_dim=1, sem_width=1) for _, c, _ in rows], [r for _, _, r in rows])
    for c, (start, _, _) in zip(tab, rows):
        c.start = start
    return tab


def _bad_tables():
    """(what the message must name, N, table)"""
    nan = float("nan")
    yield "overlap", 12, _table([(0, 8, BKGD), (6, 6, ACTOR)])
    yield "sorted", 12, _table([(6, 6, ACTOR), (0, 6, BKGD)])
    yield "gaps", 12, _table([(0, 5, BKGD), (6, 6, ACTOR)])
    yield "n_split", 12, _table([(0, 6, dict(BKGD, n_split=0)), (6, 6, dict(ACTOR, n_split=0))])
    yield "n_split", 12, _table([(0, 6, BKGD), (6, 6, dict(ACTOR, n_split=3))])
    yield "grad_column", 12, _table([(0, 6, dict(BKGD, grad_column=2)), (6, 6, ACTOR)])
    t = _table([(0, 6, BKGD), (6, 6, ACTOR)])
    t[0].sphere[3] = nan
    yield "sphere", 12, t
    t = _table([(0, 6, BKGD), (6, 6, ACTOR)])
    t[1].box[4] = nan
    yield "box", 12, t
    t = _table([(0, 6, BKGD), (6, 6, ACTOR)])
    t[1].variant = 7
    yield "variant", 12, t


@pytest.mark.parametrize("what,N,tab", list(_bad_tables()))
def test_every_entry_point_rejects_a_bad_table_before_any_hip_call(what, N, tab):
    """SGR_E_INVALID with the table's own message (the table is checked first: no pointer is looked at, so none is given)."""
    L = _native.lib()
    K = len(tab)
    tot, cnt, nc = (C.c_int64 * (4 * K))(), (C.c_int64 * (5 * K))(), (C.c_int64 * K)(1, 1)
    calls = [lambda: L.sgr_densify_scene_plan(N, K, tab, *[None] * 6, tot, None),
             lambda: L.sgr_densify_scene_map(N, K, tab, *[None] * 5, None),
             lambda: L.sgr_densify_scene_prune(N, K, tab, *[None] * 13, cnt, None),
             lambda: L.sgr_densify_scene_gather_ragged(K, tab, None, nc, None, 0, None, None, None, 0, None, None)]
    for call in calls:
        assert call() == -SGR_E_INVALID, what
        assert what in L.sgr_last_error().decode(), (what, L.sgr_last_error())


def test_segments_must_cover_all_rows():
    L = _native.lib()
    tab = _table([(0, 6, BKGD), (6, 6, ACTOR)])
    tot = (C.c_int64 * 8)()
    for N in (11, 13):
        assert L.sgr_densify_scene_plan(N, 2, tab, *[None] * 6, tot, None) == -SGR_E_INVALID
        assert b"cover [0, N)" in L.sgr_last_error()
        assert L.sgr_densify_scene_map(N, 2, tab, *[None] * 5, None) == -SGR_E_INVALID
        assert b"cover [0, N)" in L.sgr_last_error()


def test_missing_arrays_and_too_many_rows_are_invalid():
    L = _native.lib()
    tab = _table([(0, 6, BKGD), (6, 6, ACTOR)])
    dev = C.c_void_p(4096)
    tot, cnt = (C.c_int64 * 8)(), (C.c_int64 * 10)()
    assert L.sgr_densify_scene_plan(12, 2, tab, dev, dev, None, dev, dev, dev, tot, None) == -SGR_E_INVALID  # no denom
    assert L.sgr_densify_scene_plan(12, 0, tab, dev, dev, dev, dev, dev, dev, tot, None) == -SGR_E_INVALID   # no segments
    assert L.sgr_densify_scene_plan(12, 1025, tab, dev, dev, dev, dev, dev, dev, tot, None) == -SGR_E_INVALID
    # the actor rule with prune_big reads box_normals: NULL is refused
    args = [dev] * 13
    args[5] = None
    assert L.sgr_densify_scene_prune(12, 2, tab, *args, cnt, None) == -SGR_E_INVALID
    assert b"box_normals" in L.sgr_last_error()
    # 2^30 split points with two children each: 2^31 candidates
    big = (C.c_int64 * 8)(0, 0, 2 ** 30, 2 ** 30, 0, 0, 0, 0)
    lay = (C.c_int64 * 9)()
    assert L.sgr_densify_scene_layout(2, tab, big, lay) == -SGR_E_INVALID
    assert b"2^31" in L.sgr_last_error()
    big[3] = 2 ** 30 - 1
    assert L.sgr_densify_scene_layout(2, tab, big, lay) == 0


def _layout_numpy(totals, n_split, has_box):
    """The layout contract of include/sgr_densify_scene.h: a model's candidates are its kept originals, its clones and
    n_split children per split point with children; blocks follow each other in model order."""
    totals = np.asarray(totals, dtype=np.int64)
    n_cand = totals[:, 0] + totals[:, 1] + n_split * totals[:, 3]
    n_norm = n_split * totals[:, 2]
    ex = lambda v: np.concatenate([[0], np.cumsum(v)])
    requests = []
    for s in range(len(totals)):
        if n_norm[s]:
            requests.append((s, "split", int(n_norm[s])))
        if has_box[s]:
            requests.append((s, "box", int(2 * n_cand[s])))
    return ex(n_cand), ex(n_norm), ex(n_cand * np.asarray(has_box)), requests


@pytest.mark.parametrize("n_split", [2, 3])
def test_layout_rule_against_numpy(n_split):
    rules = [dict(BKGD, n_split=n_split), dict(ACTOR, n_split=n_split), dict(ACTOR, n_split=n_split, prune_big=False),
             dict(ACTOR, n_split=n_split), dict(KW, n_split=n_split), dict(ACTOR, n_split=n_split)]
    has_box = [False, True, False, True, False, True]
    meta = [dict(count=c, fourier_dim=2, sem_width=1) for c in (2500, 0, 255, 257, 1, 0)]
    tab = densify.scene_table(meta, rules)
    assert [(c.start, c.dc_offset, c.sem_offset) for c in tab] == [(0, 0, 0), (2500, 15000, 2500), (2500, 15000, 2500),
                                                                   (2755, 16530, 2755), (3012, 18072, 3012), (3013, 18078, 3013)]
    # kept originals, clones, split points, split points with children (the deferred plan: the last two are equal)
    totals = [[2000, 300, 500, 500], [0, 0, 0, 0], [255, 0, 0, 0], [200, 57, 57, 57], [0, 0, 1, 1], [0, 0, 0, 0]]
    lay = densify.scene_layout(tab, len(meta), totals)
    cand, norm, box, requests = _layout_numpy(totals, n_split, has_box)
    assert np.array_equal(lay["cand_base"], cand) and np.array_equal(lay["normals_base"], norm)
    assert np.array_equal(lay["box_base"], box)
    assert lay["requests"] == requests
    # the empty actors still ask for their (empty) box block, as the per-model call does; the model that splits nothing asks
    # for no split block
    assert (1, "box", 0) in requests and (5, "box", 0) in requests and not any(s == 2 for s, _, _ in requests)
