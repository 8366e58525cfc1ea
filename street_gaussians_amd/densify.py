"""Adaptive density control as plan + gather (include/sgr_densify.h).

``densify_and_prune`` computes what ``GaussianModel.densify_and_prune`` of the reference computes
(/root/reference/lib/models/gaussian_model.py:522-553: densify_and_clone :494-520, densify_and_split :448-492,
prune_points :409-427, with the Adam-state surgery of cat_optimizer / prune_optimizer :363-407) on plain tensors:
it returns the new parameter tensors, the new Adam moments and the reference's ``scalar_dict`` counters.  Wrapping the
results back into ``nn.Parameter`` / ``optimizer.state`` stays with the caller.

The split draws ``samples = normal(0, std)``; here the caller may pass the standard normals (``normals``), otherwise
they are drawn with ``torch.randn`` -- same distribution, not the same random stream.  GPU only.

``variant`` selects the prune rule of the model classes street_gaussians instantiates (both override the base method):
``"bkgd"`` = GaussianModelBkgd.densify_and_prune (gaussian_model_bkgd.py:74-114: big points farther than
2 * sphere_radius from sphere_center are exempt; scalars also carry points_below_min_opacity / points_big_ws) and
``"actor"`` = GaussianModelActor.densify_and_prune (gaussian_model_actor.py:204-261: points whose sampled extent
leaves the tracking box are pruned).  Those rules look at the NEW points' positions, so the candidates (kept originals,
clones, split children) are laid out first and pruned in a second step (sgr_densify_prune_mask / _compact).
``reset_opacity`` is GaussianModel.reset_opacity (gaussian_model.py:410-414).

``densify_scene`` is the reference's loop over its models (street_gaussian_model.py:573-586) for a ``scene.FlatScene``: every
model's own rule applied to its block of the flat tensors in one pass (include/sgr_densify_scene.h), bit-identical to
calling ``densify_and_prune`` per model and concatenating."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _alloc, _native
from ._native import SgrError, call, check, ptr, require_hip

PARAMS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic")  # optimiser group names (:409-412)


class _CParams(C.Structure):
    _fields_ = [("max_grad", C.c_float), ("min_opacity", C.c_float), ("extent", C.c_float), ("percent_dense", C.c_float),
                ("percent_big_ws", C.c_float), ("prune_big", C.c_int32), ("grad_column", C.c_int32), ("n_split", C.c_int32),
                ("defer_prune", C.c_int32)]


_VARIANTS = {None: 0, "base": 0, "bkgd": 1, "actor": 2}


# ---- memory for a loop that re-sizes under load ------------------------------------------------------------------------
# Every densify step changes N: parameters, gradients, Adam moments and the rasterizer's three scratch buffers come back in
# new sizes, and with an empty caching allocator every new size is a device allocation (tens of ms for a multi-GB block on
# some hosts -- in the middle of a training step).  The reference lives with that (torch.cat per parameter,
# gaussian_model.py:363-407).  Here the trainer reserves ONE block of about twice the bytes that are live at the largest
# size it expects and hands it straight back to torch's caching allocator, which then serves every re-sized tensor by
# splitting it: no device allocation inside the loop.  The pool belongs to the library (round 4 left a fixed 48 GB
# reservation in bench.py); it grows (by the difference, at least an eighth) when the estimate outgrows it; a request that did not fit is not repeated.
def live_bytes_estimate(n_points: int, sh_coeffs: int = 16, semantic_channels: int = 0, instances_per_point: float = 8.0) -> int:
    """Bytes live at n_points Gaussians in one training iteration: raw parameters, gradients, two Adam moments, the activated
    rasterizer inputs with their gradients, the geometry / binning buffers and the backward's partial rows
    (140 B per Gaussian, 18.5 + 48 B per tile instance)."""
    per_point = 4 * (3 + 3 * sh_coeffs + 1 + 3 + 4 + semantic_channels)  # one copy of the parameters
    inst = int(instances_per_point * n_points)
    return int(n_points * (4 * per_point + 2 * per_point + 140 + 64) + inst * (18.5 + 48 + 4 * semantic_channels))


class Pool:
    """reserve(n_points): makes sure torch's caching allocator holds one free block of `factor` x the live-bytes estimate
    (head-room for the size steps of the ladder, _alloc.py, and for the densify step itself, where the old and the new
    parameters + Adam moments are alive together)."""

    def __init__(self, device, factor: float = 1.5, **estimate_kw):
        self.device, self.factor, self.kw = torch.device(device), float(factor), estimate_kw
        self.reserved = 0  # bytes handed to the allocator so far (the sum of the blocks below)
        self.failed_at = None  # smallest request that did not fit: not asked for again (a failed torch allocation flushes the
                               # caching allocator first -- exactly the stall the pool exists to remove)

    def reserve(self, n_points: int) -> int:
        want = int(self.factor * live_bytes_estimate(n_points, **self.kw))
        if want <= self.reserved:
            return self.reserved
        want = max(want, self.reserved + self.reserved // 8)
        # grow by the DELTA: the block reserved earlier stays with the allocator (possibly split among live tensors), so a
        # fresh block of `want` bytes next to it would make the allocator hold reserved + want
        delta = want - self.reserved
        if self.failed_at is not None and delta >= self.failed_at:
            return self.reserved
        try:
            blk = torch.empty(delta, dtype=torch.uint8, device=self.device)
            del blk  # stays with the caching allocator as a free block
            self.reserved = want
        except RuntimeError:
            self.failed_at = delta  # not enough memory for the head-room: the loop allocates as it goes, and is not asked again
        return self.reserved


def densify_and_prune(params: Dict[str, torch.Tensor], xyz_gradient_accum: torch.Tensor, denom: torch.Tensor, *,
                      max_grad: float, min_opacity: float, extent: float, percent_dense: float, percent_big_ws: float,
                      prune_big: bool, states: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = None,
                      grad_column: int = 0, n_split: int = 2, normals: Optional[torch.Tensor] = None,
                      variant: Optional[str] = None, sphere_center=None, sphere_radius: Optional[float] = None,
                      box_min=None, box_max=None, box_normals: Optional[torch.Tensor] = None, normal_source=None):
    """params: {'xyz' [N,3], 'f_dc' [N,C,3], 'f_rest' [N,M-1,3], 'opacity' [N,1], 'scaling' [N,3], 'rotation' [N,4],
    'semantic' [N,S]} raw parameters; states: optional {name: (exp_avg, exp_avg_sq)} shaped like the parameters.
    Returns (new_params, new_states, scalars, index) with scalars = {'points_total', 'points_clone', 'points_split',
    'points_pruned'} and index = {'src', 'kind'} (source row and 0 keep / 1 clone / 2 split child per result row).
    variant "bkgd" needs sphere_center [3] and sphere_radius; variant "actor" needs box_min / box_max [3] and takes
    box_normals [n_candidates, 2, 3] (standard normals; drawn when omitted).
    normal_source: a callable (rows, device[, cols]) -> standard normals, asked for the split's samples (and the actor
    variant's box samples) when the tensors are not given -- how view-sharded training keeps replicated Gaussians
    identical across ranks (multiview.ReplicatedNormals)."""
    if variant not in _VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    require_hip("densify_and_prune needs HIP (cuda) tensors: there is no CPU path", params["xyz"])
    dev = params["xyz"].device
    rule = dict(max_grad=max_grad, min_opacity=min_opacity, extent=extent, percent_dense=percent_dense,
                percent_big_ws=percent_big_ws, prune_big=prune_big, grad_column=grad_column, n_split=n_split)
    # one guard, one library and stream lookup and hand-written launches for the ~30 launches of a call: _native.call per
    # launch costs 1-2 us each, which shows in a loop over many small models (profiles/bindings_refactor/bench.json)
    with torch.cuda.device(dev):
        on = (_native.lib(), _native.stream(dev))
        if _VARIANTS[variant] != 0:
            return _densify_two_step(on, params, xyz_gradient_accum, denom, states=states, normals=normals,
                                     variant=variant, sphere_center=sphere_center, sphere_radius=sphere_radius,
                                     box_min=box_min, box_max=box_max, box_normals=box_normals,
                                     normal_source=normal_source, **rule)
        cp, counts, src, kind, srow, new_params = _candidates(on, params, xyz_gradient_accum, denom,
                                                              [k for k in PARAMS if k in params], False, normals,
                                                              normal_source, **rule)
        N, n_out = params["xyz"].shape[0], src.numel()
        new_states = None
        if states is not None:
            new_states = {k: (_gather(on, a, src, kind, n_out, True, N), _gather(on, b, src, kind, n_out, True, N))
                          for k, (a, b) in states.items()}
    return new_params, new_states, _scalars(counts[0], counts[1], counts[2], counts[3]), {"src": src, "kind": kind}


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _gather(on, t, src, kind, n_out, zero_new, N):
    t = _f32(t)
    width = t[0].numel() if N else 0
    out = _alloc.empty((n_out,) + tuple(t.shape[1:]), torch.float32, t.device)  # ladder-sized backing: see _alloc.py
    L, s = on
    check(L.sgr_densify_gather(n_out, width, ptr(t), ptr(src), ptr(kind), int(zero_new), ptr(out), s))
    return out


def _draw_normals(given, shape, normal_source, dev, name):
    """Standard normals of ``shape`` ([rows, 3] or [rows, 2, 3]) as contiguous float32: the caller's tensor ``given``, else
    the rows ``normal_source`` hands out, else ``torch.randn``'s."""
    if given is None:
        if normal_source is None:
            given = torch.randn(*shape, device=dev)
        else:
            given = normal_source(math.prod(shape[:-1]), dev)
            if len(shape) > 2:
                given = given.view(shape)
    if tuple(given.shape) != tuple(shape):
        raise RuntimeError(f"{name} must have dimensions {tuple(shape)}")
    return _f32(given)


def _gather_and_split(on, T, scaling, keys, src, kind, srow, N, n_split, n_norm, normals, normal_source=None):
    """The candidates' rows of ``T[k]`` for k in ``keys`` (xyz and scaling among them), split children computed from
    ``n_norm`` standard normals (``_draw_normals``).  ``scaling``: T["scaling"] as contiguous float32, which the caller has."""
    n_cand = src.numel()
    cand = {k: _gather(on, T[k], src, kind, n_cand, False, N) for k in keys}
    if n_norm:
        zs = _draw_normals(normals, (n_norm, 3), normal_source, src.device, "normals")
        L, s = on
        check(L.sgr_densify_split_children(n_cand, int(n_split), ptr(src), ptr(kind), ptr(srow), ptr(_f32(T["xyz"])),
                                           ptr(scaling), ptr(_f32(T["rotation"])), ptr(zs), ptr(cand["xyz"]),
                                           ptr(cand["scaling"]), s))
    return cand


def _candidates(on, params, xyz_gradient_accum, denom, keys, defer_prune, normals, normal_source, *, max_grad,
                min_opacity, extent, percent_dense, percent_big_ws, prune_big, grad_column, n_split):
    """The front of a per-model densify: the parameter struct, the plan (``counts``: total, clones, split points, pruned,
    candidate rows, normals), the candidates' ``src`` / ``kind`` / ``srow`` map and their rows of ``params[k]`` for k in
    ``keys`` with the split children computed.  ``defer_prune``: the plan prunes nothing (the two-step variants)."""
    xyz = params["xyz"]
    dev, N = xyz.device, xyz.shape[0]
    cp = _CParams(float(max_grad), float(min_opacity), float(extent), float(percent_dense), float(percent_big_ws),
                  int(bool(prune_big)), int(grad_column), int(n_split), int(defer_prune))
    counts = (C.c_int64 * 6)()
    acc, den, sc, op = _f32(xyz_gradient_accum), _f32(denom), _f32(params["scaling"]), _f32(params["opacity"])
    L, s = on
    work = torch.empty(L.sgr_densify_work_bytes(N), dtype=torch.uint8, device=dev)
    check(L.sgr_densify_plan(N, C.byref(cp), ptr(acc), ptr(den), ptr(sc), ptr(op), ptr(work), counts, s))
    n_cand, n_norm = int(counts[4]), int(counts[5])
    src = torch.empty(n_cand, dtype=torch.int32, device=dev)
    kind = torch.empty(n_cand, dtype=torch.uint8, device=dev)
    srow = torch.empty(n_cand, dtype=torch.int32, device=dev)
    check(L.sgr_densify_map(N, C.byref(cp), ptr(work), ptr(src), ptr(kind), ptr(srow), s))
    cand = _gather_and_split(on, params, sc, keys, src, kind, srow, N, n_split, n_norm, normals, normal_source)
    return cp, counts, src, kind, srow, cand


def _floats(v, n, what, strict):
    """``v`` as a list of floats; with ``strict``, a ValueError unless it holds n values."""
    out = [float(x) for x in torch.as_tensor(v).flatten().tolist()]
    if strict and len(out) != n:
        raise ValueError(f"densify_scene: {what} must hold {n} values, got {len(out)}")
    return out


def _regions(rule, where="", strict=False):
    """A rule's (sphere, box) as the kernels take them -- centre + radius for the bkgd variant, min + max for the actor
    variant with prune_big, None where the rule has none.  ValueError for a missing value and, with ``strict``, for one of
    the wrong length; ``where`` prefixes the message."""
    sphere = box = None
    if rule["variant"] == "bkgd":
        if rule["sphere_center"] is None or rule["sphere_radius"] is None:
            raise ValueError(f'{where}variant "bkgd" needs sphere_center and sphere_radius')
        c = _floats(rule["sphere_center"], 3, "sphere_center", strict)
        sphere = (C.c_float * 4)(c[0], c[1], c[2], _floats(rule["sphere_radius"], 1, "sphere_radius", strict)[0])
    if rule["variant"] == "actor" and rule["prune_big"]:
        if rule["box_min"] is None or rule["box_max"] is None:
            raise ValueError(f'{where}variant "actor" needs box_min and box_max')
        box = (C.c_float * 6)(*_floats(rule["box_min"], 3, "box_min", strict), *_floats(rule["box_max"], 3, "box_max", strict))
    return sphere, box


def _scalars(total, clone, split, pruned, variant=0, prune_big=False, pc=None):
    """The reference's scalar_dict of one model.  For the bkgd variant (``variant`` is its number) the extras come from the
    prune's counters ``pc`` (below min opacity, big in world space, ...)."""
    d = {"points_total": int(total), "points_clone": int(clone), "points_split": int(split), "points_pruned": int(pruned)}
    if variant == _VARIANTS["bkgd"]:
        d["points_below_min_opacity"] = int(pc[0])
        if prune_big:
            d["points_big_ws"] = int(pc[1])
    return d


def _densify_two_step(on, params, xyz_gradient_accum, denom, *, states, normals, variant, sphere_center, sphere_radius,
                      box_min, box_max, box_normals, normal_source=None, **rule):
    cp, counts, src, kind, srow, cand = _candidates(on, params, xyz_gradient_accum, denom,
                                                    ("xyz", "scaling", "rotation", "opacity"), True, normals, normal_source,
                                                    **rule)
    dev, N, n_cand = src.device, params["xyz"].shape[0], src.numel()
    sphere, box = _regions(dict(variant=variant, prune_big=rule["prune_big"], sphere_center=sphere_center,
                                sphere_radius=sphere_radius, box_min=box_min, box_max=box_max))
    if box is not None:
        box_normals = _draw_normals(box_normals, (n_cand, 2, 3), normal_source, dev, "box_normals")
    prune = torch.empty(n_cand, dtype=torch.uint8, device=dev)
    pc = (C.c_int64 * 4)()
    L, s = on
    check(L.sgr_densify_prune_mask(n_cand, C.byref(cp), _VARIANTS[variant], ptr(cand["xyz"]), ptr(cand["scaling"]),
                                   ptr(cand["rotation"]), ptr(cand["opacity"]), sphere, box,
                                   ptr(box_normals) if box is not None else None, ptr(prune), pc, s))
    sel = torch.empty(n_cand, dtype=torch.int32, device=dev)
    n_out = C.c_int64(0)
    work2 = torch.empty(L.sgr_densify_work_bytes(n_cand), dtype=torch.uint8, device=dev)
    check(L.sgr_densify_compact(n_cand, ptr(prune), ptr(work2), ptr(sel), C.byref(n_out), s))
    n_out = int(n_out.value)
    sel = sel[:n_out]
    sel64 = sel.long()
    src_f, kind_f = src[sel64].contiguous(), kind[sel64].contiguous()
    keep0 = torch.zeros(n_out, dtype=torch.uint8, device=dev)  # rows copied from the candidate arrays as they are
    new_params = {}
    for k in PARAMS:
        if k not in params:
            continue
        if k in cand:
            new_params[k] = _gather(on, cand[k], sel, keep0, n_out, False, n_cand)
            if params[k].dim() != new_params[k].dim():
                new_params[k] = new_params[k].reshape((n_out,) + tuple(params[k].shape[1:]))
        else:
            new_params[k] = _gather(on, params[k], src_f, kind_f, n_out, False, N)
    new_states = None
    if states is not None:
        new_states = {k: (_gather(on, a, src_f, kind_f, n_out, True, N), _gather(on, b, src_f, kind_f, n_out, True, N))
                      for k, (a, b) in states.items()}
    scalars = _scalars(counts[0], counts[1], counts[2], pc[3], _VARIANTS[variant], rule["prune_big"], pc)
    return new_params, new_states, scalars, {"src": src_f, "kind": kind_f}


# ---- a whole FlatScene in one pass (include/sgr_densify_scene.h) -----------------------------------------------------
class _CSceneSeg(C.Structure):
    _fields_ = [("start", C.c_int32), ("count", C.c_int32), ("dc_width", C.c_int32), ("sem_width", C.c_int32),
                ("dc_offset", C.c_int64), ("sem_offset", C.c_int64), ("params", _CParams), ("variant", C.c_int32),
                ("sphere", C.c_float * 4), ("box", C.c_float * 6)]


_RULE_REQUIRED = ("max_grad", "min_opacity", "extent", "percent_dense", "percent_big_ws", "prune_big")
_RULE_OPTIONAL = {"grad_column": 0, "n_split": 2, "variant": None, "sphere_center": None, "sphere_radius": None,
                  "box_min": None, "box_max": None}
_FLAT_ATTRS = ("xyz", "rotation", "scaling", "opacity", "features_dc", "features_rest", "semantic")


def scene_table(meta: Sequence[dict], rules: Sequence[dict]):
    """The sgr_densify_scene_segment table (host) of a FlatScene's ``meta`` and one rule per model: the keyword arguments
    of ``densify_and_prune`` (max_grad, min_opacity, extent, percent_dense, percent_big_ws, prune_big; optional grad_column,
    n_split, variant, sphere_center, sphere_radius, box_min, box_max).  ValueError for a malformed rule."""
    if len(rules) != len(meta):
        raise ValueError(f"densify_scene: {len(meta)} models but {len(rules)} rules")
    tab = (_CSceneSeg * max(len(meta), 1))()
    row = dc = sem = 0
    nan = float("nan")
    for i, (m, rule) in enumerate(zip(meta, rules)):
        unknown = [k for k in rule if k not in _RULE_REQUIRED and k not in _RULE_OPTIONAL]
        missing = [k for k in _RULE_REQUIRED if k not in rule]
        if unknown or missing:
            raise ValueError(f"densify_scene: rules[{i}]: unknown keys {unknown}, missing keys {missing}")
        r = dict(_RULE_OPTIONAL, **rule)
        if r["variant"] not in _VARIANTS:
            raise ValueError(f"densify_scene: rules[{i}]: unknown variant {r['variant']!r}")
        c = tab[i]
        n, dcw, sw = int(m["count"]), 3 * int(m["fourier_dim"]), int(m["sem_width"])
        c.start, c.count, c.dc_width, c.sem_width, c.dc_offset, c.sem_offset = row, n, dcw, sw, dc, sem
        row, dc, sem = row + n, dc + n * dcw, sem + n * sw
        c.params = _CParams(float(r["max_grad"]), float(r["min_opacity"]), float(r["extent"]), float(r["percent_dense"]),
                            float(r["percent_big_ws"]), int(bool(r["prune_big"])), int(r["grad_column"]), int(r["n_split"]), 1)
        c.variant = _VARIANTS[r["variant"]]
        sphere, box = _regions(r, f"densify_scene: rules[{i}]: ", strict=True)
        c.sphere = sphere if sphere is not None else (C.c_float * 4)(nan, nan, nan, nan)
        c.box = box if box is not None else (C.c_float * 6)(*[nan] * 6)
    return tab


def scene_layout(table, nseg: int, totals) -> dict:
    """Where every model's blocks start, from the per-model totals of the plan ([nseg, 4]: kept originals, clones, split
    points, split points with children), by sgr_densify_scene_layout (host only).  Returns ``cand_base``, ``normals_base``,
    ``box_base`` (nseg + 1 entries each, the last = the size of the candidate arrays / of ``normals`` / of ``box_normals``
    in rows) and ``requests``: the ``(model, "split" | "box", rows)`` blocks of standard normals in the order the per-model
    loop asks its ``normal_source`` for them -- per model its split block (when it splits anything), then its box block (the
    actor rule with prune_big: two samples per candidate, also when it has no candidates)."""
    tot = (C.c_int64 * (4 * nseg))(*[int(v) for v in np.asarray(totals).reshape(-1)])
    lay = (C.c_int64 * (3 * (nseg + 1)))()
    check(_native.lib().sgr_densify_scene_layout(nseg, table, tot, lay))
    lay = np.array(lay[:], dtype=np.int64).reshape(nseg + 1, 3)
    requests = []
    for s in range(nseg):
        n_norm, n_box = int(lay[s + 1, 1] - lay[s, 1]), int(lay[s + 1, 0] - lay[s, 0])
        if n_norm:
            requests.append((s, "split", n_norm))
        if table[s].variant == _VARIANTS["actor"] and table[s].params.prune_big:
            requests.append((s, "box", 2 * n_box))
    return {"cand_base": lay[:, 0], "normals_base": lay[:, 1], "box_base": lay[:, 2], "requests": requests}


def _scene_normals(lay, normals, box_normals, normal_source, dev):
    """The scene's ``normals`` [rows, 3] and ``box_normals`` [rows, 2, 3]: the caller's tensors (shape-checked), else
    filled block by block from ``normal_source`` / ``torch.randn`` in the order of ``lay['requests']``."""
    n_norm, n_box = int(lay["normals_base"][-1]), int(lay["box_base"][-1])
    given = {"split": normals is not None, "box": box_normals is not None}
    if given["split"] and tuple(normals.shape) != (n_norm, 3):
        raise ValueError(f"densify_scene: normals must have dimensions ({n_norm}, 3)")
    if given["box"] and tuple(box_normals.shape) != (n_box, 2, 3):
        raise ValueError(f"densify_scene: box_normals must have dimensions ({n_box}, 2, 3)")
    out = {"split": _f32(normals) if given["split"] else torch.empty(n_norm, 3, device=dev),
           "box": _f32(box_normals).view(2 * n_box, 3) if given["box"] else torch.empty(2 * n_box, 3, device=dev)}
    base = {"split": lay["normals_base"], "box": 2 * lay["box_base"]}
    for s, what, rows in lay["requests"]:
        if given[what]:
            continue
        t = normal_source(rows, dev) if normal_source is not None else torch.randn(rows, 3, device=dev)
        if tuple(t.shape) != (rows, 3):
            raise ValueError(f"densify_scene: normal_source returned {tuple(t.shape)} for a request of ({rows}, 3)")
        if rows:
            b = int(base[what][s])
            out[what][b:b + rows].copy_(t)
    return out["split"], out["box"]


def densify_scene(flat, xyz_gradient_accum: torch.Tensor, denom: torch.Tensor, rules: Sequence[dict],
                  moments: Optional[Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]] = None,
                  normals: Optional[torch.Tensor] = None, box_normals: Optional[torch.Tensor] = None, normal_source=None):
    """Density control of every model of a ``scene.FlatScene`` in one pass: ``rules[i]`` (see ``scene_table``) is applied to
    model i's block.  ``xyz_gradient_accum`` [N, 2] / ``denom`` [N, 1] are ``scene.FlatStats``' flat tensors; ``moments`` =
    ``(exp_avg, exp_avg_sq)``, dicts keyed by flat attribute as ``optim.SegmentedAdam`` holds them.

    Returns ``(new_flat, new_moments, scalars, index)``: block i of every new flat tensor is bit for bit what
    ``densify_and_prune(flat.views()[i], ..., **rules[i])`` returns (moments of new rows zero), ``scalars[i]`` is that
    call's counter dict, ``index`` = {'src' (flat source row), 'kind', 'counts' (rows per model)}.  ``new_flat`` shares
    ``flat``'s pose leaf and per-model settings; hand ``new_moments`` to ``SegmentedAdam.rebuild_flat``.

    ``normals`` [sum of n_split * points_split, 3] / ``box_normals`` [sum of the candidates of the actor models with
    prune_big, 2, 3] are the per-model tensors concatenated in model order; when not given, ``normal_source`` (or
    ``torch.randn``) is asked per model, in the per-model loop's order and sizes (``scene_layout``).  Two host waits and
    a fixed number of launches, whatever the number of models; n_split is one value for the scene.  GPU only."""
    from .optim import _pinned_to
    from .scene import FlatScene
    K = len(flat.meta)
    table = scene_table(flat.meta, rules)
    if K == 0:
        raise ValueError("densify_scene: the scene has no models")
    if moments is not None:
        if len(moments) != 2 or any(set(d) != set(_FLAT_ATTRS) for d in moments):
            raise ValueError(f"densify_scene: moments = (exp_avg, exp_avg_sq), each a dict with the keys {_FLAT_ATTRS}")
    ins = [flat.tensors[k] for k in _FLAT_ATTRS] + [xyz_gradient_accum, denom] + ([t for d in moments for t in d.values()] if moments else [])
    require_hip("densify_scene needs HIP (cuda) tensors: there is no CPU path", *ins)
    dev, N = flat.xyz.device, int(flat.xyz.shape[0])
    L = _native.lib()
    T = {k: _f32(flat.tensors[k]) for k in _FLAT_ATTRS}
    if moments is not None:
        for d in moments:
            for k in _FLAT_ATTRS:
                if d[k].numel() != T[k].numel():
                    raise ValueError(f"densify_scene: the moments of {k} have {d[k].numel()} elements, the parameter {T[k].numel()}")
    acc, den = _f32(xyz_gradient_accum), _f32(denom)
    if acc.numel() != 2 * N or den.numel() != N:
        raise ValueError(f"densify_scene: statistics of {den.numel()} rows for a scene of {N}")
    want = {"xyz": 3 * N, "rotation": 4 * N, "scaling": 3 * N, "opacity": N,  # the kernels index by these sizes
            "features_dc": sum(c.count * c.dc_width for c in table), "semantic": sum(c.count * c.sem_width for c in table)}
    if sum(c.count for c in table) != N or any(T[k].numel() != n for k, n in want.items()) or T["features_rest"].shape[0] != N:
        raise ValueError("densify_scene: the flat tensors do not have the sizes flat.meta describes")
    n_split = int(table[0].params.n_split)
    stream = _native.stream(dev)
    on = (L, stream)  # what the per-model helpers launch on
    with torch.cuda.device(dev):
        table_dev = _pinned_to(np.frombuffer(table, dtype=np.uint8), dev)
        segs = (table, ptr(table_dev))
        work = torch.empty(L.sgr_densify_scene_work_bytes(N, K), dtype=torch.uint8, device=dev)
        totals = (C.c_int64 * (4 * K))()
        check(L.sgr_densify_scene_plan(N, K, *segs, ptr(acc), ptr(den), ptr(T["scaling"]), ptr(T["opacity"]), ptr(work),
                                       totals, stream))                                                   # host wait 1
        lay = scene_layout(table, K, totals)
        n_cand, n_norm = int(lay["cand_base"][-1]), int(lay["normals_base"][-1])
        zs, zb = _scene_normals(lay, normals, box_normals, normal_source, dev)
        src = torch.empty(n_cand, dtype=torch.int32, device=dev)
        kind = torch.empty(n_cand, dtype=torch.uint8, device=dev)
        srow = torch.empty(n_cand, dtype=torch.int32, device=dev)
        check(L.sgr_densify_scene_map(N, K, *segs, ptr(work), ptr(src), ptr(kind), ptr(srow), stream))
        # the candidates' geometry: gathered rows, split children computed (the per-model kernels: src holds flat rows)
        cand = _gather_and_split(on, T, T["scaling"], ("xyz", "scaling", "rotation", "opacity"), src, kind, srow, N, n_split,
                                 n_norm, zs)
        sel = torch.empty(n_cand, dtype=torch.int32, device=dev)
        src_f = torch.empty(n_cand, dtype=torch.int32, device=dev)
        kind_f = torch.empty(n_cand, dtype=torch.uint8, device=dev)
        cand_work = torch.empty(L.sgr_densify_scene_work_bytes(n_cand, K), dtype=torch.uint8, device=dev)
        pc = (C.c_int64 * (5 * K))()
        check(L.sgr_densify_scene_prune(n_cand, K, *segs, ptr(cand["xyz"]), ptr(cand["scaling"]), ptr(cand["rotation"]),
                                        ptr(cand["opacity"]), ptr(zb) if zb.numel() else None, ptr(src), ptr(kind), ptr(work),
                                        ptr(cand_work), ptr(sel), ptr(src_f), ptr(kind_f), pc, stream))        # host wait 2
        pc = np.array(pc[:], dtype=np.int64).reshape(K, 5)
        new_counts = [int(v) for v in pc[:, 4]]
        n_out = sum(new_counts)
        sel, src_f, kind_f = sel[:n_out], src_f[:n_out], kind_f[:n_out]
        nc = (C.c_int64 * K)(*new_counts)

        def ragged(t, which, zero_new):
            width = "sem_width" if which else "dc_width"
            out = _alloc.empty((sum(n * getattr(table[s], width) for s, n in enumerate(new_counts)),), torch.float32, dev)
            check(L.sgr_densify_scene_gather_ragged(K, *segs, nc, ptr(work), which, ptr(t), ptr(src_f), ptr(kind_f),
                                                    int(zero_new), ptr(out), stream))
            return out

        def final(k, t, zero_new):
            if k in ("features_dc", "semantic"):
                return ragged(t, int(k == "semantic"), zero_new)
            if k in cand and not zero_new:  # rows of the candidate arrays as they are (split children are computed rows)
                return _gather(on, cand[k], sel, kind_f, n_out, False, n_cand)
            return _gather(on, t, src_f, kind_f, n_out, zero_new, N)

        new_tensors = {k: final(k, T[k], False).requires_grad_(flat.tensors[k].requires_grad) for k in _FLAT_ATTRS}
        new_moments = None
        if moments is not None:
            new_moments = tuple({k: final(k, _f32(d[k]).view(T[k].shape), True) for k in _FLAT_ATTRS} for d in moments)
    new_flat = FlatScene([dict(m, count=n) for m, n in zip(flat.meta, new_counts)], new_tensors, flat.poses)
    tot = np.array(totals[:], dtype=np.int64).reshape(K, 4)
    scalars = [_scalars(c.count, tot[s, 1], tot[s, 2], pc[s, 3], c.variant, c.params.prune_big, pc[s])
               for s, c in enumerate(table)]
    return new_flat, new_moments, scalars, {"src": src_f, "kind": kind_f, "counts": new_counts}


def reset_opacity(opacity: torch.Tensor, state: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """GaussianModel.reset_opacity (gaussian_model.py:410-414): returns inverse_sigmoid(min(sigmoid(opacity), 0.01)) as a
    new tensor; ``state`` = the group's (exp_avg, exp_avg_sq), zero-filled IN PLACE like reset_optimizer (:344-361)."""
    require_hip("reset_opacity needs a HIP (cuda) tensor: there is no CPU path", opacity)
    dev = opacity.device
    out = opacity.detach().to(torch.float32).contiguous().clone()
    a = b = None
    if state is not None:
        a, b = state
        for t in (a, b):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != out.numel():
                raise SgrError("the Adam moments must be contiguous float32 tensors shaped like opacity")
    call("sgr_reset_opacity", dev, out.numel(), out, a, b)
    return out
