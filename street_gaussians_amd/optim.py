"""Per-segment Adam over a ``scene.FlatScene`` (include/sgr_optim.h).

The reference trains one ``torch.optim.Adam(eps=1e-15)`` per sub-model with seven named groups (``xyz, f_dc, f_rest,
opacity, scaling, rotation, semantic``: the reference's lib/models/gaussian_model.py:292-304,
gaussian_model_actor.py:170-192) and steps it once per iteration (``update_optimizer``, gaussian_model.py:316-318).
Adam's update does not change when a gradient is scaled, so a single Adam over the flat leaves cannot express
per-model learning rates, and it would keep one step count where the reference keeps one per model: a model absent
from a frame gets no gradient, and torch's Adam skips it (no moment decay, no move, no step).

``SegmentedAdam`` keeps the learning rate and the step count per (segment, group) and updates every present block of
every flat leaf in one HIP launch, with the arithmetic of torch's ``_multi_tensor_adam`` (op order in the header).
Its state reads and writes as ``torch.optim.Adam.state_dict()`` per model, and as the ``(exp_avg, exp_avg_sq)`` pairs
``densify.densify_and_prune(states=...)`` takes.  ``sink()`` plans a step that the backward of
``FlatScene.compose(grad_sink=...)`` applies itself, without gradient tensors (include/sgr_scene_step.h).  There is no
CPU implementation: tensors must live on the GPU."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from ._native import SgrError, launch, require_hip

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic")
# group name -> FlatScene attribute
ATTR = {"xyz": "xyz", "f_dc": "features_dc", "f_rest": "features_rest", "opacity": "opacity", "scaling": "scaling",
        "rotation": "rotation", "semantic": "semantic"}

CHUNK_DTYPE = np.dtype([("p", "<u8"), ("m", "<u8"), ("v", "<u8"), ("count", "<i8")])
RECORD_DTYPE = np.dtype([("g", "<u8"), ("chunk", "<i4"), ("span_start", "<i4"), ("step_size", "<f4"),
                         ("bc2_sqrt", "<f4"), ("eps", "<f4"), ("pad", "<i4")])
assert CHUNK_DTYPE.itemsize == 32 and RECORD_DTYPE.itemsize == 32


def bias_corrections(step: int, beta1: float, beta2: float) -> Tuple[float, float]:
    """(bc1, bc2_sqrt) in double, as torch/optim/adam.py: _multi_tensor_adam computes them from ``step.item()``."""
    s = float(step)
    bc1 = 1 - beta1 ** s
    bc2 = 1 - beta2 ** s
    return bc1, bc2 ** 0.5


def segment_layout(meta: Sequence[dict], rest_width: int) -> List[Dict[str, Tuple[int, int, tuple]]]:
    """Per segment: {group: (element offset in the flat tensor, element count, per-model shape)}.  ``rest_width`` is the
    row width of the flat features_rest tensor (3 (M - 1))."""
    out, row, dc, sem = [], 0, 0, 0
    for m in meta:
        n, fd, sw = int(m["count"]), int(m["fourier_dim"]), int(m["sem_width"])
        out.append({"xyz": (3 * row, 3 * n, (n, 3)),
                    "f_dc": (dc, 3 * fd * n, (n, fd, 3)),
                    "f_rest": (rest_width * row, rest_width * n, (n, rest_width // 3, 3)),
                    "opacity": (row, n, (n, 1)),
                    "scaling": (3 * row, 3 * n, (n, 3)),
                    "rotation": (4 * row, 4 * n, (n, 4)),
                    "semantic": (sem, sw * n, (n, sw))})
        row += n
        dc += 3 * fd * n
        sem += sw * n
    return out


def _rest_width(flat) -> int:
    t = flat.tensors["features_rest"]
    return int(t.shape[1]) if t.dim() == 2 else 0


def _spans(count: int, span: int) -> int:
    return (count + span - 1) // span


def _pinned_to(arr: np.ndarray, dev) -> torch.Tensor:
    """Device copy of a host table through a pinned staging buffer and a non-blocking copy on the current stream (torch's
    host allocator keeps the staging block until the copy has completed): no host synchronisation."""
    raw = arr.view(np.uint8).reshape(-1)
    host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = raw
    return host.to(dev, non_blocking=True)


def chunk_table(layout, p: Dict[str, int], m: Dict[str, int], v: Dict[str, int]) -> np.ndarray:
    """sgr_adam_chunk table (CHUNK_DTYPE) of every (segment, group), index seg * 7 + group, from the base addresses of
    the flat parameter and moment tensors per group.  Empty chunks have null pointers."""
    tab = np.zeros(len(layout) * len(GROUPS), dtype=CHUNK_DTYPE)
    for s, lay in enumerate(layout):
        for gi, g in enumerate(GROUPS):
            off, cnt, _ = lay[g]
            i = s * len(GROUPS) + gi
            tab["count"][i] = cnt
            if cnt:
                tab["p"][i], tab["m"][i], tab["v"][i] = p[g] + 4 * off, m[g] + 4 * off, v[g] + 4 * off
    return tab


def step_scalars(step: int, lr: float, betas: Tuple[float, float], bc_cache: dict) -> Tuple[float, float]:
    """(step_size, bc2_sqrt) of one (segment, group) at step count ``step``, in double: ``-(lr / bc1)`` and
    ``(1 - beta2 ** step) ** 0.5`` (include/sgr_optim.h).  The one definition ``plan_step`` and ``plan_sink`` share;
    ``bc_cache`` keeps the bias corrections per step count.  The caller rounds to float32."""
    bc = bc_cache.get(step)
    if bc is None:
        bc = bc_cache[step] = bias_corrections(step, *betas)
    return -(lr / bc[0]), bc[1]


def _segment_set(segments: Optional[Sequence[int]], nseg: int, who: str) -> List[int]:
    if segments is None:
        return list(range(nseg))
    segs = sorted({int(s) for s in segments})
    if segs and (segs[0] < 0 or segs[-1] >= nseg):
        raise IndexError(f"{who}: segment index out of range [0, {nseg})")
    return segs


def plan_sink(layout, steps: List[Dict[str, int]], lrs: List[Dict[str, float]], segments: Optional[Sequence[int]],
              groups: Sequence[str], betas: Tuple[float, float], bc_cache: Optional[dict] = None
              ) -> Dict[Tuple[int, str], Tuple[np.float32, np.float32]]:
    """{(segment, group): (step_size, bc2_sqrt)} as float32, the scalars ``plan_step(advance=True)`` would put into its
    records for the same ``segments`` and groups: those of step count + 1.  Every (segment, group) of the set has an
    entry, an empty block included (its count advances on commit as torch steps an empty parameter).  ``steps`` is only
    read."""
    bc_cache = {} if bc_cache is None else bc_cache
    plan = {}
    for s in _segment_set(segments, len(layout), "SegmentedAdam.sink"):
        for g in GROUPS:
            if g in groups:
                ss, b2 = step_scalars(steps[s][g] + 1, lrs[s][g], betas, bc_cache)
                plan[(s, g)] = (np.float32(ss), np.float32(b2))
    return plan


def plan_step(layout, steps: List[Dict[str, int]], lrs: List[Dict[str, float]], segments: Optional[Sequence[int]],
              grads: Dict[str, int], betas: Tuple[float, float], eps: float, span: int, advance: bool = True,
              bc_cache: Optional[dict] = None, max_records: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """The sgr_adam_record table (RECORD_DTYPE) of one step and its span total.  A (segment, group) takes part when
    the segment is in ``segments`` (None = all) and the group's flat gradient is in ``grads`` ({group: base address});
    with ``advance`` its step count goes up by one first -- count 0 included, as torch steps an empty parameter -- and
    only chunks with count > 0 get a record.  A step of more than ``max_records`` records (sgr_adam_max_records()) is
    refused with an SgrError before any step count advances."""
    nseg = len(layout)
    segs = _segment_set(segments, nseg, "SegmentedAdam.step")
    if max_records is not None:
        n = sum(1 for s in segs for g in GROUPS if g in grads and layout[s][g][1])
        if n > max_records:
            raise SgrError(f"SegmentedAdam: {n} records in one step, the limit is {max_records} (sgr_adam_max_records): "
                           "step the segments in several calls")
    bc_cache = {} if bc_cache is None else bc_cache
    rec = np.zeros(nseg * len(GROUPS), dtype=RECORD_DTYPE)
    n, span_start = 0, 0
    for s in segs:
        lay, st, lr = layout[s], steps[s], lrs[s]
        for gi, g in enumerate(GROUPS):
            if g not in grads:
                continue
            if advance:
                st[g] += 1
            off, cnt, _ = lay[g]
            if not cnt:
                continue
            rec["g"][n] = grads[g] + 4 * off
            rec["chunk"][n] = s * len(GROUPS) + gi
            rec["span_start"][n] = span_start
            rec["step_size"][n], rec["bc2_sqrt"][n] = step_scalars(st[g], lr[g], betas, bc_cache)
            rec["eps"][n] = eps
            n += 1
            span_start += _spans(cnt, span)
    if span_start > 2 ** 31 - 1:
        raise SgrError("SegmentedAdam: more than 2^31 - 1 spans in one step")
    return rec[:n], span_start


def _group_defaults(betas, eps) -> dict:
    """The keys and defaults torch.optim.Adam puts in a param group, taken from torch itself."""
    probe = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=0.0, betas=betas, eps=eps)
    d = dict(probe.param_groups[0])
    d.pop("params")
    return d


def adam_state_dict(views: Dict[str, Tuple[torch.Tensor, torch.Tensor]], steps: Dict[str, int], lrs: Dict[str, float],
                    betas, eps) -> dict:
    """``torch.optim.Adam.state_dict()`` of one model with the reference's seven groups, from its moment views."""
    defaults = _group_defaults(betas, eps)
    groups, state = [], {}
    for gi, g in enumerate(GROUPS):
        groups.append(dict(defaults, lr=lrs[g], name=g, params=[gi]))
        if steps[g] > 0:
            m, v = views[g]
            state[gi] = {"step": torch.tensor(float(steps[g]), dtype=torch.float32), "exp_avg": m.clone(),
                         "exp_avg_sq": v.clone()}
    return {"state": state, "param_groups": groups}


def load_adam_state_dict(views, steps: Dict[str, int], lrs: Dict[str, float], sd: dict, betas, eps) -> None:
    """Inverse of adam_state_dict: copies the moments into ``views`` and sets ``steps`` / ``lrs`` in place."""
    groups = sd["param_groups"]
    if len(groups) != len(GROUPS):
        raise ValueError(f"load_model_state_dict: expected {len(GROUPS)} param groups, got {len(groups)}")
    for gi, (g, pg) in enumerate(zip(GROUPS, groups)):
        if pg.get("name", g) != g:
            raise ValueError(f"load_model_state_dict: param group {gi} is {pg.get('name')!r}, expected {g!r}")
        if len(pg["params"]) != 1:
            raise ValueError(f"load_model_state_dict: group {g!r} must hold one parameter")
        if tuple(float(b) for b in pg.get("betas", betas)) != tuple(betas) or float(pg.get("eps", eps)) != eps:
            raise ValueError(f"load_model_state_dict: group {g!r} has betas / eps {pg.get('betas')} / {pg.get('eps')}, "
                             f"this optimiser {tuple(betas)} / {eps}")
        for name, default in (("weight_decay", 0), ("amsgrad", False), ("maximize", False)):
            if pg.get(name, default) != default:
                raise NotImplementedError(f"load_model_state_dict: {name}={pg[name]!r} is not implemented")
    for gi, (g, pg) in enumerate(zip(GROUPS, groups)):
        st = sd["state"].get(pg["params"][0])
        m, v = views[g]
        if st is None:
            m.zero_()
            v.zero_()
            step = 0
        else:
            for dst, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
                src = st[key]
                if src.numel() != dst.numel():
                    raise ValueError(f"load_model_state_dict: {g}.{key} has {src.numel()} elements, the model "
                                     f"{dst.numel()}")
                dst.copy_(src.detach().to(device=dst.device, dtype=torch.float32).reshape(dst.shape))
            step = int(float(st["step"]))
        lrs[g] = float(pg["lr"])
        steps[g] = step


class AdamSink:
    """One frame's Adam step, planned by ``SegmentedAdam.sink`` and applied by the backward of
    ``FlatScene.compose(grad_sink=...)`` (include/sgr_scene_step.h).  ``segments``: the sorted persistent indices of the
    frame; ``plan``: {(segment, group): (step_size, bc2_sqrt)} as float32, for step count + 1; ``eps``: float32.
    ``consumed`` turns True when the backward has applied the plan (on ``stream``, the stream it ran on); the step
    counts advance when ``SegmentedAdam.step`` commits it."""

    def __init__(self, opt: "SegmentedAdam", segments: List[int], plan: dict):
        self.opt = opt
        self.segments = list(segments)
        self.plan = plan
        self.eps = np.float32(opt.eps)
        self.consumed = False
        self.stream = None

    @property
    def armed(self) -> bool:
        return self.opt._sink is self

    def discard(self) -> None:
        """Drops an armed plan whose backward has not run: nothing was stepped, no count advances.  A consumed sink
        cannot be discarded -- the parameters have moved -- and raises RuntimeError: commit it with ``step``."""
        if self.consumed:
            raise RuntimeError("AdamSink.discard: the backward has already applied this step; commit it with "
                               "SegmentedAdam.step(segments)")
        if self.armed:
            self.opt._sink = None


class SegmentedAdam:
    """One Adam per segment of ``flat`` (seven named groups each), stepped in one launch.

    ``lrs``: one dict per segment keyed by ``GROUPS``.  ``self.lrs[seg][group]`` and ``self.steps[seg][group]`` are
    mutable (the reference's ``update_learning_rate`` sets the ``xyz`` lr of every model each iteration).  The moments
    are flat tensors shaped like the flat leaves (``self.exp_avg[attr]``, ``self.exp_avg_sq[attr]``)."""

    def __init__(self, flat, lrs: Sequence[Dict[str, float]], betas=(0.9, 0.999), eps: float = 1e-15,
                 weight_decay: float = 0, amsgrad: bool = False, *, maximize: bool = False, capturable: bool = False):
        for name, val, default in (("weight_decay", weight_decay, 0), ("amsgrad", amsgrad, False),
                                   ("maximize", maximize, False), ("capturable", capturable, False)):
            if val != default:
                raise NotImplementedError(f"SegmentedAdam: {name}={val!r} is not implemented (the reference uses "
                                          f"{name}={default!r})")
        beta1, beta2 = float(betas[0]), float(betas[1])
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"SegmentedAdam: betas must lie in [0, 1), got {betas}")
        if not eps >= 0.0:
            raise ValueError(f"SegmentedAdam: invalid eps {eps}")
        self.betas = (beta1, beta2)
        self.eps = float(eps)
        self._check_flat(flat)
        if len(lrs) != len(flat.meta):
            raise ValueError(f"SegmentedAdam: {len(flat.meta)} segments but {len(lrs)} lr dicts")
        self.lrs = [self._check_lrs(d, i) for i, d in enumerate(lrs)]
        self.steps = [{g: 0 for g in GROUPS} for _ in flat.meta]
        self.flat = flat
        self.exp_avg = {a: torch.zeros_like(t, memory_format=torch.contiguous_format) for a, t in flat.tensors.items()}
        self.exp_avg_sq = {a: torch.zeros_like(t, memory_format=torch.contiguous_format) for a, t in flat.tensors.items()}
        self._sink = None
        self._relayout()

    # ---- checks ------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_flat(flat):
        dev = flat.xyz.device
        for a in (ATTR[g] for g in GROUPS):
            t = flat.tensors[a]
            require_hip("SegmentedAdam needs HIP (cuda) tensors: there is no CPU path", t)
            if t.device != dev:
                raise ValueError("SegmentedAdam: every flat leaf must be on the same device")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"SegmentedAdam: flat.{a} must be a contiguous float32 tensor")

    @staticmethod
    def _check_lrs(d, i):
        missing = [g for g in GROUPS if g not in d]
        extra = [k for k in d if k not in GROUPS]
        if missing or extra:
            raise ValueError(f"SegmentedAdam: lrs[{i}] must have exactly the groups {GROUPS} "
                             f"(missing {missing}, unknown {extra})")
        return {g: float(d[g]) for g in GROUPS}

    # ---- layout --------------------------------------------------------------------------------------------------
    def _relayout(self):
        self.layout = segment_layout(self.flat.meta, _rest_width(self.flat))
        self._span = int(_native.lib().sgr_adam_span_elems())
        self._max_records = int(_native.lib().sgr_adam_max_records())
        self._chunks_dev = None
        self._chunks_key = None
        self._bc = {}

    def _chunk_table(self):
        """Device table of every (segment, group) chunk; rebuilt when a pointer changes."""
        ptr = lambda d: {g: d[ATTR[g]].data_ptr() for g in GROUPS}
        p, m, v = ptr(self.flat.tensors), ptr(self.exp_avg), ptr(self.exp_avg_sq)
        key = tuple(p.values()) + tuple(m.values()) + tuple(v.values())
        if self._chunks_dev is None or key != self._chunks_key:
            self._chunks_dev = _pinned_to(chunk_table(self.layout, p, m, v), self.flat.xyz.device)
            self._chunks_key = key
        return self._chunks_dev

    # ---- the step inside the compose backward ------------------------------------------------------------------------
    def sink(self, segments: Optional[Sequence[int]] = None) -> AdamSink:
        """Plans this frame's step for ``FlatScene.compose(..., grad_sink=)`` (host only, nothing is launched and no count
        advances): per (segment, group) of ``segments`` (None = all) the scalars ``step`` would use now -- step count
        + 1 and the CURRENT ``lrs``, so call it after the iteration's learning-rate update (the reference updates them
        at the top of the iteration, train.py:67).  A group whose flat leaf has ``requires_grad == False`` is left out.

        The contract of the armed sink:
          * the backward of that ``compose`` applies the step: the seven flat leaves and the moments CHANGE during
            ``loss.backward()``, and the leaves get no ``.grad``;
          * ``compose`` must be the only autograd consumer of the seven leaves in that graph: a regulariser computed
            directly on a leaf would read it in an undefined order relative to the step and lose its gradient;
          * one backward per sink (a second one raises RuntimeError); ``step(segments)`` with the same segments then
            commits it: it launches nothing and advances exactly the planned step counts;
          * not for use with the ``multiview`` reducers, which need the gradients;
          * moments, ``state_views``, ``model_state_dict`` and ``densify_scene(moments=...)`` work unchanged.

        Raises RuntimeError while another sink is armed, and when the library's lazy forward is on (``sgr_set_lazy``): a
        lazy frame that is found invalid one call late must be discarded, and a step already applied cannot be."""
        if self._sink is not None:
            raise RuntimeError("SegmentedAdam.sink: another sink is still armed (commit it with step(segments) or drop it "
                               "with its discard())")
        if int(_native.lib().sgr_set_lazy(-1)) == 1:
            raise RuntimeError("SegmentedAdam.sink: the lazy forward is on (sgr_set_lazy): a lazy frame found invalid one "
                               "call late must be discarded, and a step applied inside the backward cannot be")
        groups = [g for g in GROUPS if self.flat.tensors[ATTR[g]].requires_grad]
        segs = _segment_set(segments, len(self.layout), "SegmentedAdam.sink")
        plan = plan_sink(self.layout, self.steps, self.lrs, segs, groups, self.betas, bc_cache=self._bc)
        self._sink = AdamSink(self, segs, plan)
        return self._sink

    def _refuse_armed(self, who: str) -> None:
        if self._sink is not None:
            raise RuntimeError(f"SegmentedAdam.{who}: a sink is armed (commit it with step(segments) or drop it with its "
                               "discard())")

    def _commit_sink(self, segments) -> bool:
        """True when an armed, consumed sink was committed (the step has been applied by the backward already)."""
        sink = self._sink
        if sink is None:
            return False
        if not sink.consumed:  # no output had an upstream gradient: the backward never ran, nothing was stepped
            self._sink = None
            return False
        if _segment_set(segments, len(self.layout), "SegmentedAdam.step") != sink.segments:
            raise ValueError(f"SegmentedAdam.step: segments {segments} do not match the consumed sink's {sink.segments}")
        stray = [ATTR[g] for g in GROUPS if self.flat.tensors[ATTR[g]].grad is not None]
        if stray:
            raise ValueError(f"SegmentedAdam.step: the sink has stepped this frame, but {stray} carry a .grad: a mixed "
                             "step (another autograd consumer of the leaves?); nothing changes")
        for s, g in sink.plan:
            self.steps[s][g] += 1
        self._sink = None
        return True

    # ---- the step ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, segments: Optional[Sequence[int]] = None) -> None:
        """One Adam step of the segments in ``segments`` (indices into ``flat.meta``; None = every segment), on the
        current stream, without a host synchronisation.  A group whose flat leaf has ``.grad is None`` is skipped for
        every segment; a skipped (segment, group) keeps its bytes and its step count.  Set the leaves' ``.grad`` to
        None afterwards, as the reference's ``zero_grad(set_to_none=True)`` does.  One step takes at most
        sgr_adam_max_records() (4096) non-empty (segment, group) blocks, 585 models with all seven: more is refused with
        an SgrError before anything changes, and the caller steps the segments in several calls.

        After a backward into this optimiser's ``sink()``, the step has been applied already: this call launches
        nothing, checks that ``segments`` is the sink's set and that no leaf carries a ``.grad`` (ValueError, nothing
        changes), advances the planned step counts and disarms.  An armed sink whose backward never ran is dropped
        and the call behaves as without one."""
        if self._commit_sink(segments):
            return
        grads = {}
        for g in GROUPS:
            leaf = self.flat.tensors[ATTR[g]]
            gt = leaf.grad
            if gt is None:
                continue
            if gt.layout != torch.strided:
                raise NotImplementedError(f"SegmentedAdam: sparse gradients ({ATTR[g]}) are not implemented")
            if gt.dtype != torch.float32 or gt.shape != leaf.shape or gt.device != leaf.device:
                raise ValueError(f"SegmentedAdam: flat.{ATTR[g]}.grad must be float32 and shaped like the leaf")
            grads[g] = gt if gt.is_contiguous() else gt.contiguous()
        rec, n_spans = plan_step(self.layout, self.steps, self.lrs, segments, {g: t.data_ptr() for g, t in grads.items()},
                                 self.betas, self.eps, self._span, bc_cache=self._bc, max_records=self._max_records)
        if n_spans == 0:
            return
        dev = self.flat.xyz.device
        with torch.cuda.device(dev):  # the pinned staging buffers of the two tables are allocated with dev current
            chunks = self._chunk_table()
            recs = _pinned_to(rec, dev)
            launch("sgr_adam_step", _native.stream(dev), chunks, len(self.layout) * len(GROUPS), recs, len(rec), n_spans,
                   self.betas[0], self.betas[1])
        # the contiguous copies of strided gradients and the tables are freed on this stream: reused only after the launch

    # ---- state ---------------------------------------------------------------------------------------------------
    def state_views(self, seg: int) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """{group: (exp_avg, exp_avg_sq)} of segment ``seg``, views of the flat moments shaped like its parameters
        (what ``densify.densify_and_prune(states=...)`` and ``densify.reset_opacity(..., state)`` take)."""
        out = {}
        for g in GROUPS:
            off, cnt, shape = self.layout[seg][g]
            a = ATTR[g]
            out[g] = tuple(t[a].reshape(-1)[off:off + cnt].view(shape) for t in (self.exp_avg, self.exp_avg_sq))
        return out

    def model_state_dict(self, seg: int) -> dict:
        """Segment ``seg``'s optimiser in ``torch.optim.Adam.state_dict()``'s layout, as the reference saves it under
        'optimizer' (gaussian_model.py:178-200): seven param groups in the reference's order, state (copies) for every
        group that has taken a step."""
        return adam_state_dict(self.state_views(seg), self.steps[seg], self.lrs[seg], self.betas, self.eps)

    def load_model_state_dict(self, seg: int, sd: dict) -> None:
        """Restores segment ``seg`` from a ``torch.optim.Adam.state_dict()`` over the reference's seven groups: learning
        rates, step counts and moments (a group without state gets step 0 and zero moments)."""
        self._refuse_armed("load_model_state_dict")
        load_adam_state_dict(self.state_views(seg), self.steps[seg], self.lrs[seg], sd, self.betas, self.eps)

    def rebuild(self, new_flat, states: Sequence[Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]]) -> None:
        """Re-lays the moments for ``new_flat`` (same segments, new counts: a ``FlatScene`` rebuilt from the per-model
        results of ``densify_and_prune``).  ``states[i]`` is segment i's new ``{group: (exp_avg, exp_avg_sq)}`` (the
        ``new_states`` of its densify call), or None to keep its current moments (its counts must be unchanged).
        Learning rates and step counts carry over per segment, as cat_optimizer / prune_optimizer keep them."""
        self._refuse_armed("rebuild")
        if len(new_flat.meta) != len(self.layout):
            raise ValueError(f"rebuild: {len(self.layout)} segments before, {len(new_flat.meta)} after")
        if len(states) != len(self.layout):
            raise ValueError(f"rebuild: need one state entry (or None) per segment, got {len(states)}")
        self._check_flat(new_flat)
        new_layout = segment_layout(new_flat.meta, _rest_width(new_flat))
        ea = {a: torch.zeros_like(t, memory_format=torch.contiguous_format) for a, t in new_flat.tensors.items()}
        eas = {a: torch.zeros_like(t, memory_format=torch.contiguous_format) for a, t in new_flat.tensors.items()}
        with torch.no_grad():
            for s, (lay, st) in enumerate(zip(new_layout, states)):
                src = self.state_views(s) if st is None else st
                for g in GROUPS:
                    off, cnt, _ = lay[g]
                    if g not in src:
                        raise ValueError(f"rebuild: segment {s} has no state for {g!r}")
                    for dst, t in zip((ea, eas), src[g]):
                        if t.numel() != cnt:
                            raise ValueError(f"rebuild: segment {s} {g}: {t.numel()} moment elements for {cnt} parameters")
                        if cnt:
                            dst[ATTR[g]].reshape(-1)[off:off + cnt].copy_(t.detach().reshape(-1))
        self.flat, self.exp_avg, self.exp_avg_sq = new_flat, ea, eas
        self._relayout()

    def rebuild_flat(self, new_flat, new_moments) -> None:
        """Adopts ``densify.densify_scene``'s results without a copy: ``new_moments`` = ``(exp_avg, exp_avg_sq)``, dicts
        keyed by flat attribute and shaped like ``new_flat``'s leaves, become this optimiser's moments.  Learning rates and
        step counts carry over per segment, as ``rebuild`` keeps them."""
        self._refuse_armed("rebuild_flat")
        if len(new_flat.meta) != len(self.layout):
            raise ValueError(f"rebuild_flat: {len(self.layout)} segments before, {len(new_flat.meta)} after")
        self._check_flat(new_flat)
        if len(new_moments) != 2:
            raise ValueError("rebuild_flat: new_moments = (exp_avg, exp_avg_sq)")
        for d in new_moments:
            for a, t in new_flat.tensors.items():
                m = d.get(a)
                if m is None or m.shape != t.shape or m.dtype != torch.float32 or m.device != t.device or not m.is_contiguous():
                    raise ValueError(f"rebuild_flat: the moments of {a} must be a contiguous float32 tensor shaped like the leaf")
        self.flat = new_flat
        self.exp_avg, self.exp_avg_sq = ({a: d[a] for a in new_flat.tensors} for d in new_moments)
        self._relayout()
