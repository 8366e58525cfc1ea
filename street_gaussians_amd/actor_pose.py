"""The producer of ``FlatScene.compose(poses=)``: every actor's world pose of a frame, what the reference's
``parse_camera`` (lib/models/street_gaussian_model.py:254-265) computes per actor through ``ActorPose``
(lib/models/actor_pose.py:83-173), as one HIP launch (csrc/sgr_actor_pose.hip, include/sgr_actor_pose.h) with an autograd
backward to ``opt_trans`` / ``opt_rots``.

Everything the reference fetches from the device per actor and per iteration -- ``track_idx``, the tracklet timestamps, the
camera timestamps -- is known on the host at construction, so the index choice and the interpolation weights are made in
numpy (``plan``), in float64 exactly as the reference makes them, and only the differentiable arithmetic runs on the GPU
(``poses``).  After construction nothing here waits on the device.

``plan`` runs anywhere; ``poses`` needs the tensors on the GPU: there is no CPU implementation in the product."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Hashable, Optional, Sequence

import numpy as np
import torch

from ._native import call, require_hip

CONTRIB, PARTS = 16, 23  # include/sgr_actor_pose.h SGR_ACTOR_POSE_CONTRIB / _PARTS


class _CSample(C.Structure):  # sgr_actor_pose_sample
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("th1", C.c_int32), ("th2", C.c_int32),
                ("wa", C.c_float), ("wb", C.c_float), ("wd", C.c_float), ("r", C.c_float)]


class _CRecord(C.Structure):  # sgr_actor_pose_record
    _fields_ = [("s", _CSample * 2), ("Wa", C.c_float), ("Wb", C.c_float), ("Wd", C.c_float), ("R", C.c_float),
                ("n_samples", C.c_int32), ("pad", C.c_int32 * 3)]


RECORD_DTYPE = np.dtype(_CRecord)
assert C.sizeof(_CSample) == 32 and C.sizeof(_CRecord) == 96 and RECORD_DTYPE.itemsize == 96


def closest_two(stamps: np.ndarray, t):
    """``find_closest_indices`` / ``find_closest_camera_timestamps`` (actor_pose.py:88-89, :103-104): positions of the
    closest and the second closest of ``stamps`` to ``t``, ties as numpy's default sort leaves them."""
    idx1, idx2 = np.argsort(np.abs(stamps - t))[:2]
    return int(idx1), int(idx2)


class Plan:
    """The host plan of one frame: ``records`` (K x sgr_actor_pose_record, numpy) and, once ``poses`` has used it on a
    device, its copy there.  ``copies`` counts the host-to-device copies made for this plan."""

    def __init__(self, records: np.ndarray, signature):
        self.records = records
        self.signature = signature
        self.copies = 0
        self._device: Dict[torch.device, torch.Tensor] = {}

    def __len__(self):
        return int(self.records.shape[0])

    def cells(self) -> np.ndarray:
        """[K, 2, 4] int: (a, b, th1, th2) of both samples (the second repeats the first where n_samples = 1)."""
        s = self.records["s"]
        out = np.stack([s["a"], s["b"], s["th1"], s["th2"]], axis=-1).astype(np.int64)
        one = self.records["n_samples"] == 1
        out[one, 1] = out[one, 0]
        return out

    def on(self, dev: torch.device) -> torch.Tensor:
        """The records on ``dev``: built in pinned memory and copied on the current stream without blocking, once."""
        t = self._device.get(dev)
        if t is None:
            raw = self.records.view(np.uint8).reshape(-1)
            host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
            host.numpy()[:] = raw
            t = host.to(dev, non_blocking=True)
            self._device[dev] = t
            self.copies += 1
        return t


class _Poses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opt_trans, opt_rots, owner, recs, K, ego):
        ctx.owner, ctx.recs, ctx.K, ctx.ego = owner, recs, K, ego
        ctx.save_for_backward(opt_trans, opt_rots)
        return owner._forward(recs, K, ego, opt_trans, opt_rots)[0]

    @staticmethod
    def backward(ctx, dposes):
        opt_trans, opt_rots = ctx.saved_tensors
        o, K = ctx.owner, ctx.K
        dev = opt_trans.device
        g = dposes.to(torch.float32).contiguous()
        d_trans = torch.empty_like(opt_trans, memory_format=torch.contiguous_format)
        d_rots = torch.empty_like(opt_rots, memory_format=torch.contiguous_format)
        contrib = torch.empty(K * CONTRIB, dtype=torch.float32, device=dev)
        call("sgr_actor_pose_backward", dev, K, ctx.recs, o.n_cells, o.input_trans, o.input_rots, opt_trans, opt_rots,
             ctx.ego, g, contrib, d_trans, d_rots)
        return d_trans, d_rots, None, None, None, None


class ActorPoses:
    """``ActorPoses(track_ids [F, O], input_trans [F, O, 3], input_rots [F, O, 4] (w, x, y, z), timestamps [F],
    camera_timestamps {cam: {'train_timestamps': [...]}}, obj_info {track_id: {'start_timestamp', 'end_timestamp'}},
    opt_trans=None, opt_rots=None)``: the tracklet table of ``ActorPose.__init__``.  ``opt_trans`` [F, O, 3] and
    ``opt_rots`` [F, O, 1] are given together and mean that tracking is optimised (the reference's ``opt_track``); they
    are kept as the objects they are, so an optimiser or a ``state_dict`` that holds them goes on working.

    Construction may wait on the device once (``track_ids`` comes to the host); ``plan`` and ``poses`` never do."""

    def __init__(self, track_ids, input_trans, input_rots, timestamps, camera_timestamps, obj_info, opt_trans=None,
                 opt_rots=None):
        if (opt_trans is None) != (opt_rots is None):
            raise ValueError("ActorPoses: opt_trans and opt_rots are given together (opt_track) or not at all")
        F, O = (int(x) for x in track_ids.shape)
        for name, t, shape in (("input_trans", input_trans, (F, O, 3)), ("input_rots", input_rots, (F, O, 4)),
                               ("opt_trans", opt_trans, (F, O, 3)), ("opt_rots", opt_rots, (F, O, 1))):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise ValueError(f"ActorPoses: {name} must be a float32 tensor of shape {list(shape)}")
            if not t.is_contiguous():
                raise ValueError(f"ActorPoses: {name} must be contiguous")
        self.F, self.O, self.n_cells = F, O, F * O
        self.input_trans, self.input_rots = input_trans.detach(), input_rots.detach()
        self.opt_trans, self.opt_rots = opt_trans, opt_rots
        self.opt_track = opt_trans is not None
        self.timestamps = np.asarray(timestamps)
        if self.timestamps.shape != (F,):
            raise ValueError(f"ActorPoses: {F} frames but timestamps of shape {list(self.timestamps.shape)}")
        self.camera_timestamps = camera_timestamps
        ids = track_ids.detach().cpu().numpy() if isinstance(track_ids, torch.Tensor) else np.asarray(track_ids)  # the one sync
        # torch.argwhere(self.track_ids == track_id) (actor_pose.py:30): rows (frame, column) in row-major order
        self._tracks = {tid: (np.argwhere(ids == tid), float(info["start_timestamp"]), float(info["end_timestamp"]))
                        for tid, info in obj_info.items()}
        self._plans: Dict[Hashable, Plan] = {}

    @classmethod
    def from_reference(cls, actor_pose) -> "ActorPoses":
        """From the reference's ``ActorPose`` module: its ``input_trans`` / ``input_rots`` (constants; slices of the
        tracklet table there, so made contiguous here) and, with ``opt_track``, its very ``opt_trans`` / ``opt_rots``
        Parameters."""
        opt = bool(actor_pose.opt_track)
        return cls(actor_pose.track_ids, actor_pose.input_trans.contiguous(), actor_pose.input_rots.contiguous(),
                   actor_pose.timestamps, actor_pose.camera_timestamps, actor_pose.obj_info,
                   opt_trans=actor_pose.opt_trans if opt else None, opt_rots=actor_pose.opt_rots if opt else None)

    # ---- host ---------------------------------------------------------------------------------------------------------
    def _sample(self, rec_s, rows, stamps, t):
        """One sample of actor_pose.py:107-122 / :138-158 at time ``t``: the cells and the float64 weights, rounded to
        float32 by the assignment into the record."""
        idx1, idx2 = closest_two(stamps, t)
        (f1, c1), (f2, c2) = rows[idx1], rows[idx2]
        t1, t2 = self.timestamps[f1], self.timestamps[f2]
        with np.errstate(divide="ignore", invalid="ignore"):
            rec_s["wa"], rec_s["wb"], rec_s["wd"], rec_s["r"] = t2 - t, t - t1, t2 - t1, (t - t1) / (t2 - t1)
        rec_s["a"], rec_s["b"] = f1 * self.O + c1, f2 * self.O + c2
        rec_s["th1"], rec_s["th2"] = f1 * self.O + c1, f1 * self.O + c2  # (frame_ind1, column_ind2): actor_pose.py:148

    def plan(self, track_ids: Sequence, timestamp, cam=None, is_val: bool = False, key: Optional[Hashable] = None) -> Plan:
        """The frame's plan: one record per ``track_ids`` entry, in that order.  Host only.  With ``key`` the plan is kept
        and returned again (with its device copy) as long as the other arguments are the same."""
        track_ids = list(track_ids)
        signature = (tuple(track_ids), timestamp, cam, bool(is_val))
        if key is not None:
            hit = self._plans.get(key)
            if hit is not None and hit.signature == signature:
                return hit
        recs = np.zeros(len(track_ids), dtype=RECORD_DTYPE)
        for k, tid in enumerate(track_ids):
            if tid not in self._tracks:
                raise ValueError(f"ActorPoses.plan: track_id {tid!r} is not in obj_info")
            rows, start, end = self._tracks[tid]
            if len(rows) < 2:
                raise ValueError(f"ActorPoses.plan: track_id {tid!r} has {len(rows)} tracklet entries, two are needed")
            stamps = np.array(self.timestamps[rows[:, 0]])
            rec = recs[k]
            rec["n_samples"] = 1
            outer = None
            if self.opt_track and is_val:  # actor_pose.py:93-105
                cts = np.array([x for x in self.camera_timestamps[cam]["train_timestamps"] if x >= start and x <= end])
                if len(cts) >= 2:
                    i1, i2 = closest_two(cts, timestamp)
                    outer = (cts[i1], cts[i2])
            if outer is None:
                self._sample(rec["s"][0], rows, stamps, timestamp)
            else:
                T1, T2 = outer
                self._sample(rec["s"][0], rows, stamps, T1)
                self._sample(rec["s"][1], rows, stamps, T2)
                rec["n_samples"] = 2
                with np.errstate(divide="ignore", invalid="ignore"):
                    rec["Wa"], rec["Wb"], rec["Wd"], rec["R"] = T2 - timestamp, timestamp - T1, T2 - T1, \
                        (timestamp - T1) / (T2 - T1)
        plan = Plan(recs, signature)
        if key is not None:
            self._plans[key] = plan
        return plan

    # ---- device -------------------------------------------------------------------------------------------------------
    def _forward(self, recs, K, ego, opt_trans, opt_rots, parts: bool = False):
        dev = self.input_trans.device
        out = torch.empty(K, 7, dtype=torch.float32, device=dev)
        pt = torch.empty(K, PARTS, dtype=torch.float32, device=dev) if parts else None
        call("sgr_actor_pose_forward", dev, K, recs, self.n_cells, self.input_trans, self.input_rots, opt_trans, opt_rots,
             ego, out, pt)
        return out, pt

    def _check_device(self, ego_pose):
        ts = [self.input_trans, self.input_rots, ego_pose] + ([self.opt_trans, self.opt_rots] if self.opt_track else [])
        require_hip("ActorPoses.poses: every tensor must be a HIP (cuda) tensor: there is no CPU path", *ts)
        if any(t.device != ts[0].device for t in ts):
            raise ValueError("ActorPoses.poses: every tensor must be on the same device")

    def poses(self, plan: Plan, ego_pose: torch.Tensor) -> torch.Tensor:
        """[K, 7] (obj_rot w, x, y, z, then obj_trans; world space; the plan's order) on the device.  ``ego_pose`` is the
        camera's [4, 4] float32 ego pose, read on the device.  With optimised tracking the result carries the graph to
        ``opt_trans`` and ``opt_rots`` (dense gradients, every element written); ``ego_pose`` gets no gradient."""
        if not isinstance(ego_pose, torch.Tensor) or ego_pose.dtype != torch.float32 or tuple(ego_pose.shape) != (4, 4):
            raise ValueError("ActorPoses.poses: ego_pose must be a float32 tensor of shape [4, 4]")
        self._check_device(ego_pose)
        K = len(plan)
        dev = self.input_trans.device
        if K == 0:
            return torch.empty(0, 7, dtype=torch.float32, device=dev)
        recs = plan.on(dev)
        ego = ego_pose.detach().contiguous()
        if not self.opt_track:
            return self._forward(recs, K, ego, None, None)[0]
        if not (self.opt_trans.is_contiguous() and self.opt_rots.is_contiguous()):
            raise ValueError("ActorPoses.poses: opt_trans and opt_rots must be contiguous")
        return _Poses.apply(self.opt_trans, self.opt_rots, self, recs, K, ego)
