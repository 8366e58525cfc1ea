#!/usr/bin/env python
"""Measurement of the per-frame actor poses (street_gaussians_amd/actor_pose.py) on one MI355X: K = 20 actors in a
tracklet table of F = 200 frames, tracking optimised, forward + backward of sum(poses * g) per call.

  reference_way   the torch restatement (tests/torch_ref_actor_pose.py) driven as the reference drives ActorPose
                  (lib/models/actor_pose.py:83-173, street_gaussian_model.py:254-265): per actor, track_idx on the device,
                  `.cpu()` reads for the index choice and the timestamps, once for the translation and once for the rotation
  actor_poses     ActorPoses.plan + poses + backward, with a new plan per call (host planning and one small copy) and with
                  a cached plan (`key=`)

Wall time is host time per call with a device synchronisation at the end of the timed block (what the training loop
pays before it can issue the rasterizer); launches are the device kernels per call counted by torch.profiler.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_ref_actor_pose as rp  # noqa: E402
from street_gaussians_amd.actor_pose import ActorPoses  # noqa: E402

dev = torch.device("cuda")
K, F = 20, 200


def scene(seed=0):
    rng = np.random.default_rng(seed)
    ids = np.full((F, K), -1, np.int64)
    for k in range(K):  # actor k lives in frames [start, end), in a column that changes along the way
        start = int(rng.integers(0, F // 4))
        for f in range(start, F - int(rng.integers(0, F // 4))):
            ids[f, (k + f // 50) % K] = k
    stamps = 1.5e9 + 0.1 * np.arange(F)
    q = rng.standard_normal((F, K, 4))
    q /= np.sqrt((q * q).sum(-1, keepdims=True))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    info = {k: dict(start_timestamp=stamps[np.nonzero((ids == k).any(1))[0][0]],
                    end_timestamp=stamps[np.nonzero((ids == k).any(1))[0][-1]]) for k in range(K)}
    return dict(track_ids=torch.from_numpy(ids).to(dev), input_trans=t(10 * rng.standard_normal((F, K, 3))), input_rots=t(q),
                stamps=stamps, info=info, opt_trans=torch.nn.Parameter(t(0.05 * rng.standard_normal((F, K, 3)))),
                opt_rots=torch.nn.Parameter(t(0.1 * rng.standard_normal((F, K, 1)))),
                ego=t(np.eye(4)), g=t(rng.standard_normal((K, 7))))


def reference_way(sc, track_idx, timestamp):
    """One frame the reference's way; -> [K, 7]."""
    stamps, out = sc["stamps"], []

    def closest(k):  # find_closest_indices: a device-to-host read per call
        tidx = track_idx[k]
        frame_ts = np.array(stamps[tidx[:, 0].cpu()])
        i1, i2 = np.argsort(np.abs(frame_ts - timestamp))[:2]
        return tidx[i1], tidx[i2]

    E = sc["ego"]
    for k in range(K):
        # get_tracking_rotation_
        ind1, ind2 = closest(k)
        t1, t2 = stamps[ind1[0].cpu()], stamps[ind2[0].cpu()]
        qa = rp.mul_theta_cs(sc["input_rots"][ind1[0], ind1[1]], torch.cos(sc["opt_rots"][ind1[0], ind1[1]]),
                             torch.sin(sc["opt_rots"][ind1[0], ind1[1]]))
        th2 = sc["opt_rots"][ind1[0], ind2[1]]
        qb = rp.mul_theta_cs(qa, torch.cos(th2), torch.sin(th2))
        r = torch.tensor([(timestamp - t1) / (t2 - t1)], device=dev).float()
        Q = rp.slerp(qa.reshape(1, 4), qb.reshape(1, 4), r)
        # get_tracking_translation_
        ind1, ind2 = closest(k)
        t1, t2 = stamps[ind1[0].cpu()], stamps[ind2[0].cpu()]
        ta = sc["input_trans"][ind1[0], ind1[1]] + sc["opt_trans"][ind1[0], ind1[1]]
        tb = sc["input_trans"][ind2[0], ind2[1]] + sc["opt_trans"][ind2[0], ind2[1]]
        T = (ta * (t2 - timestamp) + tb * (timestamp - t1)) / (t2 - t1)
        # parse_camera
        qe = rp.matrix_to_quaternion(E[:3, :3])
        out.append(torch.cat([rp.qmul(qe.reshape(1, 4), Q).reshape(4), E[:3, :3] @ T + E[:3, 3]]))
    return torch.stack(out)


def wall_ms(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n if n else "not measured: the profiler recorded no device kernels"
    except Exception as e:  # a profiler that cannot trace this device is not a reason to lose the timings
        return f"not measured: {type(e).__name__}: {e}"


if __name__ == "__main__":
    sc = scene()
    ap = ActorPoses(sc["track_ids"], sc["input_trans"], sc["input_rots"], sc["stamps"], {}, sc["info"],
                    opt_trans=sc["opt_trans"], opt_rots=sc["opt_rots"])
    track_idx = [torch.argwhere(sc["track_ids"] == k) for k in range(K)]
    frame = F // 2
    timestamp = float(sc["stamps"][frame] + 0.03)
    ids = list(range(K))

    def zero():
        sc["opt_trans"].grad = sc["opt_rots"].grad = None

    def ref():
        zero()
        (reference_way(sc, track_idx, timestamp) * sc["g"]).sum().backward()

    def ours(key):
        zero()
        ap.poses(ap.plan(ids, timestamp, 0, key=key), sc["ego"]).backward(sc["g"])

    a = reference_way(sc, track_idx, timestamp).detach()
    b = ap.poses(ap.plan(ids, timestamp, 0), sc["ego"]).detach()
    res = {"what": f"actor poses of one frame, K = {K} actors, F = {F} frames, opt_track, forward + backward",
           "device": torch.cuda.get_device_name(0), "max_abs_difference": float((a - b).abs().max()),
           "reference_way": {"wall_ms": round(wall_ms(ref, n=5, warm=1), 3), "launches": launches(ref)},
           "actor_poses_uncached_plan": {"wall_ms": round(wall_ms(lambda: ours(None)), 4), "launches": launches(lambda: ours(None))},
           "actor_poses_cached_plan": {"wall_ms": round(wall_ms(lambda: ours("cam")), 4), "launches": launches(lambda: ours("cam"))}}
    print(json.dumps(res))
