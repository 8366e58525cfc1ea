#!/usr/bin/env python
"""Measurement of the SegmentedAdam sink (include/sgr_scene_step.h) on one MI355X: the compose backward + optimiser
slice of a flat-mode training iteration, with the Adam step as a launch of its own against the step applied inside
the compose backward.

Workload: flat mode, a background plus 20 actors x 10 k Gaussians, SH degree 3, 19 classes, 12 of the 20 actors in the
frame, at 1.8 M and at 5 M background Gaussians; the loss is a fixed random linear functional of the compose outputs,
so no rasterizer is in the window.  Two legs, timed with device events, alternating in one process after both are warm:

  (a) compose forward + backward + opt.step(segments) + .grad = None
  (b) opt.sink(segments) + compose(grad_sink=) forward + backward + opt.step(segments)

    python tools/bench_scene_step.py [--sizes 1800000 5000000] [--reps 30] [--leg both|a|b] [--out profiles/scene_step/bench.json]

`--leg a` / `--leg b` runs one leg alone (for a kernel trace of that leg).  Prints one JSON line and writes it to --out:
per size and leg the median and the 5-95 % width in ms, and whether the sink wins at that size -- (b)'s median below
(a)'s by more than (a)'s 5-95 % width."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from street_gaussians_amd import scene  # noqa: E402
from street_gaussians_amd.optim import GROUPS, SegmentedAdam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1_800_000, 5_000_000])
ap.add_argument("--actors", type=int, default=20)
ap.add_argument("--actor-gaussians", type=int, default=10_000)
ap.add_argument("--present", type=int, default=12)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--leg", choices=["both", "a", "b"], default="both")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_step", "bench.json"))
args = ap.parse_args()
M, S, C = 16, 19, 5
dev = torch.device("cuda")
gen = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)


def make_flat(n_bg):
    counts = [n_bg] + [args.actor_gaussians] * args.actors
    segs = []
    for k, n in enumerate(counts):
        d = dict(xyz=rnd(n, 3), rotation=rnd(n, 4), scaling=rnd(n, 3) * 0.3, opacity=rnd(n, 1),
                 features_rest=rnd(n, M - 1, 3))
        if k == 0:
            d.update(features_dc=rnd(n, 1, 3), semantic=rnd(n, S))
        else:
            d.update(features_dc=rnd(n, C, 3), semantic=rnd(n, 1), pose=rnd(7), idft=rnd(C), class_label=k % S)
        segs.append(scene.Segment(**d))
    return scene.FlatScene.from_segments(segs)


def measure(n_bg):
    flat = make_flat(n_bg)
    K = len(flat.meta)
    opt = SegmentedAdam(flat, [{g: 1e-5 for g in GROUPS} for _ in range(K)])
    present = [0] + list(range(1, 1 + args.present))
    N = sum(flat.meta[i]["count"] for i in present)
    ups = [rnd(N, 3), rnd(N, 4), rnd(N, 3), rnd(N, 1), rnd(N, M, 3), rnd(N, S)]  # the loss: sum of <w_k, out_k>

    def leg_a():
        outs = flat.compose(M, S, segments=present)
        torch.autograd.backward(outs, ups)
        opt.step(present)
        for t in flat.tensors.values():
            t.grad = None
        flat.poses.grad = None

    def leg_b():
        sink = opt.sink(present)
        outs = flat.compose(M, S, segments=present, grad_sink=sink)
        torch.autograd.backward(outs, ups)
        opt.step(present)
        flat.poses.grad = None

    legs = {"a": leg_a, "b": leg_b}
    run = [k for k in ("a", "b") if args.leg in ("both", k)]
    for _ in range(args.warmup):
        for k in run:
            legs[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(args.reps):
        for k in run:  # alternating: drift of clocks and temperature falls on both legs alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            legs[k]()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    elements = sum(t.numel() for t in flat.tensors.values())
    stepped = sum(flat.meta[i]["count"] * (3 + 4 + 3 + 1 + 3 * flat.meta[i]["fourier_dim"] + 3 * (M - 1) + flat.meta[i]["sem_width"])
                  for i in present)
    out = {"background": n_bg, "elements": elements, "stepped_elements": stepped}
    for k in run:
        t = np.asarray(times[k])
        p5, p50, p95 = np.percentile(t, [5, 50, 95])
        out[f"leg_{k}_median_ms"] = round(float(p50), 4)
        out[f"leg_{k}_p5_p95_width_ms"] = round(float(p95 - p5), 4)
    if len(run) == 2:
        out["sink_wins"] = bool(out["leg_a_median_ms"] - out["leg_b_median_ms"] > out["leg_a_p5_p95_width_ms"])
        out["b_over_a"] = round(out["leg_b_median_ms"] / out["leg_a_median_ms"], 4)
    del flat, opt, ups
    torch.cuda.empty_cache()
    return out


result = {"what": "compose forward + backward + Adam step, flat mode: (a) two-step hand-over, (b) SegmentedAdam sink "
                  "(include/sgr_scene_step.h); device-event times, legs alternating in one process",
          "actors": args.actors, "actor_gaussians": args.actor_gaussians, "present": args.present, "M": M, "S": S,
          "reps": args.reps, "leg": args.leg, "device": torch.cuda.get_device_name(0),
          "sizes": [measure(n) for n in args.sizes]}
line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
