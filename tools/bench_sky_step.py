#!/usr/bin/env python
"""Sky backward + sky optimiser step on one MI355X at the reference's defaults (1920x1280, a 6 x 1024 x 1024 x 3 cube
map, train mode, colour correction on), two legs alternating in one process:

  (a) composite_sky's backward into a dense cube_map.grad, torch.optim.Adam(eps=1e-15).step(),
      zero_grad(set_to_none=True) -- the path without this optimiser (cube_sink=None runs the parent's kernels);
  (b) composite_sky(cube_sink=) + SkyAdam.step().

Sky fractions 25 % (a mask over the top quarter) and 100 %.  The camera cycles through 8 views yawed -35..35 degrees in
10-degree steps; the cycle runs once first so that the active set has saturated, then 10 discarded pairs, then 100 timed
pairs.  Device events around the backward and the step (the forward is outside); median and 5-95 % width per leg, the
saturated active fraction, whether leg (b) ends with the bytes of the dense gradient stepped through sgr_adam_step (a
third, untimed leg), and its distance to torch's result.  Prints one JSON line.

    python tools/bench_sky_step.py                 # the measurement
    python tools/bench_sky_step.py --trace-run B   # leg a or b alone, 20 iterations at 25 %, for a kernel trace
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from street_gaussians_amd.sky import SkyAdam, composite_sky  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=100)
ap.add_argument("--discard", type=int, default=10)
ap.add_argument("--trace-run", choices=["a", "b"], default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_sky_step: needs a GPU")

H, W, R = 1280, 1920, 1024
LR = 0.01
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
rgb = (torch.rand(3, H, W, generator=g) * 0.8).to(dev).requires_grad_(True)
acc_base = torch.rand(1, H, W, generator=g).to(dev)
cube0 = torch.rand(6, R, R, 3, generator=g)
affine = torch.cat([torch.eye(3) + 0.05 * torch.randn(3, 3, generator=g), 0.02 * torch.randn(3, 1, generator=g)], 1)
affine = affine.to(dev).requires_grad_(True)
perturb = torch.rand(2, H, W, generator=g).to(dev)
dout = torch.randn(3, H, W, generator=g).to(dev)
f = 0.9 * W
K = torch.tensor([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]], device=dev)


def view(yaw_deg):
    yaw = math.radians(yaw_deg)
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
    w2c[:3, 3] = torch.tensor([1.5, -0.3, 4.0])
    return w2c.to(dev)


VIEWS = [view(y) for y in range(-35, 36, 10)]
assert len(VIEWS) == 8


class Leg:
    """kind: "torch" = leg (a); "sink" = leg (b); "dense" = the dense gradient stepped by SkyAdam through sgr_adam_step,
    untimed: the bitwise check of leg (b) at this size (torch's own kernels round differently)."""

    def __init__(self, kind):
        self.cube = cube0.clone().to(dev).requires_grad_(True)
        self.fused = kind == "sink"
        self.opt = torch.optim.Adam([self.cube], lr=LR, eps=1e-15) if kind == "torch" else SkyAdam(self.cube, LR)
        self.events = []

    def iteration(self, acc, sky_mask, w2c, timed):
        sink = self.opt.sink() if self.fused else None
        out = composite_sky(rgb, acc, self.cube, K, w2c, sky_mask=sky_mask, affine=affine, perturb=perturb, cube_sink=sink)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out.backward(dout)
        self.opt.step()
        if not self.fused:
            self.opt.zero_grad(set_to_none=True)
        e1.record()
        rgb.grad = affine.grad = None
        if timed:
            self.events.append((e0, e1))

    def times_us(self):
        torch.cuda.synchronize()
        t = np.array([1e3 * a.elapsed_time(b) for a, b in self.events])
        self.events = []
        return t


def scene(frac):
    sky_mask = torch.zeros(1, H, W, dtype=torch.bool, device=dev)
    sky_mask[:, : int(round(frac * H))] = True
    acc = acc_base.clone()
    acc[sky_mask] = 0.0
    return acc, sky_mask


def summary(t):
    lo, med, hi = np.percentile(t, [5, 50, 95])
    return {"median_us": round(float(med), 1), "p5_us": round(float(lo), 1), "p95_us": round(float(hi), 1),
            "width_us": round(float(hi - lo), 1), "n": int(t.size)}


if args.trace_run:
    acc, sky_mask = scene(0.25)
    leg = Leg("sink" if args.trace_run == "b" else "torch")
    for i in range(8 + 20):
        leg.iteration(acc, sky_mask, VIEWS[i % 8], False)
    torch.cuda.synchronize()
    print(json.dumps({"bench": "sky_step_trace_run", "leg": args.trace_run, "iterations": 28}))
    sys.exit(0)

results = []
for frac in (0.25, 1.0):
    acc, sky_mask = scene(frac)
    a, b, c = Leg("torch"), Leg("sink"), Leg("dense")
    for w2c in VIEWS:  # the cycle once: every block the rig will ever touch is active afterwards
        a.iteration(acc, sky_mask, w2c, False)
        b.iteration(acc, sky_mask, w2c, False)
        c.iteration(acc, sky_mask, w2c, False)
    saturated = b.opt.active_fraction()
    for i in range(args.discard + args.pairs):
        w2c = VIEWS[i % 8]
        a.iteration(acc, sky_mask, w2c, i >= args.discard)
        b.iteration(acc, sky_mask, w2c, i >= args.discard)
        c.iteration(acc, sky_mask, w2c, False)
    ta, tb = a.times_us(), b.times_us()
    sa, sb = summary(ta), summary(tb)
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in
               ((c.cube.detach(), b.cube.detach()), (c.opt.exp_avg, b.opt.exp_avg), (c.opt.exp_avg_sq, b.opt.exp_avg_sq)))
    vs_torch = float((a.cube.detach() - b.cube.detach()).abs().max())
    results.append({"sky_fraction": frac, "sky_pixels": int(sky_mask.sum()),
                    "dense_backward_torch_adam": sa, "sink_backward_sky_adam": sb,
                    "active_fraction_saturated": round(saturated, 4),
                    "active_fraction_end": round(b.opt.active_fraction(), 4),
                    "speedup_median": round(sa["median_us"] / sb["median_us"], 3),
                    "faster_by_more_than_dense_width": bool(sa["median_us"] - sb["median_us"] > sa["width_us"]),
                    "sink_equals_dense_sgr_adam_bitwise": bool(same),
                    "max_abs_cube_difference_to_torch_adam": vs_torch})
    del a, b, c
    torch.cuda.empty_cache()

print(json.dumps({"bench": "sky_step", "H": H, "W": W, "R": R, "pairs": args.pairs, "discarded_pairs": args.discard,
                  "device": torch.cuda.get_device_name(0), "results": results}))
