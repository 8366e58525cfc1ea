#!/usr/bin/env python
"""Measurement of the layered forward (GaussianRasterizer.forward_layers, include/sgr_layers.h) on one MI355X: the three
images the reference's StreetGaussianRenderer.render_all asks for (lib/models/street_gaussian_renderer.py:13-72) -- composite,
background alone, objects alone -- of a street-like frame (synthetic.make_street_segments: 1 M Gaussians, 12 actors,
composed by scene.compose) at 1920x1280, SH degree 3, in the strict mode (EXACT | REF_RECT) and the default mode.

Timed with device events after a warm-up, the three alternating in the same process, one event pair per call:
  layered   one forward_layers call (split = rows of the background model, white layer background)
  separate  the three forwards it replaces: the whole set on the frame's background, [0, split) on white, [split, P) on white
            (their inputs are sliced beforehand: the two extra composes the reference also pays are NOT counted)
  plain     one forward of the whole set: layered - plain = what the extra launch costs
Reports the median and the 5 / 25 / 75 / 95 % quantiles of each; `spread` is the 5-95 % width.  `faster_beyond_spread` is the
acceptance condition: median(separate) - median(layered) > spread(separate).  The extra kernel's own time comes from a
`rocprofv3 --kernel-trace --stats` run of this script (sgr_blend_layers_kernel).  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from street_gaussians_amd import _C, scene as sg, synthetic as syn  # noqa: E402
from street_gaussians_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--actors", type=int, default=12)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1280)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--modes", default="strict,default")
args = ap.parse_args()

dev = torch.device("cuda")
W, H = args.width, args.height
cam = syn.make_camera(W, H, fx=2050.0 * W / 1920.0)
raw = syn.make_street_segments(args.gaussians, cam, n_actors=args.actors)
split = int(raw[0]["xyz"].shape[0])  # compose puts the background model's rows first
segs = [sg.Segment(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items() if v is not None}) for d in raw]
with torch.no_grad():
    means, rot, scl, opa, shs, _ = sg.compose(segs, 16, 0)
del segs
P = means.shape[0]


def inputs(lo, hi):
    c = lambda t: t[lo:hi].contiguous()
    return dict(means3D=c(means), means2D=torch.zeros(hi - lo, 3, device=dev), opacities=c(opa), shs=c(shs), scales=c(scl),
                rotations=c(rot))


def settings(bg):
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg,
                                         scale_modifier=1.0, viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev),
                                         sh_degree=3, campos=cam.campos.to(dev), prefiltered=False, debug=False)


frame_bg = torch.tensor([0.1, 0.3, 0.6], device=dev)
white = torch.ones(3, device=dev)
whole, first, rest = inputs(0, P), inputs(0, split), inputs(split, P)
r_frame, r_white = GaussianRasterizer(settings(frame_bg)), GaussianRasterizer(settings(white))


def layered():
    return r_frame.forward_layers(**whole, split=split, layer_background=white)


def separate():
    return r_frame(**whole), r_white(**first), r_white(**rest)


def plain():
    return r_frame(**whole)


def quantiles(ms):
    t = torch.tensor(sorted(ms), dtype=torch.float64)
    q = lambda p: round(float(torch.quantile(t, p)), 4)
    return {"median_ms": q(0.5), "p05_ms": q(0.05), "p25_ms": q(0.25), "p75_ms": q(0.75), "p95_ms": q(0.95),
            "spread_ms": round(q(0.95) - q(0.05), 4), "n": len(ms)}


def measure():
    paths = (("layered", layered), ("separate", separate), ("plain", plain))
    with torch.no_grad():
        for _ in range(args.warmup):
            for _, fn in paths:
                fn()
        torch.cuda.synchronize()
        ev = {name: [] for name, _ in paths}
        for _ in range(args.iters):
            for name, fn in paths:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
    out = {name: quantiles([a.elapsed_time(b) for a, b in pairs]) for name, pairs in ev.items()}
    gain = out["separate"]["median_ms"] - out["layered"]["median_ms"]
    out["separate_over_layered"] = round(out["separate"]["median_ms"] / out["layered"]["median_ms"], 3)
    out["extra_launch_ms"] = round(out["layered"]["median_ms"] - out["plain"]["median_ms"], 4)
    out["faster_beyond_spread"] = bool(gain > out["separate"]["spread_ms"])
    return out


MASKS = {"strict": _C.EXACT | _C.REF_RECT, "default": 0}
results = {}
prev = _C.test_switches(-1)
try:
    for mode in args.modes.split(","):
        _C.test_switches(MASKS[mode])
        results[mode] = measure()
finally:
    _C.test_switches(prev)

print(json.dumps({"bench": "layers", "device": torch.cuda.get_device_name(0), "gaussians": P, "split": split,
                  "actors": args.actors, "width": W, "height": H, "sh_degree": 3, "iters": args.iters, "warmup": args.warmup,
                  "results": results}))
