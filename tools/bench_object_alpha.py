#!/usr/bin/env python
"""Measurement of the object-alpha head (GaussianRasterizer.forward_with_object_alpha, include/sgr_object_alpha.h) on one
MI355X: one training step of the iterations in which the reference regularises the objects' accumulated alpha
(train.py:114-122) -- the composite's forward + backward AND the alpha image of the actors alone with its gradient -- on the
street-like frame of tools/bench_layers.py (synthetic.make_street_segments: 1 M Gaussians, 12 actors, composed by
scene.compose) at 1920x1280, SH degree 3, in the strict mode (EXACT | REF_RECT) and the default mode.

Both ways start from the same composed leaf tensors and end with their .grad filled:
  two_renders  (a) composite forward + backward, plus an actors-only forward + backward over the rows [split, P) sliced from
               the composed tensors, upstream gradient on alpha only: the best form without the head (the second compose the
               reference also pays is NOT counted)
  one_call     (b) forward_with_object_alpha(..., split=) and ONE backward over both heads
Timed with device events around the whole step, the two alternating in the same process after `--warmup` discarded pairs.
Reports the median and the 5 / 25 / 75 / 95 % quantiles of each; `spread` is the 5-95 % width.  `faster_beyond_spread` is the
acceptance condition: median(two_renders) - median(one_call) > spread(two_renders).  The new kernels' own times come from a
`rocprofv3 --kernel-trace --stats` run of this script (sgr_object_alpha_fwd_kernel / _bwd_kernel).  Prints one JSON line and
writes it to --out (default profiles/object_alpha/bench_object_alpha.json)."""
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
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--modes", default="strict,default")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_alpha", "bench_object_alpha.json"))
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
leaves = dict(means3D=means, opacities=opa, shs=shs, scales=scl, rotations=rot)
leaves = {k: v.detach().contiguous().requires_grad_(True) for k, v in leaves.items()}
means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
means2D_obj = torch.zeros(P - split, 3, device=dev, requires_grad=True)

st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                   bg=torch.tensor([0.1, 0.3, 0.6], device=dev), scale_modifier=1.0,
                                   viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), sh_degree=3,
                                   campos=cam.campos.to(dev), prefiltered=False, debug=False)
rast = GaussianRasterizer(st)
lw = syn.loss_weights(cam, S=0)
wc, wd, wa = lw["color"].to(dev), lw["depth"].to(dev), lw["alpha"].to(dev)
wo = torch.rand(1, H, W, generator=torch.Generator().manual_seed(5)).to(dev) * 2.0 - 1.0


def clear():
    for t in list(leaves.values()) + [means2D, means2D_obj]:
        t.grad = None


def two_renders():
    clear()
    color, _, depth, alpha, _ = rast(means2D=means2D, **leaves)
    sub = {k: v[split:] for k, v in leaves.items()}
    _, _, _, acc, _ = rast(means2D=means2D_obj, **sub)
    ((color * wc).sum() + (depth * wd).sum() + (alpha * wa).sum() + (acc * wo).sum()).backward()


def one_call():
    clear()
    color, _, depth, alpha, _, acc = rast.forward_with_object_alpha(means2D=means2D, **leaves, split=split)
    ((color * wc).sum() + (depth * wd).sum() + (alpha * wa).sum() + (acc * wo).sum()).backward()


def quantiles(ms):
    t = torch.tensor(sorted(ms), dtype=torch.float64)
    q = lambda p: round(float(torch.quantile(t, p)), 4)
    return {"median_ms": q(0.5), "p05_ms": q(0.05), "p25_ms": q(0.25), "p75_ms": q(0.75), "p95_ms": q(0.95),
            "spread_ms": round(q(0.95) - q(0.05), 4), "n": len(ms)}


def measure():
    paths = (("two_renders", two_renders), ("one_call", one_call))
    for _ in range(max(1, args.warmup)):  # discarded pairs
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
    gain = out["two_renders"]["median_ms"] - out["one_call"]["median_ms"]
    out["gain_ms"] = round(gain, 4)
    out["two_renders_over_one_call"] = round(out["two_renders"]["median_ms"] / out["one_call"]["median_ms"], 3)
    out["faster_beyond_spread"] = bool(gain > out["two_renders"]["spread_ms"])
    return out


def same_results():
    """Faster and different is not faster: the two ways' gradients on this frame, as the largest difference over the
    tensor's largest entry (reordered float32 sums: rounding level)."""
    two_renders()
    torch.cuda.synchronize()
    a = {k: v.grad.clone() for k, v in leaves.items()}
    one_call()
    torch.cuda.synchronize()
    return {k: float((v.grad - a[k]).abs().max() / a[k].abs().max().clamp_min(1e-30)) for k, v in leaves.items()}


MASKS = {"strict": _C.EXACT | _C.REF_RECT, "default": 0}
results, agree = {}, {}
prev = _C.test_switches(-1)
try:
    for mode in args.modes.split(","):
        _C.test_switches(MASKS[mode])
        agree[mode] = same_results()
        results[mode] = measure()
finally:
    _C.test_switches(prev)

line = json.dumps({"bench": "object_alpha", "device": torch.cuda.get_device_name(0), "gaussians": P, "split": split,
                   "actors": args.actors, "width": W, "height": H, "sh_degree": 3, "iters": args.iters, "warmup": args.warmup,
                   "results": results, "max_grad_difference_over_scale": agree})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
