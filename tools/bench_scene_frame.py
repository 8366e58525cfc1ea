#!/usr/bin/env python
"""Measurement of the per-frame compose (include/sgr_scene_frame.h) on one MI355X, flat-parameter mode, SH degree 3,
19 semantic classes, a background plus posed actors (BASELINE.json configs[2] scale):

  * a frame with `--present` of the actors (FlatScene.compose(segments=...)) against the full compose, and the target:
    the full compose's time scaled to the rows present plus the absent blocks' zero spans at HBM rate;
  * actors only (the render_object pass) against background only;
  * the camera pose correction on against off, at the background size and at `--big` background Gaussians;
  * the reference's torch formulation of the correction (correct_gaussian_xyz / _rotation + autograd) for comparison.

    python tools/bench_scene_frame.py [--background 1800000] [--actors 20] [--actor-gaussians 10000] [--present 12]

Prints one JSON line; times are ms per forward+backward (wall, synchronised, mean over --steps)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_ref_scene_frame as fref  # noqa: E402  (the torch formulation of the correction, as the thing to beat)
from street_gaussians_amd import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--background", type=int, default=1_800_000)
ap.add_argument("--big", type=int, default=5_000_000)
ap.add_argument("--actors", type=int, default=20)
ap.add_argument("--actor-gaussians", type=int, default=10_000)
ap.add_argument("--present", type=int, default=12)
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
M, S, C = 16, 19, 5
dev = torch.device("cuda")
gen = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)


def make_flat(n_bg):
    counts = [n_bg] + [args.actor_gaussians] * args.actors
    segs = []
    for k, n in enumerate(counts):
        d = dict(xyz=rnd(n, 3), rotation=rnd(n, 4), scaling=rnd(n, 3), opacity=rnd(n, 1), features_rest=rnd(n, M - 1, 3))
        if k == 0:
            d.update(features_dc=rnd(n, 1, 3), semantic=rnd(n, S))
        else:
            d.update(features_dc=rnd(n, C, 3), semantic=rnd(n, 1), pose=rnd(7), idft=rnd(C), class_label=k % S)
        segs.append(scene.Segment(**d))
    return scene.FlatScene.from_segments(segs)


def timeit(fn, leaves):
    ups = {}

    def run():
        for t in leaves:
            t.grad = None
        outs = [o for o in fn() if o.requires_grad and o.numel()]
        key = tuple(o.shape for o in outs)
        if key not in ups:
            ups[key] = [torch.randn_like(o) for o in outs]
        torch.autograd.backward(outs, ups[key])
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


def leaves_of(flat, *extra):
    return list(flat.tensors.values()) + [flat.poses] + list(extra)


flat = make_flat(args.background)
K = len(flat.meta)
corr = torch.tensor([0.99, 0.01, -0.02, 0.005, 0.1, -0.05, 0.02], device=dev, requires_grad=True)
present = [0] + list(range(1, 1 + args.present))
L = leaves_of(flat)
full = timeit(lambda: flat.compose(M, S), L)
subset = timeit(lambda: flat.compose(M, S, segments=present), L)
actors_only = timeit(lambda: flat.compose(M, S, segments=list(range(1, K))), L)
background_only = timeit(lambda: flat.compose(M, S, segments=[0]), L)
corr_off = full
corr_on = timeit(lambda: flat.compose(M, S, correction=corr), leaves_of(flat, corr))

# target of the subset frame: the full compose's time scaled to the rows present + the absent blocks' zeros at HBM rate
rows_all = sum(m["count"] for m in flat.meta)
rows_present = sum(flat.meta[i]["count"] for i in present)
absent_floats = sum(m["count"] * (3 + 4 + 3 + 1 + 3 * m["fourier_dim"] + 3 * (M - 1) + m["sem_width"])
                    for i, m in enumerate(flat.meta) if i not in present)
absent_floats += 7 * (args.actors - args.present)
HBM_GBPS = 8000.0
subset_target = full * rows_present / rows_all + 4 * absent_floats / HBM_GBPS / 1e6

# torch formulation of the correction on the composed background rows (what INTEGRATION.md used to prescribe)
nb = flat.meta[0]["count"]
xb = torch.randn(nb, 3, device=dev, requires_grad=True)
qb = torch.nn.functional.normalize(torch.randn(nb, 4, device=dev)).requires_grad_(True)
torch_corr = timeit(lambda: (fref.correct_xyz(corr, xb), fref.correct_rotation(corr, qb)), [xb, qb, corr])
del flat, L, xb, qb
torch.cuda.empty_cache()

big = make_flat(args.big)
LB = leaves_of(big)
big_off = timeit(lambda: big.compose(M, S), LB)
big_on = timeit(lambda: big.compose(M, S, correction=corr), leaves_of(big, corr))

print(json.dumps({
    "what": "per-frame scene compose forward+backward, flat mode (include/sgr_scene_frame.h)",
    "background": args.background, "actors": args.actors, "actor_gaussians": args.actor_gaussians, "M": M, "S": S,
    "full_ms": round(full, 3), "subset_present": args.present, "subset_ms": round(subset, 3),
    "subset_target_ms": round(subset_target, 3), "actors_only_ms": round(actors_only, 3),
    "background_only_ms": round(background_only, 3),
    "correction_off_ms": round(corr_off, 3), "correction_on_ms": round(corr_on, 3),
    "correction_overhead": round(corr_on / corr_off - 1, 3),
    "big_background": args.big, "big_correction_off_ms": round(big_off, 3), "big_correction_on_ms": round(big_on, 3),
    "big_correction_overhead": round(big_on / big_off - 1, 3),
    "torch_correction_only_ms": round(torch_corr, 3), "hbm_peak_GBps": HBM_GBPS}))
