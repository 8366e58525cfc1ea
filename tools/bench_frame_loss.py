#!/usr/bin/env python
"""Measurement of the fused frame loss (include/sgr_frame_loss.h) on one MI355X: forward + backward of
every image-space term of train.py:100-133 at 1920x1280, C = 3, masked, all terms on,

    fused        losses.frame_loss(...) and loss.backward()
    composition  color_loss + l * sky_loss + l * obj_acc_loss + l * lidar_depth_loss (today's stand-alone ops, the
                 weights and sums in torch, the two dL/dacc images added by autograd) and loss.backward()

in one process, alternated after warm-up, timed with device events over windows of at least a second; the composition is
also timed against itself (the spread a difference has to exceed); host synchronisations of one step of each path are
counted with torch.cuda.set_sync_debug_mode("warn"); algorithmic bytes come from the shapes.  Prints one JSON line.

    python tools/bench_frame_loss.py [--steps N] [--warmup N] [--rounds N]

Launch counts and kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_frame_loss.py --trace-only fused|composition --steps 20
"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from street_gaussians_amd import losses  # noqa: E402

H, W, C = 1280, 1920, 3
L_DSSIM, L_SKY, L_REG, L_LIDAR, SKY_SCALE = 0.2, 0.05, 0.1, 0.1, 1.3


def make_inputs(dev):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    gt = r(C, H, W)
    d = dict(gt=gt, image=(gt + 0.1 * torch.randn(C, H, W, generator=g)).clamp(0, 1), mask=r(1, H, W) < 0.9,
             acc=r(1, H, W) * 0.98 + 0.01, acc_obj=r(1, H, W) * 0.98 + 0.01, depth=r(1, H, W) * 40, sky_mask=r(1, H, W) < 0.2,
             obj_bound=r(1, H, W) < 0.3, lidar=torch.where(r(1, H, W) < 0.3, r(1, H, W) * 60, torch.zeros(1, H, W)))
    d = {k: v.to(dev) for k, v in d.items()}
    for k in ("image", "acc", "acc_obj", "depth"):
        d[k].requires_grad_(True)
    return d


def fused(d):
    loss, terms = losses.frame_loss(d["image"], d["gt"], d["mask"], lambda_dssim=L_DSSIM, acc=d["acc"], sky_mask=d["sky_mask"],
                                    lambda_sky=L_SKY, sky_scale=SKY_SCALE, acc_obj=d["acc_obj"], obj_bound=d["obj_bound"],
                                    lambda_reg=L_REG, depth=d["depth"], lidar_depth=d["lidar"], lambda_depth_lidar=L_LIDAR)
    loss.backward()
    return loss


def composition(d):
    loss = losses.color_loss(d["image"], d["gt"], d["mask"], lambda_dssim=L_DSSIM)                       # train.py:100-104
    loss = loss + L_SKY * (losses.sky_loss(d["acc"], d["sky_mask"]) * SKY_SCALE)                         # :106-112
    loss = loss + L_REG * losses.obj_acc_loss(d["acc_obj"], d["obj_bound"])                              # :114-122
    loss = loss + L_LIDAR * losses.lidar_depth_loss(d["depth"], d["acc"], d["lidar"], d["mask"])         # :124-132
    loss.backward()
    return loss


def step(fn, d):
    for k in ("image", "acc", "acc_obj", "depth"):
        d[k].grad = None
    return fn(d)


def window_ms(fn, d, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step(fn, d)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def count_syncs(fn, d):
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step(fn, d)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    return sum("called a synchronizing" in str(w.message) for w in seen)  # (not the mode's own "prototype feature" notice)


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="steps per timed window (0: as many as fill 1.2 s)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="alternated windows per path")
    ap.add_argument("--trace-only", choices=("fused", "composition"), help="run only this path --steps times (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    dev = torch.device("cuda")
    d = make_inputs(dev)
    if a.trace_only:
        fn = fused if a.trace_only == "fused" else composition
        for _ in range(a.steps or 20):
            step(fn, d)
        torch.cuda.synchronize()
        print(json.dumps({"what": "trace run", "path": a.trace_only, "steps": a.steps or 20}))
        return
    lf, lc = step(fused, d).item(), step(composition, d).item()
    gf = {k: d[k].grad.clone() for k in ("image", "acc", "acc_obj", "depth")}
    step(composition, d)
    grad_diff = {k: float((gf[k] - d[k].grad).abs().max() / d[k].grad.abs().max()) for k in gf}
    for fn in (fused, composition):
        for _ in range(a.warmup):
            step(fn, d)
    torch.cuda.synchronize()
    steps = a.steps or max(20, int(1200.0 / max(window_ms(composition, d, 20), 1e-3)))
    t = {"fused": [], "composition": [], "composition_again": []}
    for _ in range(a.rounds):
        t["fused"].append(window_ms(fused, d, steps))
        t["composition"].append(window_ms(composition, d, steps))
        t["composition_again"].append(window_ms(composition, d, steps))
    both = t["composition"] + t["composition_again"]
    spread = (max(both) - min(both)) / median(both)
    px, n = 4 * H * W, H * W
    # bytes every kernel has to move at least once, from the shapes (f32 images, byte masks, the LiDAR keys)
    fused_bytes = (2 * C * px + n + 4 * px + 2 * n + 3 * C * px + px) + (3 * C * px + 2 * C * px + n + 5 * px + 2 * n + C * px + 3 * px)
    comp_bytes = (2 * C * px + n) + (2 * C * px + n + 3 * C * px) + (3 * C * px + 2 * C * px + n + C * px) + 2 * (px + n) + \
        2 * (px + n + px) + (3 * px + n + px) + (4 * px + 2 * px) + 3 * px
    mf, mc = median(t["fused"]), median(both)
    print(json.dumps({
        "what": "frame loss forward+backward, every image-space term of train.py:100-133 (SURVEY 8f n3), 1920x1280, C=3, masked",
        "device": torch.cuda.get_device_name(0), "steps_per_window": steps, "rounds": a.rounds, "warmup": a.warmup,
        "loss_fused": lf, "loss_composition": lc, "max_grad_diff_over_max_grad": grad_diff,
        "fused_ms": round(mf, 4), "composition_ms": round(mc, 4), "ratio_composition_over_fused": round(mc / mf, 3),
        "composition_spread": round(spread, 4), "windows_ms": {k: [round(x, 4) for x in v] for k, v in t.items()},
        "host_syncs_per_step": {"fused": count_syncs(fused, d), "composition": count_syncs(composition, d),
                                "counter_check_step_plus_item": count_syncs(lambda x: fused(x).item(), d)},
        "algorithmic_bytes": {"fused": fused_bytes, "composition": comp_bytes},
        "fused_GBps": round(fused_bytes / mf / 1e6, 1), "hbm_peak_GBps": 8000.0}))


if __name__ == "__main__":
    main()
