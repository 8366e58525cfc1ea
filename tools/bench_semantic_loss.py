#!/usr/bin/env python
"""Measurement of the fused semantic cross-entropy (include/sgr_semantic_loss.h) on one MI355X: forward + backward at
S = 19, 1920x1280, about 20 % of the pixels ignored, in both modes,

    fused  losses.semantic_loss(...) and loss.backward()
    torch  the float32 torch formulation (tests/torch_ref_semantic_loss.py: permute / reshape, F.cross_entropy, or the
           normalise-and-log of street_gaussian_renderer.py:261-262 and F.nll_loss) and loss.backward()

in one process, alternated after warm-up, timed with device events over windows of at least a second; the torch path is
also timed against itself (the width a difference has to exceed); host synchronisations of one step of each path are
counted with torch.cuda.set_sync_debug_mode("warn"); algorithmic bytes come from the shapes.  Prints one JSON line.

    python tools/bench_semantic_loss.py [--steps N] [--warmup N] [--rounds N]

Launch counts and kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_semantic_loss.py --trace-only fused|torch --mode logits --steps 20
"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_ref_semantic_loss as ref  # noqa: E402
from street_gaussians_amd import losses  # noqa: E402

H, W, S = 1280, 1920, 19
IGNORED = 0.2
HBM_ACHIEVABLE_GBPS = 6300.0  # a float4 copy on this chip; the 8 TB/s of the data sheet is not reachable


def make_inputs(dev, mode):
    g = torch.Generator().manual_seed(0)
    if mode == "logits":
        x = torch.randn(S, H, W, generator=g) * 4.0
    else:
        x = torch.softmax(torch.randn(S, H, W, generator=g) * 3.0, dim=0) * torch.rand(1, H, W, generator=g)
    labels = torch.randint(0, S, (H, W), generator=g)
    labels[torch.rand(H, W, generator=g) < IGNORED] = -1
    return dict(x=x.to(dev).requires_grad_(True), labels=labels.to(dev), mode=mode)


def fused(d):
    loss, _ = losses.semantic_loss(d["x"], d["labels"], mode=d["mode"])
    loss.backward()
    return loss


def formulation(d):
    loss = ref.formulation(d["x"], d["labels"].reshape(-1), d["mode"], -1)  # (the labels are in [-1, S): no clean-up pass)
    loss.backward()
    return loss


def step(fn, d):
    d["x"].grad = None
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


def measure(dev, mode, a):
    d = make_inputs(dev, mode)
    lf = step(fused, d).item()
    gf = d["x"].grad.clone()
    lt = step(formulation, d).item()
    grad_diff = float((gf - d["x"].grad).abs().max() / d["x"].grad.abs().max())
    n_valid = int((d["labels"] >= 0).sum())
    for fn in (fused, formulation):
        for _ in range(a.warmup):
            step(fn, d)
    torch.cuda.synchronize()
    # each path's window holds as many of its own steps as fill 1.2 s: the two differ by more than an order of magnitude
    steps = {fn: a.steps or max(20, int(1200.0 / max(window_ms(fn, d, 20), 1e-3))) for fn in (fused, formulation)}
    t = {"fused": [], "torch": [], "torch_again": []}
    for _ in range(a.rounds):
        t["fused"].append(window_ms(fused, d, steps[fused]))
        t["torch"].append(window_ms(formulation, d, steps[formulation]))
        t["torch_again"].append(window_ms(formulation, d, steps[formulation]))
    both = t["torch"] + t["torch_again"]
    width = (max(both) - min(both)) / median(both)
    px, lab = 4 * H * W, 8 * H * W
    # bytes the fused kernels have to move at least once: forward reads the valid pixels' S values and every label; the
    # backward reads both again and writes S values for every pixel
    valid_share = n_valid / (H * W)
    fused_bytes = int(S * px * valid_share + lab) + int(S * px * valid_share + lab + S * px)
    mf, mt = median(t["fused"]), median(both)
    return {"mode": mode, "loss_fused": lf, "loss_torch": lt, "max_grad_diff_over_max_grad": grad_diff, "n_valid": n_valid,
            "ignored_share": round(1 - valid_share, 4), "steps_per_window": {"fused": steps[fused], "torch": steps[formulation]}, "fused_ms": round(mf, 4),
            "torch_ms": round(mt, 4), "ratio_torch_over_fused": round(mt / mf, 3), "torch_width": round(width, 4),
            "fused_beats_torch_by_more_than_the_width": bool(mt - mf > width * mt),
            "windows_ms": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "host_syncs_per_step": {"fused": count_syncs(fused, d), "torch": count_syncs(formulation, d),
                                    "counter_check_step_plus_item": count_syncs(lambda x: fused(x).item(), d)},
            "fused_algorithmic_bytes": fused_bytes, "fused_GBps": round(fused_bytes / mf / 1e6, 1),
            "fused_share_of_achievable": round(fused_bytes / mf / 1e6 / HBM_ACHIEVABLE_GBPS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="steps per timed window (0: as many as fill 1.2 s)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="alternated windows per path")
    ap.add_argument("--mode", choices=("logits", "probabilities"), help="only this mode (default: both)")
    ap.add_argument("--trace-only", choices=("fused", "torch"), help="run only this path --steps times (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    dev = torch.device("cuda")
    modes = (a.mode,) if a.mode else ("logits", "probabilities")
    if a.trace_only:
        fn = fused if a.trace_only == "fused" else formulation
        for mode in modes:
            d = make_inputs(dev, mode)
            for _ in range(a.steps or 20):
                step(fn, d)
        torch.cuda.synchronize()
        print(json.dumps({"what": "trace run", "path": a.trace_only, "modes": modes, "steps": a.steps or 20}))
        return
    print(json.dumps({
        "what": f"semantic cross-entropy forward+backward, S={S}, {W}x{H}, int64 labels, {IGNORED:.0%} ignored",
        "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
        "hbm_achievable_GBps": HBM_ACHIEVABLE_GBPS, "results": [measure(dev, mode, a) for mode in modes]}))


if __name__ == "__main__":
    main()
