#!/usr/bin/env python
"""Measurement of the optimiser step that closes a street_gaussians iteration (StreetGaussianModel.update_optimizer) on
one MI355X: a background plus 20 actors, SH degree 3, 19 semantic classes, at 1 M and 5 M Gaussians.

  fused       SegmentedAdam.step() over the FlatScene leaves (host planning + one HIP launch), and the bare launch
              with prebuilt tables (kernel only)
  reference   one torch.optim.Adam(eps=1e-15) per model over its seven named groups, default (foreach) and fused=True

Algorithmic bytes: every stepped element reads p, g, m, v and writes p, m, v (28 B).  The working set is far above the
256 MiB Infinity Cache, so the bytes come from HBM.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from street_gaussians_amd import _native, optim  # noqa: E402
from street_gaussians_amd.optim import ATTR, GROUPS, SegmentedAdam  # noqa: E402
from street_gaussians_amd.scene import FlatScene, Segment  # noqa: E402

HBM_BPS = 6.3e12   # achievable streaming rate (float4 copy) of the MI355X
dev = torch.device("cuda")


def scene(total, seed):
    """Background (80 %, fourier_dim 1, 19 classes) + 20 actors of odd, unequal sizes (fourier_dim 5, 1 class)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    n_act = [int(total * 0.2 * w / 210) | 1 for w in range(1, 21)]
    n_bg = total - sum(n_act)
    segs = [Segment(r(n_bg, 3), r(n_bg, 4), r(n_bg, 3), r(n_bg, 1), r(n_bg, 1, 3), r(n_bg, 15, 3), semantic=r(n_bg, 19))]
    for n in n_act:
        segs.append(Segment(r(n, 3), r(n, 4), r(n, 3), r(n, 1), r(n, 5, 3), r(n, 15, 3), semantic=r(n, 1), pose=r(7),
                            idft=r(5)))
    return FlatScene.from_segments(segs)


def timed(fn, n, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n  # ms


def lrs_for(n):
    return [{"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3,
             "semantic": 1e-3} for _ in range(n)]


def case(total, n_iter=50):
    flat = scene(total, 0)
    for t in flat.tensors.values():
        t.grad = torch.randn_like(t) * 1e-3
    elems = sum(t.numel() for t in flat.tensors.values())
    nbytes = 28 * elems
    opt = SegmentedAdam(flat, lrs_for(len(flat.meta)))
    step_ms = timed(opt.step, n_iter)

    # the bare launch with this step's tables, built once
    grads = {g: flat.tensors[ATTR[g]].grad.data_ptr() for g in GROUPS}
    rec, n_spans = optim.plan_step(opt.layout, opt.steps, opt.lrs, None, grads, opt.betas, opt.eps, opt._span,
                                   advance=False)
    chunks, recs = opt._chunk_table(), optim._pinned_to(rec, dev)
    L = _native.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    launch = lambda: _native.check(L.sgr_adam_step(C.c_void_p(chunks.data_ptr()), len(opt.layout) * 7,
                                                   C.c_void_p(recs.data_ptr()), len(rec), n_spans, 0.9, 0.999, stream))
    kernel_ms = timed(launch, n_iter)

    # the reference's form: one Adam per model over clones of its tensors
    ref = {}
    views = flat.views()
    for name, kw in (("torch_foreach", {}), ("torch_fused", {"fused": True})):
        try:
            opts = []
            for s, v in enumerate(views):
                ps = [torch.nn.Parameter(v[ATTR[g]].detach().clone()) for g in GROUPS]
                for p, g in zip(ps, GROUPS):
                    p.grad = torch.randn_like(p) * 1e-3
                opts.append(torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": g} for p, g in zip(ps, GROUPS)],
                                             lr=0.0, eps=1e-15, **kw))
            ref[name + "_ms"] = round(timed(lambda: [o.step() for o in opts], n_iter), 4)
            del opts, ps
        except (RuntimeError, ValueError) as e:
            ref[name + "_ms"] = f"not measured: {e}"
        torch.cuda.empty_cache()
    out = {"gaussians": total, "segments": len(flat.meta), "elements": elems, "algorithmic_bytes": nbytes,
           "fused_step_ms": round(step_ms, 4), "fused_kernel_ms": round(kernel_ms, 4),
           "kernel_hbm_fraction": round(nbytes / (kernel_ms * 1e-3) / HBM_BPS, 3),
           "step_hbm_fraction": round(nbytes / (step_ms * 1e-3) / HBM_BPS, 3), **ref}
    for k in ("torch_foreach_ms", "torch_fused_ms"):
        if isinstance(out[k], float):
            out["speedup_vs_" + k[:-3]] = round(out[k] / step_ms, 2)
    return out


def bitwise_vs_torch_foreach():
    """Share of elements where one fused step equals torch's foreach Adam bit for bit (p, exp_avg, exp_avg_sq)."""
    flat = scene(20_000, 1)
    for t in flat.tensors.values():
        t.grad = torch.randn_like(t)
    views = flat.views()
    ps = [[torch.nn.Parameter(v[ATTR[g]].detach().clone()) for g in GROUPS] for v in views]
    tops = [torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": g} for p, g in zip(pp, GROUPS)], lr=0.0, eps=1e-15,
                             foreach=True) for pp in ps]
    for pp, v in zip(ps, views):
        for p, g in zip(pp, GROUPS):
            off = v[ATTR[g]].data_ptr() - flat.tensors[ATTR[g]].data_ptr()
            p.grad = flat.tensors[ATTR[g]].grad.reshape(-1)[off // 4: off // 4 + p.numel()].view(p.shape).clone()
    opt = SegmentedAdam(flat, [{g: 1e-3 for g in GROUPS}] * len(views))
    for _ in range(3):
        opt.step()
        for o in tops:
            o.step()
    torch.cuda.synchronize()
    eq = tot = 0
    for s, (pp, o) in enumerate(zip(ps, tops)):
        sv = opt.state_views(s)
        for p, g in zip(pp, GROUPS):
            for a, b in ((flat.views()[s][ATTR[g]].detach(), p.detach()), (sv[g][0], o.state[p]["exp_avg"]),
                         (sv[g][1], o.state[p]["exp_avg_sq"])):
                eq += int((a.reshape(-1).view(torch.int32) == b.reshape(-1).view(torch.int32)).sum())
                tot += a.numel()
    return round(eq / tot, 6)


if __name__ == "__main__":
    res = {"what": "per-segment Adam step, background + 20 actors, SH3, 19 classes", "hbm_achievable_Bps": HBM_BPS,
           "bitwise_share_vs_torch_foreach_3_steps": bitwise_vs_torch_foreach()}
    sizes = [int(a) for a in sys.argv[1:]] or [1_000_000, 5_000_000]
    res["cases"] = [case(n) for n in sizes]
    print(json.dumps(res))
