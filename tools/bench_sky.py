#!/usr/bin/env python
"""Measurement of the sky model's cube-map lookup (lib/models/sky_cubemap.py:99-120) on one MI355X: a 6 x 1024 x 1024 x 3
cube map sampled at every pixel of a 1920x1280 view, and at about 25 % of them as the masked [1, 1, N, 3] list, forward
and backward, with the HIP op (nvdiffrast.torch.texture drop-in, street_gaussians_amd/texture.py) and with the same
lookup in torch ops on the GPU (the float32 restatement tests/torch_ref_texture.py).  Prints one JSON line."""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nvdiffrast.torch as dr  # noqa: E402
import torch_ref_texture as ref  # noqa: E402

R, Cc, H, W = 1024, 3, 1280, 1920
HBM_GBPS = 8000.0
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
sky = torch.rand(6, R, R, Cc, generator=g).to(dev).requires_grad_(True)


def rays(h, w, yaw):
    """A pinhole camera's ray directions (get_rays_torch without perturbation): fx = fy = 0.9 w."""
    j, i = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    d = torch.stack([(i + 0.5 - w / 2) / (0.9 * w), -(j + 0.5 - h / 2) / (0.9 * w), torch.ones_like(i)], -1)
    c, s = math.cos(yaw), math.sin(yaw)
    rot = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return (d @ rot.T).to(dev)


rays_d = rays(H, W, 0.6)  # a yaw that puts a cube edge in view
mask = (torch.rand(H, W, generator=g) < 0.25).to(dev)
uv_full = rays_d[None].contiguous()
uv_mask = rays_d[mask][None, None].contiguous()


def ops_lookup(tex, uv):  # the restatement's arithmetic in float32 on the GPU
    Bt, _, Rr, _, C = tex.shape
    idx, w, _ = ref.tap_weights(uv, Bt, Rr)
    vals = tex.reshape(-1, C)[idx.clamp(min=0)]
    return (vals * w.to(tex.dtype).unsqueeze(-1)).sum(1).reshape(*uv.shape[:3], C)


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # us


def case(uv, n=50):
    N = uv.shape[1] * uv.shape[2]
    out = dr.texture(sky[None], uv, filter_mode="linear", boundary_mode="cube")
    dout = torch.rand_like(out)
    fwd = timed(lambda: dr.texture(sky[None], uv, filter_mode="linear", boundary_mode="cube"), n)
    both = timed(lambda: torch.autograd.grad(dr.texture(sky[None], uv, filter_mode="linear", boundary_mode="cube"), sky,
                                             dout), n)
    ofwd = timed(lambda: ops_lookup(sky[None], uv), 10)
    oboth = timed(lambda: torch.autograd.grad(ops_lookup(sky[None], uv), sky, dout), 10)
    a = dr.texture(sky[None], uv, filter_mode="linear", boundary_mode="cube")
    b = ops_lookup(sky[None], uv)
    tex_bytes = 6 * R * R * Cc * 4
    # algorithmic bytes: forward reads directions and writes outputs (the footprint texels are reused by neighbours and
    # counted once, at most the whole map); backward reads directions and dL/dout, writes the whole gradient once
    fwd_bytes = N * (12 + 4 * Cc) + min(tex_bytes, N * 4 * Cc)
    bwd_bytes = N * (12 + 4 * Cc) + tex_bytes
    bwd = both - fwd
    return {"samples": N, "fwd_us": round(fwd, 1), "bwd_us": round(bwd, 1), "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
            "fwd_hbm_fraction": round(fwd_bytes / (fwd * 1e-6) / (HBM_GBPS * 1e9), 3),
            "bwd_hbm_fraction": round(bwd_bytes / (bwd * 1e-6) / (HBM_GBPS * 1e9), 3),
            "torch_ops_fwd_us": round(ofwd, 1), "torch_ops_bwd_us": round(oboth - ofwd, 1),
            "speedup_fwd_bwd": round(oboth / both, 2), "max_abs_diff_vs_torch_ops": float((a - b).abs().max().detach())}


print(json.dumps({"what": "sky cube-map lookup, R=1024 C=3 at 1920x1280 (sky_cubemap.py:99-120)", "hbm_peak_GBps": HBM_GBPS,
                  "unmasked": case(uv_full), "masked_25pct": case(uv_mask)}))
