#!/usr/bin/env python
"""Measurement of Step 2 of the reference's render() (street_gaussian_renderer.py:107-117) on one MI355X at 1920x1280
with a 6 x 1024 x 1024 x 3 cube map, train mode: the fused HIP op (street_gaussians_amd.sky.composite_sky) against the
reference's formulation run as torch ops on the GPU (SkyCubeMap.forward with get_rays_torch, the composite, the
colour-correction einsum), which uses our HIP texture() for the lookup.  Sky fractions of 25 % (a sky mask over the top
quarter) and 100 %, with and without colour correction.  Forward and backward times, algorithmic bytes, the fraction of
the 6.3 TB/s HBM they imply, and the host synchronisations of each path (torch.cuda.set_sync_debug_mode("warn")).
Prints one JSON line."""
import json
import math
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nvdiffrast.torch as dr  # noqa: E402
from street_gaussians_amd.sky import composite_sky  # noqa: E402

H, W, R = 1280, 1920, 1024
HBM = 6.3e12
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
rgb = (torch.rand(3, H, W, generator=g) * 0.8).to(dev).requires_grad_(True)
acc_base = torch.rand(1, H, W, generator=g).to(dev)
cube = torch.rand(6, R, R, 3, generator=g).to(dev).requires_grad_(True)
affine = torch.cat([torch.eye(3) + 0.05 * torch.randn(3, 3, generator=g), 0.02 * torch.randn(3, 1, generator=g)], 1)
affine = affine.to(dev).requires_grad_(True)
f = 0.9 * W
K = torch.tensor([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]], device=dev)
yaw = math.radians(45.0)  # the view straddles a cube face edge
w2c = torch.eye(4)
w2c[:3, :3] = torch.tensor([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
w2c[:3, 3] = torch.tensor([1.5, -0.3, 4.0])
w2c = w2c.to(dev)
dout = torch.randn(3, H, W, generator=g).to(dev)


def torch_path(rgb, acc, cube, K, w2c, sky_mask, aff):
    """The reference's Step 2 as torch ops (train mode, white background)."""
    mask = sky_mask[0].clone()
    mask[:50, :] = True
    Rm, T = w2c[:3, :3], w2c[:3, 3]
    rays_o = -torch.matmul(Rm.T, T)
    i, j = torch.meshgrid(torch.arange(W, dtype=torch.float32, device=dev), torch.arange(H, dtype=torch.float32, device=dev),
                          indexing="xy")
    pi = torch.rand(H, W, device=dev)
    pj = torch.rand(H, W, device=dev)
    xy1 = torch.stack([i + pi, j + pj, torch.ones_like(i)], dim=2)
    pc = torch.matmul(xy1, torch.inverse(K).T)
    pw = torch.matmul(pc - T, Rm)
    d = pw - rays_o[None, None]
    d = d / torch.norm(d, dim=2, keepdim=True)
    sky = torch.ones(H, W, 3, device=dev)
    if mask.sum() > 0:
        sky[mask] = dr.texture(cube[None], d[mask][None, None], filter_mode="linear", boundary_mode="cube")[0, 0]
    sky = sky.permute(2, 0, 1).clamp(0.0, 1.0)
    out = rgb + sky * (1 - acc)
    if aff is not None:
        out = torch.einsum("ij,jhw->ihw", aff[:3, :3], out) + aff[:3, 3].unsqueeze(-1).unsqueeze(-1)
    return out


def fused_path(rgb, acc, cube, K, w2c, sky_mask, aff):
    return composite_sky(rgb, acc, cube, K, w2c, sky_mask=sky_mask, affine=aff)


def timed(fn, n=20):
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


def syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    # (the first set_sync_debug_mode call of a process also warns that the mode is a prototype: not a synchronisation)
    return sum(1 for x in w if "synchroniz" in str(x.message).lower() and "prototype" not in str(x.message))


def measure(path, acc, sky_mask, aff):
    inputs = (rgb, acc, cube, K, w2c, sky_mask, aff)

    def fwd():
        return path(*inputs)

    def fwd_bwd():
        path(*inputs).backward(dout)

    t_f = timed(fwd)
    t_fb = timed(fwd_bwd)
    return t_f, t_fb - t_f, syncs(fwd_bwd)


results = []
for frac in (0.25, 1.0):
    sky_mask = torch.zeros(1, H, W, dtype=torch.bool, device=dev)
    sky_mask[:, : int(round(frac * H))] = True
    acc = acc_base.clone()
    acc[sky_mask] = 0.0
    n_sky = int(sky_mask.sum())
    for with_aff in (False, True):
        aff = affine if with_aff else None
        # algorithmic bytes: forward reads rgb, acc, the two perturbation images and writes the output, plus one sky
        # value per sky pixel; the backward reads dL/dout, rgb, acc and writes dL/drgb, dL/dacc, reads and writes one
        # ray and one upstream per sky pixel (the texture backward's input) and writes the cube-map gradient once
        b_fwd = H * W * (12 + 4 + 8 + 12) + n_sky * 12
        b_bwd = H * W * (12 + 12 + 4 + 12 + 4) + n_sky * 24 + 6 * R * R * 3 * 4
        row = {"sky_fraction": frac, "sky_pixels": n_sky, "affine": with_aff, "fwd_bytes": b_fwd, "bwd_bytes": b_bwd}
        for name, path in (("fused", fused_path), ("torch", torch_path)):
            tf, tb, ns = measure(path, acc, sky_mask, aff)
            row[name] = {"fwd_us": round(tf, 1), "bwd_us": round(tb, 1), "host_syncs": ns,
                         "fwd_hbm_frac": round(b_fwd / (tf * 1e-6) / HBM, 3),
                         "bwd_hbm_frac": round(b_bwd / (tb * 1e-6) / HBM, 3)}
        results.append(row)

print(json.dumps({"bench": "sky_pass", "H": H, "W": W, "R": R, "device": torch.cuda.get_device_name(0),
                  "results": results}))
