"""Pins the image-space terms of a training step to the reference's own Python and writes tests/golden/frame_loss/pins.npz.

Cut out of the reference's files when this runs and executed here (no GPU), nothing of their text kept: the block of
train.py from ``# rgb loss`` to ``# color correction loss`` (train.py:100-133), and ``l1_loss``, ``gaussian``,
``create_window``, ``ssim``, ``_ssim`` and ``psnr`` of lib/utils/loss_utils.py.  The block runs on stub objects, as in
tests/test_loss_cpu.py::test_restated_sky_object_lidar_terms_match_train_py; ``acc`` and ``render_pkg['acc']`` are the
SAME leaf, so its gradient holds the sky term (clamped copy) and the LiDAR term (unclamped).  Run where the reference
checkout exists:

    python tests/golden/make_frame_loss_fixture.py

Every case is evaluated in float32 (what the reference computes) and in float64 on the same float32 inputs.  One textual
change, in the float64 run only: the clamp bounds ``min=1e-6, max=1.-1e-6`` are replaced by their float32 roundings.  The
float32 run clamps there (1 - 1e-6 is not a float32), and -log(1 - acc) at the bound is 13.80 in float32 and 13.82 at the
double bound: the bound is part of the function, not of its rounding error.

Inputs (shared by the cases, H x W = 41 x 57, C = 3, from a seeded CPU generator): ``image``, ``gt`` [3,H,W]; ``acc``
[1,H,W] with rows 0-2 pinned to 0 and rows 3-4 to 1 (both clamps active); ``acc_obj``, ``depth`` [1,H,W]; ``lidar`` [1,H,W],
0 where there is no return (about 60 %, and all of rows 0-2, where nothing was accumulated); ``mask``, ``sky_mask``,
``obj_bound`` [1,H,W] bool.  Weights: ``lambda_dssim`` 0.2, ``lambda_l1`` 1, ``lambda_sky`` 0.05, ``lambda_reg`` 0.1,
``lambda_depth_lidar`` 0.1 (stored), ``iteration`` past ``densify_until_iter``.

Cases (``names``): ``masked`` -- ``mask`` as drawn, ``lambda_sky_scale = []``; ``scaled_nomask`` -- ``lambda_sky_scale =
[0.7, 1.3]``, ``cam = 1`` and no mask, which for the reference's text is the all-True mask its training loop would carry
(``logical_and(lidar_depth > 0, None)`` does not run).  Per case ``<name>/``: ``masked``, ``sky_scale`` (NaN = empty
list); the scalars ``l1_loss``, ``sky_loss``, ``obj_acc_loss``, ``lidar_depth_loss`` (scalar_dict), ``loss``, ``psnr``
(the cut-out function), ``ssim`` (the cut-out function) and ``mse`` (the line of psnr that computes it, restated here);
the gradients of ``loss``: ``d_image``, ``d_acc``, ``d_depth``, ``d_acc_obj``; each as ``<key>32`` and ``<key>64``.
Global: ``e_ref_<key>`` = max over the cases of |f32 - f64| / scale, scale = |f64| of a scalar, the largest |f64| entry of
a gradient (tests/golden/README.md).
"""
import os
import re
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden import make_callsite_fixture as mk  # noqa: E402

OUT = os.path.join(HERE, "frame_loss", "pins.npz")
REF = mk.REF
H, W, C = 41, 57, 3
WEIGHTS = dict(lambda_dssim=0.2, lambda_l1=1.0, lambda_sky=0.05, lambda_reg=0.1, lambda_depth_lidar=0.1)
SCALARS = ("l1_loss", "sky_loss", "obj_acc_loss", "lidar_depth_loss", "loss", "psnr", "ssim", "mse")
GRADS = ("d_image", "d_acc", "d_depth", "d_acc_obj")
CASES = {"masked": dict(masked=True, scale=[], cam=0), "scaled_nomask": dict(masked=False, scale=[0.7, 1.3], cam=1)}
CLAMP = "min=1e-6, max=1.-1e-6"
CLAMP32 = f"min={float(np.float32(1e-6))!r}, max={float(np.float32(1. - 1e-6))!r}"


def make_inputs():
    g = torch.Generator().manual_seed(20241019)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    image = r(C, H, W)
    gt = (image + 0.2 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
    acc = r(1, H, W)
    acc[0, :3] = 0.0
    acc[0, 3:5] = 1.0
    acc_obj = r(1, H, W)
    depth = r(1, H, W) * 30
    lidar = r(1, H, W) * 30 * (r(1, H, W) < 0.4)
    lidar[0, :3] = 0.0
    return dict(image=image, gt=gt, acc=acc, acc_obj=acc_obj, depth=depth, lidar=lidar, mask=r(1, H, W) < 0.8,
                sky_mask=r(1, H, W) < 0.2, obj_bound=r(1, H, W) < 0.3)


def reference_text():
    """-> (the train.py block, dedented; the namespace holding loss_utils' cut-out functions)."""
    src = open(os.path.join(REF, "train.py")).read()
    a, b = src.index("        # rgb loss"), src.index("        # color correction loss")
    block = textwrap.dedent(src[a:b])
    assert block.count(CLAMP) == 2, "the two clamps of train.py:107,117"
    lu = open(os.path.join(REF, "lib/utils/loss_utils.py")).read()
    ns = {"torch": torch, "F": torch.nn.functional, "exp": __import__("math").exp, "Variable": lambda t: t}
    for name in ("l1_loss", "gaussian", "create_window", "ssim", "_ssim", "psnr"):
        m = re.search(rf"^def {name}\(.*?(?=^def |\Z)", lu, re.S | re.M)
        assert m, name
        exec(m.group(0), ns)
    return block, ns


def evaluate_case(inp, case, dt):
    """The reference's text on one case in dtype ``dt`` -> dict of numpy scalars and gradients."""
    block, fns = reference_text()
    if dt == torch.float64:
        block = block.replace(CLAMP, CLAMP32)
    leaf = lambda k: inp[k].clone().to(dt).requires_grad_(True)  # noqa: E731
    image, acc, depth, acc_obj = leaf("image"), leaf("acc"), leaf("depth"), leaf("acc_obj")
    gt = inp["gt"].to(dt)
    mask = inp["mask"] if case["masked"] else torch.ones_like(inp["mask"])
    ns = dict(fns, image=image, gt_image=gt, mask=mask, acc=acc, render_pkg={"acc": acc}, depth=depth,
              lidar_depth=inp["lidar"].to(dt), sky_mask=inp["sky_mask"], obj_bound=inp["obj_bound"], scalar_dict={},
              iteration=10,
              optim_args=types.SimpleNamespace(lambda_sky_scale=case["scale"], densify_until_iter=5, **WEIGHTS),
              gaussians=types.SimpleNamespace(include_sky=True, include_obj=True),
              viewpoint_cam=types.SimpleNamespace(meta={"cam": case["cam"]}),
              gaussians_renderer=types.SimpleNamespace(render_object=lambda *a, **k: {"rgb": None, "acc": acc_obj}))
    exec(block, ns)
    sd = ns["scalar_dict"]
    assert set(sd) == {"l1_loss", "sky_loss", "obj_acc_loss", "lidar_depth_loss"}, sorted(sd)
    loss = ns["loss"]
    loss.backward()
    with torch.no_grad():
        a, b = image.permute(1, 2, 0)[mask[0]], gt.permute(1, 2, 0)[mask[0]]
        out = {k: np.asarray(float(sd[k]), np.float64) for k in sd}
        out.update(loss=loss.detach().numpy(), psnr=fns["psnr"](image, gt, mask).numpy(),
                   ssim=fns["ssim"](image, gt, mask=mask).numpy(), mse=torch.mean((a - b) ** 2).numpy())
    out.update(d_image=image.grad.numpy(), d_acc=acc.grad.numpy(), d_depth=depth.grad.numpy(), d_acc_obj=acc_obj.grad.numpy())
    np_dt = np.float32 if dt == torch.float32 else np.float64
    for k in SCALARS + GRADS:
        out[k] = np.asarray(out[k]).astype(np_dt)  # (.item() of a float32 scalar is exact in a double and back)
        assert np.isfinite(out[k]).all(), k
    return out


def build():
    inp = make_inputs()
    d = {"names": np.asarray(list(CASES))}
    d.update({k: v.numpy() for k, v in inp.items()})
    d.update({k: np.float64(v) for k, v in WEIGHTS.items()})
    e_ref = {k: 0.0 for k in SCALARS + GRADS}
    for name, case in CASES.items():
        o32, o64 = evaluate_case(inp, case, torch.float32), evaluate_case(inp, case, torch.float64)
        d[f"{name}/masked"] = np.bool_(case["masked"])
        d[f"{name}/sky_scale"] = np.float64(case["scale"][case["cam"]] if case["scale"] else np.nan)
        for k in SCALARS + GRADS:
            d[f"{name}/{k}32"], d[f"{name}/{k}64"] = o32[k], o64[k]
            sc = np.abs(o64[k]).max()
            assert sc > 0, (name, k)
            e_ref[k] = max(e_ref[k], float(np.abs(o32[k].astype(np.float64) - o64[k]).max() / sc))
        assert (o64["d_acc"][0, :3] == 0).all()
        if case["masked"]:
            assert (o64["d_image"][:, ~inp["mask"][0].numpy()] == 0).all()
    for k, v in e_ref.items():
        d["e_ref_" + k] = np.float64(v)
    return d


def load(path=OUT):
    return dict(np.load(path))


def case(d, name):
    """The entries of one case, without the prefix."""
    p = name + "/"
    return {k[len(p):]: v for k, v in d.items() if k.startswith(p)}


if __name__ == "__main__":
    d = build()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: float(v) for k, v in d.items() if k.startswith("e_ref_")})
