"""Float reference of losses.frame_loss: train.py:100-133 of the reference restated as ONE function over the per-term
restatements of tests/torch_ref_loss.py, in train.py's order and with its Python-float weights (any device / dtype) --
test infrastructure only.  tests/test_frame_loss_cpu.py holds it bit for bit to what the reference's own text returned
(tests/golden/frame_loss/pins.npz)."""
import torch

import torch_ref_loss as ref

NAMES = ("l1", "ssim", "sky", "obj", "lidar", "mse", "psnr", "loss")


def clamp32(acc):
    """torch.clamp(acc, min=1e-6, max=1.-1e-6) with the bounds float32 rounds them to.  On float32 tensors that is what
    train.py:107,117 compute already (the clamp inside ref.sky_loss / ref.obj_acc_loss then changes nothing, value or
    gradient); on float64 tensors it keeps the function the same: 1 - 1e-6 is not a float32, and -log(1 - acc) at the
    bound is 13.80 at the float32 bound and 13.82 at the double one."""
    return torch.clamp(acc, min=float(torch.tensor(1e-6, dtype=torch.float32)), max=float(torch.tensor(1. - 1e-6, dtype=torch.float32)))


def mse(img1, img2, mask=None):
    """loss_utils.py:67-76: mean squared difference over the C values of the selected pixels."""
    a, b = img1.permute(1, 2, 0), img2.permute(1, 2, 0)
    if mask is not None:
        a, b = a[mask[0]], b[mask[0]]
    return torch.mean((a - b) ** 2)


def psnr(img1, img2, mask=None):
    """loss_utils.py:61-78."""
    return 20 * torch.log10(1.0 / torch.sqrt(mse(img1, img2, mask)))


def frame_loss(image, gt, mask=None, *, lambda_dssim=0.2, lambda_l1=1.0, acc=None, sky_mask=None, lambda_sky=0.0,
               sky_scale=None, acc_obj=None, obj_bound=None, lambda_reg=0.0, depth=None, lidar_depth=None,
               lambda_depth_lidar=0.0, keep=0.95):
    """-> dict of the eight 0-dim tensors of NAMES.  A term is on when both tensors of its pair are given (an off term is
    0 and is not added); ``sky_scale`` None is train.py's empty ``lambda_sky_scale`` (no multiplication)."""
    zero = torch.zeros((), dtype=image.dtype, device=image.device)
    out = {k: zero for k in NAMES}
    out["l1"] = ref.l1_loss(image, gt, mask)                                                   # train.py:101
    out["ssim"] = ref.ssim(image, gt, mask=mask)
    loss = (1.0 - lambda_dssim) * lambda_l1 * out["l1"] + lambda_dssim * (1.0 - out["ssim"])  # :103
    if acc is not None and sky_mask is not None:                                               # :106-112
        sky = ref.sky_loss(clamp32(acc), sky_mask)
        if sky_scale is not None:
            sky = sky * sky_scale
        out["sky"] = sky
        loss = loss + lambda_sky * sky
    if acc_obj is not None and obj_bound is not None:                                          # :114-122
        out["obj"] = ref.obj_acc_loss(clamp32(acc_obj), obj_bound)
        loss = loss + lambda_reg * out["obj"]
    if depth is not None and lidar_depth is not None:                                          # :124-132 (unclamped acc)
        every = torch.ones_like(lidar_depth, dtype=torch.bool) if mask is None else mask
        out["lidar"] = ref.lidar_depth_loss(depth, acc, lidar_depth, every, keep)
        loss = loss + lambda_depth_lidar * out["lidar"]
    out["mse"] = mse(image, gt, mask)
    out["psnr"] = psnr(image, gt, mask)
    out["loss"] = loss
    return out
