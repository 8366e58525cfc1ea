"""Helpers of the colour-Jacobian and skip_cov3d_grad GPU tests: gpu_utils.raw_forward / raw_backward with the extension
keywords of the native entry points (color_jacobian, skip_sh_grad, masked_color_out, skip_cov3d_grad, out)."""
import contextlib
import functools

import torch

from gpu_utils import GRAD_NAMES, dev
from street_gaussians_amd import _C


@contextlib.contextmanager
def asking_for_jacobian():
    """gpu_utils.raw_forward, with the forward asking for the colour Jacobian."""
    orig = _C.rasterize_gaussians
    _C.rasterize_gaussians = functools.partial(orig, color_jacobian=True)
    try:
        yield
    finally:
        _C.rasterize_gaussians = orig


def backward_with(kw, res, wts, **extra):
    """gpu_utils.raw_backward (S = 0) with the extension keywords of _C.rasterize_gaussians_backward."""
    e = torch.Tensor([])
    g = lambda k: dev(kw[k]) if kw.get(k) is not None else e
    P, H, W = kw["means3D"].shape[0], kw["image_height"], kw["image_width"]
    outs = _C.rasterize_gaussians_backward(
        dev(kw["bg"].float()), g("means3D"), res["radii"], g("colors_precomp"), g("scales"), g("rotations"),
        kw.get("scale_modifier", 1.0), g("cov3D_precomp"), g("viewmatrix"), g("projmatrix"), kw["tanfovx"], kw["tanfovy"],
        dev(wts["color"].float()), dev(wts["depth"].float()), dev(wts["alpha"].float()), torch.zeros(0, H, W, device="cuda"),
        g("shs"), kw["sh_degree"], g("campos"), res["geom"], res["R"], res["binning"], res["img"], res["alpha"],
        torch.zeros(P, 0, device="cuda"), True, **extra)
    return dict(zip(GRAD_NAMES, outs))


def jacobian_flag(geomBuffer) -> int:
    """Header word 8 of a forward's geometry buffer: 1 = its preprocess stored the colour Jacobian."""
    return int(_C.geometry_header(geomBuffer)[8])
