"""The sky composite and colour correction of the reference's ``StreetGaussianRenderer.render`` (Step 2,
lib/models/street_gaussian_renderer.py:107-117) as one op: the sky cube-map lookup of ``SkyCubeMap.forward``
(lib/models/sky_cubemap.py:77-123), the composite over the rasterized image, ``ColorCorrection.forward``
(lib/models/color_correction.py:129-132) and the eval clamp, in a few HIP kernels (csrc/sgr_sky.hip, include/sgr_sky.h)
with an autograd backward.  Nothing in the forward or the backward waits on the host.

Tensors must live on the GPU; there is no CPU implementation in the product."""
from __future__ import annotations

import torch

from . import _native
from ._native import call, require_hip

TRAIN, WHITE, CLAMP = 1, 2, 4  # include/sgr_sky.h SGR_SKY_*
SAVED, SCRATCH = 0, 1


class _SkyComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, acc, cube, affine, K, w2c, mask, px, py, flags):
        _, H, W = rgb.shape
        R = cube.shape[-2]
        dev = rgb.device
        L = _native.lib()
        out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        saved = torch.empty(L.sgr_sky_workspace_bytes(H, W, R, 3, SAVED), dtype=torch.uint8, device=dev)
        call("sgr_sky_forward", dev, H, W, R, 3, rgb, acc, cube, K, w2c, mask, px, py, affine, flags, out, saved)
        ctx.save_for_backward(rgb, acc, affine)
        ctx.saved_state = saved
        ctx.flags = flags
        ctx.cube_shape = cube.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        rgb, acc, affine = ctx.saved_tensors
        _, H, W = rgb.shape
        R = ctx.cube_shape[-2]
        dev = rgb.device
        L = _native.lib()
        g = dout.to(torch.float32).contiguous()
        drgb = torch.empty_like(rgb)
        dacc = torch.empty_like(acc)
        dcube = torch.empty(ctx.cube_shape, dtype=torch.float32, device=dev)
        daff = torch.empty(3, 4, dtype=torch.float32, device=dev) if affine is not None else None
        scratch = torch.empty(L.sgr_sky_workspace_bytes(H, W, R, 3, SCRATCH), dtype=torch.uint8, device=dev)
        call("sgr_sky_backward", dev, H, W, R, 3, g, rgb, acc, affine, ctx.flags, ctx.saved_state, drgb, dacc, dcube, daff,
             scratch)
        return drgb, dacc, dcube, daff, None, None, None, None, None, None


def _f32(name, t, shapes):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"composite_sky: {name} must be a tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"composite_sky: {name} must be float32, got {t.dtype}")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"composite_sky: {name} must have shape {' or '.join(str(list(s)) for s in shapes)}, "
                         f"got {list(t.shape)}")


def composite_sky(rgb, acc, cube_map, K, w2c, *, sky_mask=None, train=True, white_background=True, affine=None,
                  clamp_output=False, perturb=None) -> torch.Tensor:
    """Step 2 of ``render()``: ``rgb + sky * (1 - acc)``, colour-corrected by ``affine`` and clamped if asked; returns
    float32 [3, H, W].

    ``rgb`` [3, H, W] and ``acc`` [1, H, W] are the rasterizer's outputs; ``cube_map`` is the learnable [6, R, R, 3]
    (or [1, 6, R, R, 3]) sky map; ``K`` is ``camera.K`` [3, 3]; ``w2c`` is ``camera.world_view_transform.transpose(0, 1)``
    [4, 4].  All float32 on one GPU.  Gradients flow to ``rgb``, ``acc``, ``cube_map`` and ``affine``.

    ``sky_mask`` ([1, H, W] or [H, W] bool): with ``train``, the sky pixels are the mask with its top 50 rows set, as
    ``SkyCubeMap.forward`` does.  The reference writes those rows into ``camera.guidance['sky_mask']`` in place; that
    write is idempotent, so leaving the caller's tensor untouched, as this op does, gives the same results.  Otherwise
    (no mask, or ``train=False``) the sky pixels are those with ``(1 - acc) > 1e-3``, on the detached ``acc``.
    Non-sky pixels take the fill: 1 with ``white_background``, else 0.

    ``affine`` [3, 4] is ``ColorCorrection.get_affine_trans(camera)``; ``None`` means no colour correction.
    ``clamp_output`` is the ``cfg.mode != 'train'`` clamp.

    ``perturb``: with ``train`` and ``None``, two ``torch.rand(H, W)`` images are drawn on ``rgb.device``, x then y,
    exactly as ``get_rays_torch`` draws them, so later random draws stay aligned with the reference's; a [2, H, W]
    float32 tensor is used instead when given (tests).  Without ``train`` the rays go through pixel centres and
    nothing is drawn.  The per-pixel arithmetic is the contract of include/sgr_sky.h."""
    if not isinstance(rgb, torch.Tensor) or rgb.dim() != 3 or rgb.shape[0] != 3:
        raise ValueError(f"composite_sky: rgb must have shape [3, H, W], got "
                         f"{list(rgb.shape) if isinstance(rgb, torch.Tensor) else type(rgb).__name__}")
    _, H, W = rgb.shape
    if H < 1 or W < 1:
        raise ValueError("composite_sky: the image is empty")
    _f32("rgb", rgb, [(3, H, W)])
    _f32("acc", acc, [(1, H, W)])
    if not isinstance(cube_map, torch.Tensor) or cube_map.dim() not in (4, 5):
        raise ValueError("composite_sky: cube_map must have shape [6, R, R, C] or [1, 6, R, R, C]")
    cs = tuple(cube_map.shape[-4:])
    if cube_map.dim() == 5 and cube_map.shape[0] != 1:
        raise ValueError(f"composite_sky: a batched cube_map must have batch 1, got {list(cube_map.shape)}")
    if cs[0] != 6 or cs[1] != cs[2] or cs[1] < 1:
        raise ValueError(f"composite_sky: cube_map must have shape [6, R, R, 3], got {list(cube_map.shape)}")
    if cs[3] != 3:
        raise ValueError(f"composite_sky: only C = 3 channels are supported, got C = {cs[3]}")
    _f32("cube_map", cube_map, [tuple(cube_map.shape)])
    _f32("K", K, [(3, 3)])
    _f32("w2c", w2c, [(4, 4)])
    if affine is not None:
        _f32("affine", affine, [(3, 4)])
    if sky_mask is not None:
        if not isinstance(sky_mask, torch.Tensor) or sky_mask.dtype != torch.bool:
            raise TypeError("composite_sky: sky_mask must be a bool tensor")
        if tuple(sky_mask.shape) not in ((1, H, W), (H, W)):
            raise ValueError(f"composite_sky: sky_mask must have shape [1, H, W] or [H, W], got {list(sky_mask.shape)}")
    if perturb is not None and train:
        _f32("perturb", perturb, [(2, H, W)])
    tensors = [rgb, acc, cube_map, K, w2c] + [t for t in (affine, sky_mask, perturb if train else None) if t is not None]
    require_hip("composite_sky: every tensor must be a HIP (cuda) tensor: there is no CPU path", *tensors)
    dev = rgb.device
    if any(t.device != dev for t in tensors):
        raise ValueError("composite_sky: every tensor must be on the same device")

    flags = (TRAIN if train else 0) | (WHITE if white_background else 0) | (CLAMP if clamp_output else 0)
    mask = sky_mask.reshape(H, W).contiguous().view(torch.uint8) if (sky_mask is not None and train) else None
    px = py = None
    if train:
        if perturb is None:  # get_rays_torch's two draws, in its order
            px = torch.rand(H, W, device=dev)
            py = torch.rand(H, W, device=dev)
        else:
            px, py = perturb[0].contiguous(), perturb[1].contiguous()
    return _SkyComposite.apply(rgb.contiguous(), acc.contiguous(), cube_map.contiguous(),
                               affine.contiguous() if affine is not None else None, K.detach().contiguous(),
                               w2c.detach().contiguous(), mask, px, py, flags)
