"""Cube-map ``texture()`` of nvdiffrast, restricted to what the reference's sky model calls
(lib/models/sky_cubemap.py:99-120 and :178-191): ``boundary_mode='cube'``, bilinear filtering, the gradient with respect
to the texture.  One HIP forward kernel, and a deterministic backward (key, sort, gather: csrc/sgr_texture.hip) that
writes every element of the texture gradient once, with no float atomics.  ``import nvdiffrast.torch as dr`` resolves
here through the ``nvdiffrast`` drop-in package.

Tensors must live on the GPU; there is no CPU implementation in the product."""
from __future__ import annotations

import torch

from . import _native
from ._native import call, require_hip


class _TextureCube(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv):
        Bt, _, R, _, Cc = tex.shape
        B, H, W, _ = uv.shape
        dev = tex.device
        out = torch.empty(B, H, W, Cc, dtype=torch.float32, device=dev)
        call("sgr_texture_cube_forward", dev, Bt, B, R, Cc, H * W, tex, uv, out)
        ctx.save_for_backward(uv)
        ctx.tex_shape = tex.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        (uv,) = ctx.saved_tensors
        Bt, _, R, _, Cc = ctx.tex_shape
        B, H, W, _ = uv.shape
        dev = uv.device
        L = _native.lib()
        up = dout.to(torch.float32).contiguous()
        grad = torch.empty(ctx.tex_shape, dtype=torch.float32, device=dev)
        work = torch.empty(L.sgr_texture_cube_workspace_bytes(Bt, B, R, Cc, H * W), dtype=torch.uint8, device=dev)
        call("sgr_texture_cube_backward", dev, Bt, B, R, Cc, H * W, uv, up, grad, work)
        return grad, None


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap",
            max_mip_level=None):
    """nvdiffrast.torch.texture for cube maps: ``tex`` float32 [Bt, 6, R, R, C] (Bt = 1 or B), ``uv`` float32
    [B, H, W, 3] direction vectors (need not be normalised) -> float32 [B, H, W, C], bilinear.

    Supported: ``boundary_mode='cube'`` with ``filter_mode='linear'``, or ``'auto'`` without ``uv_da`` /
    ``mip_level_bias`` (which nvdiffrast resolves to linear); ``max_mip_level`` only matters to the mipmap modes and is
    ignored, as nvdiffrast ignores it.  Every other mode or argument raises NotImplementedError, as does a ``uv`` that
    needs a gradient (the sky model's ray directions never do).  The gradient flows to ``tex``."""
    del max_mip_level
    if boundary_mode != "cube":
        raise NotImplementedError(f"texture: boundary_mode={boundary_mode!r} is not implemented, only 'cube'")
    if uv_da is not None:
        raise NotImplementedError("texture: uv_da (mipmapped filtering) is not implemented")
    if mip_level_bias is not None:
        raise NotImplementedError("texture: mip_level_bias (mipmapped filtering) is not implemented")
    if mip is not None:
        raise NotImplementedError("texture: mip (prebuilt mipmap stacks) is not implemented")
    if filter_mode not in ("auto", "linear"):
        raise NotImplementedError(f"texture: filter_mode={filter_mode!r} is not implemented, only 'linear' (or 'auto')")
    if tex.dtype != torch.float32 or uv.dtype != torch.float32:
        raise NotImplementedError("texture: tex and uv must be float32")
    if uv.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("texture: the gradient with respect to uv (the directions) is not implemented; "
                                  "pass uv.detach()")
    if tex.dim() != 5 or tex.shape[1] != 6 or tex.shape[2] != tex.shape[3] or tex.shape[2] < 1 or tex.shape[4] < 1:
        raise ValueError(f"texture: a cube map must have shape [Bt, 6, R, R, C], got {list(tex.shape)}")
    if uv.dim() != 4 or uv.shape[3] != 3:
        raise ValueError(f"texture: cube-map directions must have shape [B, H, W, 3], got {list(uv.shape)}")
    if tex.shape[0] not in (1, uv.shape[0]):
        raise ValueError(f"texture: tex batch {tex.shape[0]} must be 1 or the uv batch {uv.shape[0]}")
    require_hip("texture: tex and uv must be HIP (cuda) tensors: there is no CPU path", tex, uv)
    if tex.device != uv.device:
        raise ValueError("texture: tex and uv must be on the same device")
    return _TextureCube.apply(tex.contiguous(), uv.detach().contiguous())
