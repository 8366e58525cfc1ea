"""The sky composite and colour correction of the reference's ``StreetGaussianRenderer.render`` (Step 2,
lib/models/street_gaussian_renderer.py:107-117) as one op: the sky cube-map lookup of ``SkyCubeMap.forward``
(lib/models/sky_cubemap.py:77-123), the composite over the rasterized image, ``ColorCorrection.forward``
(lib/models/color_correction.py:129-132) and the eval clamp, in a few HIP kernels (csrc/sgr_sky.hip, include/sgr_sky.h)
with an autograd backward.  Nothing in the forward or the backward waits on the host.  ``SkyAdam`` is the sky model's
optimiser (``SkyCubeMap.training_setup`` / ``update_optimizer``): the cube map's gradient gather and the Adam step in one
kernel over the part of the map that has ever been touched (include/sgr_sky_step.h).

Tensors must live on the GPU; there is no CPU implementation in the product."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _alloc, _native
from ._native import call, launch, require_hip
from .optim import CHUNK_DTYPE, RECORD_DTYPE, _group_defaults, _pinned_to, bias_corrections

TRAIN, WHITE, CLAMP = 1, 2, 4  # include/sgr_sky.h SGR_SKY_*
SAVED, SCRATCH, SCRATCH_DEFERRED = 0, 1, 2


class _SkyComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, acc, cube, affine, K, w2c, mask, px, py, flags, sink):
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
        ctx.sink = sink
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
        daff = torch.empty(3, 4, dtype=torch.float32, device=dev) if affine is not None else None
        sink = ctx.sink
        if sink is not None:  # the cube map's gradient stays in the sink's workspace: SkyAdam.step() gathers it
            work = sink._begin_backward(H, W, dev)
            scratch = torch.empty(L.sgr_sky_workspace_bytes(H, W, R, 3, SCRATCH_DEFERRED), dtype=torch.uint8, device=dev)
            call("sgr_sky_backward_deferred", dev, H, W, R, 3, g, rgb, acc, affine, ctx.flags, ctx.saved_state, drgb, dacc,
                 work, sink.active, daff, scratch)
            sink._end_backward(dev)
            return drgb, dacc, None, daff, None, None, None, None, None, None, None
        dcube = torch.empty(ctx.cube_shape, dtype=torch.float32, device=dev)
        scratch = torch.empty(L.sgr_sky_workspace_bytes(H, W, R, 3, SCRATCH), dtype=torch.uint8, device=dev)
        call("sgr_sky_backward", dev, H, W, R, 3, g, rgb, acc, affine, ctx.flags, ctx.saved_state, drgb, dacc, dcube, daff,
             scratch)
        return drgb, dacc, dcube, daff, None, None, None, None, None, None, None


def _f32(name, t, shapes):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"composite_sky: {name} must be a tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"composite_sky: {name} must be float32, got {t.dtype}")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"composite_sky: {name} must have shape {' or '.join(str(list(s)) for s in shapes)}, "
                         f"got {list(t.shape)}")


def composite_sky(rgb, acc, cube_map, K, w2c, *, sky_mask=None, train=True, white_background=True, affine=None,
                  clamp_output=False, perturb=None, cube_sink=None) -> torch.Tensor:
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
    nothing is drawn.  The per-pixel arithmetic is the contract of include/sgr_sky.h.

    ``cube_sink`` (``SkyAdam.sink()``): the backward then leaves the cube map's gradient in the optimiser's workspace
    instead of materialising it -- ``cube_map.grad`` stays ``None`` and ``SkyAdam.step()`` applies it; every other
    gradient is bit-identical.  ``cube_map`` must be the optimiser's own parameter.  One backward per step: a second
    one into a sink that still holds a gradient raises ``RuntimeError``."""
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

    if cube_sink is not None:
        if not isinstance(cube_sink, SkyAdam):
            raise TypeError("composite_sky: cube_sink must be a SkyAdam.sink()")
        own = cube_sink.cube_map
        if cube_map.data_ptr() != own.data_ptr() or cube_map.shape != own.shape or not cube_map.is_contiguous():
            raise ValueError("composite_sky: with cube_sink, cube_map must be the optimiser's own parameter "
                             f"(shape {list(own.shape)}, the same storage)")

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
                               w2c.detach().contiguous(), mask, px, py, flags, cube_sink)


# ---- the cube map's optimiser -----------------------------------------------------------------------------------------
def adam_scalars(lr: float, step: int, betas=(0.9, 0.999)):
    """(step_size, bc2_sqrt) of include/sgr_optim.h as the float32 values the kernel receives: ``-(lr / bc1)`` and
    ``(1 - beta2 ** step) ** 0.5`` in double, as torch's Python computes them, rounded once."""
    bc1, bc2_sqrt = bias_corrections(step, float(betas[0]), float(betas[1]))
    return C.c_float(-(lr / bc1)).value, C.c_float(bc2_sqrt).value


class SkyAdam:
    """``torch.optim.Adam(eps=1e-15)`` over the sky cube map (the reference's ``SkyCubeMap.training_setup``,
    lib/models/sky_cubemap.py:53-75), bit for bit, without a dense gradient and without touching the texels that no sky
    pixel has ever reached (include/sgr_sky_step.h).

    ``cube_map`` is the [6, R, R, 3] float32 leaf -- for the reference's module, its very ``sky_cube_map`` Parameter.
    Per iteration::

        out = composite_sky(..., cube_map, ..., cube_sink=opt.sink())
        loss.backward()                      # the cube map's gradient stays in the optimiser's workspace
        opt.lr = scheduler(iteration)        # update_learning_rate
        opt.step()                           # update_optimizer: one launch, over the blocks ever touched

    A texel that has once received a gradient keeps moving while its moments decay, so a block (256 texels) is stepped
    from its first gradient on; an untouched element (g = m = v = 0) is left bitwise unchanged by Adam's arithmetic,
    which is why skipping it changes nothing.  That needs ``eps > 0`` (in float32) and ``lr >= 0``; anything else is
    refused.  Without the sink (``cube_map.grad`` set by a plain backward) ``step()`` takes the dense path through
    ``sgr_adam_step`` and marks every block.  Nothing but ``active_fraction()`` waits on the host."""

    def __init__(self, cube_map: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-15):
        if not isinstance(cube_map, torch.Tensor) or cube_map.dim() != 4 or cube_map.shape[0] != 6 or \
                cube_map.shape[1] != cube_map.shape[2] or cube_map.shape[1] < 1 or cube_map.shape[3] != 3:
            raise ValueError("SkyAdam: cube_map must have shape [6, R, R, 3]")
        if cube_map.dtype != torch.float32 or not cube_map.is_contiguous():
            raise ValueError("SkyAdam: cube_map must be a contiguous float32 tensor")
        require_hip("SkyAdam needs a HIP (cuda) tensor: there is no CPU path", cube_map)
        beta1, beta2 = float(betas[0]), float(betas[1])
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"SkyAdam: betas must lie in [0, 1), got {betas}")
        if not C.c_float(eps).value > 0.0:
            raise ValueError(f"SkyAdam: eps must be positive in float32, got {eps} (with eps = 0 an untouched element is "
                             "0 / 0: the dense step it stands for would not leave it alone)")
        self.cube_map = cube_map
        self.lr = float(lr)
        self.betas = (beta1, beta2)
        self.eps = float(eps)
        self.step_count = 0
        self.R = int(cube_map.shape[1])
        self.block = int(_native.lib().sgr_sky_step_block_texels())
        self.n_blocks = (6 * self.R * self.R + self.block - 1) // self.block
        dev = cube_map.device
        self.exp_avg = torch.zeros_like(cube_map, memory_format=torch.contiguous_format).detach()
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.active = torch.zeros(self.n_blocks, dtype=torch.uint8, device=dev)
        self._work = None      # the deferred-gradient workspace, grown along _alloc's ladder
        self._pending = None   # the stream handle of the backward whose gradient the workspace holds
        self._chunks = None    # the dense path's one-chunk table
        self._chunks_key = None

    def sink(self) -> "SkyAdam":
        """What ``composite_sky(..., cube_sink=)`` takes."""
        return self

    # ---- the sink's side: called by the backward of composite_sky ---------------------------------------------------
    def _begin_backward(self, H: int, W: int, dev) -> torch.Tensor:
        if self._pending is not None:
            raise RuntimeError("SkyAdam: the sink already holds the gradient of a backward that has not been stepped "
                               "(step() or discard() first; accumulating several frames is not implemented)")
        need = int(_native.lib().sgr_sky_step_workspace_bytes(H, W, self.R))
        if need == 0:
            raise ValueError(f"SkyAdam: no workspace for a {H} x {W} frame at R = {self.R}")
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(_alloc.ladder(need), dtype=torch.uint8, device=dev)
        return self._work

    def _end_backward(self, dev) -> None:
        self._pending = torch.cuda.current_stream(dev).cuda_stream

    # ---- the optimiser's side ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self) -> None:
        """One Adam step with the gradient of the last backward, on the stream that backward ran on."""
        p = self.cube_map
        grad = p.grad
        if self._pending is not None and grad is not None:
            raise ValueError("SkyAdam.step: both a pending sink gradient and cube_map.grad are set")
        if self._pending is None and grad is None:
            return  # as torch's Adam skips a parameter without a gradient: no decay, no move, no step
        if not (self.lr >= 0.0 and self.lr != float("inf")):
            raise ValueError(f"SkyAdam.step: lr must be finite and >= 0, got {self.lr}")
        if p.shape != self.exp_avg.shape or not p.is_contiguous():
            raise ValueError("SkyAdam.step: cube_map changed its shape or layout")
        dev = p.device
        here = torch.cuda.current_stream(dev).cuda_stream
        step = self.step_count + 1
        ss, bc2s = adam_scalars(self.lr, step, self.betas)
        if self._pending is not None:
            if self._pending != here:
                raise ValueError("SkyAdam.step: the current stream is not the one the backward ran on")
            call("sgr_sky_adam_step", dev, self.R, p, self.exp_avg, self.exp_avg_sq, self._work, self.active, ss, bc2s,
                 self.eps, self.betas[0], self.betas[1])
            self._pending = None
        else:
            if grad.layout != torch.strided or grad.dtype != torch.float32 or grad.shape != p.shape or grad.device != dev:
                raise ValueError("SkyAdam.step: cube_map.grad must be a dense float32 tensor shaped like cube_map")
            g = grad if grad.is_contiguous() else grad.contiguous()
            span = int(_native.lib().sgr_adam_span_elems())
            n = p.numel()
            rec = np.zeros(1, dtype=RECORD_DTYPE)
            rec["g"], rec["step_size"], rec["bc2_sqrt"], rec["eps"] = g.data_ptr(), ss, bc2s, self.eps
            with torch.cuda.device(dev):
                key = (p.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr())
                if self._chunks is None or self._chunks_key != key:
                    tab = np.zeros(1, dtype=CHUNK_DTYPE)
                    tab["p"], tab["m"], tab["v"], tab["count"] = key[0], key[1], key[2], n
                    self._chunks, self._chunks_key = _pinned_to(tab, dev), key
                launch("sgr_adam_step", _native.stream(dev), self._chunks, 1, _pinned_to(rec, dev), 1,
                       (n + span - 1) // span, self.betas[0], self.betas[1])
            self.active.fill_(1)  # a dense gradient may be non-zero anywhere
        self.step_count = step

    def discard(self) -> None:
        """Drops the gradient of a backward that will not be stepped (the blocks it marked stay marked)."""
        self._pending = None

    def zero_grad(self, set_to_none: bool = True) -> None:
        """``cube_map.grad = None`` (the dense path's gradient; a sink gradient is consumed by ``step()``)."""
        self.cube_map.grad = None

    def active_fraction(self) -> float:
        """The share of blocks that are stepped.  Waits on the host."""
        return float(self.active.float().mean().item())

    def _nonzero_blocks(self) -> torch.Tensor:
        nz = ((self.exp_avg != 0) | (self.exp_avg_sq != 0)).view(-1, 3).any(1)
        nz = torch.nn.functional.pad(nz, (0, self.n_blocks * self.block - nz.numel()))
        return nz.view(self.n_blocks, self.block).any(1).to(torch.uint8)

    # ---- state -------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """``torch.optim.Adam.state_dict()``'s layout with the reference's one group (``name='sky_cube_map'``), as it
        saves it under ``state_dict['optimizer']`` (sky_cubemap.py:36-46); the moments are copies."""
        group = dict(_group_defaults(self.betas, self.eps), lr=self.lr, name="sky_cube_map", params=[0])
        state = {}
        if self.step_count > 0:
            state[0] = {"step": torch.tensor(float(self.step_count), dtype=torch.float32),
                        "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone()}
        return {"state": state, "param_groups": [group]}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """Restores learning rate, step count and moments from a ``torch.optim.Adam.state_dict()`` over the one
        parameter, and rebuilds the activity map from the non-zero moments.  A pending gradient is dropped."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != 1:
            raise ValueError("SkyAdam.load_state_dict: expected one param group with one parameter")
        pg = groups[0]
        if tuple(float(b) for b in pg.get("betas", self.betas)) != self.betas or float(pg.get("eps", self.eps)) != self.eps:
            raise ValueError(f"SkyAdam.load_state_dict: betas / eps {pg.get('betas')} / {pg.get('eps')}, this optimiser "
                             f"{self.betas} / {self.eps}")
        for name, default in (("weight_decay", 0), ("amsgrad", False), ("maximize", False)):
            if pg.get(name, default) != default:
                raise NotImplementedError(f"SkyAdam.load_state_dict: {name}={pg[name]!r} is not implemented")
        st = sd["state"].get(pg["params"][0])
        if st is None:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.step_count = 0
        else:
            for dst, key in ((self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
                src = st[key]
                if src.numel() != dst.numel():
                    raise ValueError(f"SkyAdam.load_state_dict: {key} has {src.numel()} elements, the map {dst.numel()}")
                dst.copy_(src.detach().to(device=dst.device, dtype=torch.float32).reshape(dst.shape))
            self.step_count = int(float(st["step"]))
        self.lr = float(pg["lr"])
        self.active = self._nonzero_blocks()
        self._pending = None
