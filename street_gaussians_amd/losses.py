"""Drop-in `l1_loss` and `ssim` for /root/reference/lib/utils/loss_utils.py:21-37 and :80-125:
same names, arguments and results, each backed by one forward and one backward HIP kernel (csrc/sgr_loss.hip) instead
of ~30 MIOpen / elementwise launches.  `train.py:100-104` keeps its two lines; only the import changes:

    from street_gaussians_amd.losses import l1_loss, ssim

`frame_loss` is all of `train.py:100-133` as one op (csrc/sgr_frame_loss.hip): one backward kernel for the four image
gradients and one device tensor with every scalar the loop logs; `psnr` is loss_utils.py:61-78 without its host wait.
`semantic_loss` is the cross-entropy on the rendered semantic head (csrc/sgr_semantic_loss.hip), the term the reference
renders for (`lambda_semantic`) and leaves to the trainer.

Tensors must live on the GPU; there is no CPU implementation in the product."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _native
from ._native import call, require_hip


def _prep(img, name):
    require_hip(f"{name} must be a HIP (cuda) tensor: there is no CPU path", img)
    if img.dim() == 4:
        img = img.reshape(-1, img.shape[-2], img.shape[-1])
    if img.dim() != 3:
        raise RuntimeError(f"{name} must have dimensions (C, H, W)")
    return img.to(torch.float32).contiguous()


def _prep_mask(mask, H, W):
    if mask is None:
        return None
    m = mask.reshape(-1, H, W)
    if m.shape[0] != 1:
        raise RuntimeError("mask must have dimensions (1, H, W)")
    return m[0].to(torch.uint8).contiguous()


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, mask):
        L = _native.lib()
        Cc, H, W = img1.shape
        dev = img1.device
        need = img1.requires_grad
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(L.sgr_ssim_workspace_floats(Cc, H, W), dtype=torch.float32, device=dev)
        partials = torch.empty(3 * Cc * H * W, dtype=torch.float32, device=dev) if need else None
        call("sgr_ssim_forward", dev, Cc, H, W, img1, img2, mask, out, partials, ws)
        ctx.save_for_backward(img1, img2, mask if mask is not None else torch.empty(0, device=dev), partials
                              if partials is not None else torch.empty(0, device=dev))
        ctx.has_mask = mask is not None
        return out[0]

    @staticmethod
    def backward(ctx, upstream):
        img1, img2, mask, partials = ctx.saved_tensors
        Cc, H, W = img1.shape
        dev = img1.device
        if partials.numel() == 0:
            raise RuntimeError("ssim forward ran without requires_grad")
        up = upstream.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(img1)
        call("sgr_ssim_backward", dev, Cc, H, W, img1, img2, mask if ctx.has_mask else None, partials, up, grad)
        return grad, None, None


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mask):
        L = _native.lib()
        Cc, H, W = a.shape
        dev = a.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        ws = torch.empty(L.sgr_l1_workspace_floats(Cc, H, W), dtype=torch.float32, device=dev)
        call("sgr_l1_forward", dev, Cc, H, W, a, b, mask, out, ws)
        ctx.save_for_backward(a, b, mask if mask is not None else torch.empty(0, device=dev), out)
        ctx.has_mask = mask is not None
        return out[0]

    @staticmethod
    def backward(ctx, upstream):
        a, b, mask, out = ctx.saved_tensors
        Cc, H, W = a.shape
        dev = a.device
        up = upstream.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(a)
        call("sgr_l1_backward", dev, Cc, H, W, a, b, mask if ctx.has_mask else None, out, up, grad)
        return grad, None, None


class _BCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acc, mask, mode):
        L = _native.lib()
        dev, n = acc.device, acc.numel()
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(L.sgr_l1_workspace_floats(1, 1, 1), dtype=torch.float32, device=dev)
        call("sgr_bce_forward", dev, n, mode, acc, mask, out, ws)
        ctx.save_for_backward(acc, mask)
        ctx.mode = mode
        return out[0]

    @staticmethod
    def backward(ctx, upstream):
        acc, mask = ctx.saved_tensors
        dev = acc.device
        up = upstream.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(acc)
        call("sgr_bce_backward", dev, acc.numel(), ctx.mode, acc, mask, up, grad)
        return grad, None, None


class _Lidar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, acc, lidar, mask, keep):
        L = _native.lib()
        dev, n = depth.device, depth.numel()
        out = torch.empty(4, dtype=torch.float32, device=dev)
        work = torch.empty(L.sgr_lidar_work_bytes(n), dtype=torch.uint8, device=dev)
        call("sgr_lidar_depth_forward", dev, n, depth, acc, lidar, mask, float(keep), out, work)
        ctx.save_for_backward(depth, acc, lidar, out, work)
        return out[0]

    @staticmethod
    def backward(ctx, upstream):
        depth, acc, lidar, out, work = ctx.saved_tensors
        dev = depth.device
        up = upstream.reshape(1).to(torch.float32).contiguous()
        gd, ga = torch.empty_like(depth), torch.empty_like(acc)
        call("sgr_lidar_depth_backward", dev, depth.numel(), depth, acc, lidar, out, work, up, gd, ga)
        return gd, ga, None, None, None


def _flat(t, name, like=None):
    require_hip(f"{name} must be a HIP (cuda) tensor: there is no CPU path", t)
    if like is not None and t.numel() != like.numel():
        raise RuntimeError(f"{name} must have as many elements as the rendered map")
    return t.to(torch.float32).contiguous()


def _flat_mask(m, like):
    if m is None:
        return None
    if m.numel() != like.numel():
        raise RuntimeError("mask must have as many elements as the rendered map")
    return m.to(torch.uint8).contiguous()


def sky_loss(acc: torch.Tensor, sky_mask: torch.Tensor) -> torch.Tensor:
    """train.py:107-109: clamp(acc, 1e-6, 1-1e-6), then mean of -log(1-acc) on sky pixels and -log(acc) elsewhere."""
    a = _flat(acc, "acc")
    return _BCE.apply(a, _flat_mask(sky_mask, a), 0)


def obj_acc_loss(acc_obj: torch.Tensor, obj_bound: torch.Tensor) -> torch.Tensor:
    """train.py:116-121: entropy of the clamped object accumulation inside the boxes, -log(1-acc) outside, mean."""
    a = _flat(acc_obj, "acc_obj")
    return _BCE.apply(a, _flat_mask(obj_bound, a), 1)


def lidar_depth_loss(depth: torch.Tensor, acc: torch.Tensor, lidar_depth: torch.Tensor, mask: Optional[torch.Tensor] = None,
                     keep: float = 0.95) -> torch.Tensor:
    """train.py:124-131: mean of the int(keep * n) smallest |depth / (acc + 1e-10) - lidar_depth| over the n pixels
    with lidar_depth > 0 and mask.  Gradients flow to depth and acc."""
    d = _flat(depth, "depth")
    return _Lidar.apply(d, _flat(acc, "acc", d), _flat(lidar_depth, "lidar_depth", d).detach(), _flat_mask(mask, d), keep)


class _ColorLoss(torch.autograd.Function):
    """(1 - lambda_dssim) * lambda_l1 * l1_loss + lambda_dssim * (1 - ssim)   (train.py:100-104) as one op: the two
    forward kernels, then ONE backward kernel that writes dL/dimage -- the upstream gradient the rasterizer's backward
    reads -- without materialising the two per-term gradient images and their sum."""

    @staticmethod
    def forward(ctx, img, gt, mask, lambda_dssim, lambda_l1):
        L = _native.lib()
        Cc, H, W = img.shape
        dev = img.device
        out_s = torch.empty(1, dtype=torch.float32, device=dev)
        out_l = torch.empty(2, dtype=torch.float32, device=dev)
        ws = torch.empty(max(L.sgr_ssim_workspace_floats(Cc, H, W), L.sgr_l1_workspace_floats(Cc, H, W)),
                         dtype=torch.float32, device=dev)
        partials = torch.empty(3 * Cc * H * W, dtype=torch.float32, device=dev) if img.requires_grad else None
        call("sgr_l1_forward", dev, Cc, H, W, img, gt, mask, out_l, ws)
        call("sgr_ssim_forward", dev, Cc, H, W, img, gt, mask, out_s, partials, ws)
        ctx.save_for_backward(img, gt, mask if mask is not None else torch.empty(0, device=dev),
                              partials if partials is not None else torch.empty(0, device=dev), out_l)
        ctx.has_mask = mask is not None
        ctx.w_l1, ctx.w_ssim = (1.0 - float(lambda_dssim)) * float(lambda_l1), -float(lambda_dssim)
        loss = ctx.w_l1 * out_l[0] + float(lambda_dssim) * (1.0 - out_s[0])
        ctx.mark_non_differentiable(out_l)
        return loss, out_l

    @staticmethod
    def backward(ctx, upstream, _unused):
        img, gt, mask, partials, out_l = ctx.saved_tensors
        Cc, H, W = img.shape
        dev = img.device
        if partials.numel() == 0:
            raise RuntimeError("color_loss forward ran without requires_grad")
        up = upstream.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(img)
        call("sgr_color_loss_backward", dev, Cc, H, W, img, gt, mask if ctx.has_mask else None, partials, out_l, ctx.w_l1,
             ctx.w_ssim, up, grad)
        return grad, None, None, None, None


def color_loss(image: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, lambda_dssim: float = 0.2,
               lambda_l1: float = 1.0, return_l1: bool = False):
    """train.py:100-104 in one op: ``(1 - lambda_dssim) * lambda_l1 * l1_loss(image, gt, mask) + lambda_dssim *
    (1 - ssim(image, gt, mask=mask))``; its backward is a single kernel producing dL/dimage for the rasterizer.
    With ``return_l1`` also returns the (detached) L1 term train.py logs (``scalar_dict['l1_loss']``)."""
    a, b = _prep(image, "image"), _prep(gt, "gt")
    if a.shape != b.shape:
        raise RuntimeError("image and gt must have the same shape")
    loss, out_l = _ColorLoss.apply(a, b.detach(), _prep_mask(mask, a.shape[1], a.shape[2]), lambda_dssim, lambda_l1)
    return (loss, out_l[0]) if return_l1 else loss


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """loss_utils.py:21-37: mean |network_output - gt| over the C values of the pixels selected by mask (1, H, W)."""
    a, b = _prep(network_output, "network_output"), _prep(gt, "gt")
    if a.shape != b.shape:
        raise RuntimeError("network_output and gt must have the same shape")
    return _L1.apply(a, b.detach(), _prep_mask(mask, a.shape[1], a.shape[2]))


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True,
         mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """loss_utils.py:80-125: mean SSIM (11x11 Gaussian window, sigma 1.5, zero padding), both images zeroed where the
    mask is False.  Gradient flows to img1 only (the ground truth is data)."""
    if window_size != 11 or not size_average:
        raise NotImplementedError("only window_size=11, size_average=True (the values train.py uses) are implemented")
    a, b = _prep(img1, "img1"), _prep(img2, "img2")
    if a.shape != b.shape:
        raise RuntimeError("img1 and img2 must have the same shape")
    return _SSIM.apply(a, b.detach(), _prep_mask(mask, a.shape[1], a.shape[2]))


# ---- every image-space term of a training step in one op (include/sgr_frame_loss.h) -----------------------------------
class _FrameLossArgs(C.Structure):
    """sgr_frame_loss_args: host memory read during the call."""
    _fields_ = [(n, C.c_void_p) for n in ("image", "gt", "mask", "acc", "sky_mask", "acc_obj", "obj_bound", "depth",
                                          "lidar_depth")] + \
               [(n, C.c_float) for n in ("w_l1", "lambda_dssim", "lambda_sky", "sky_scale", "lambda_reg",
                                         "lambda_depth_lidar")] + [("keep", C.c_double)]


class FrameTerms(NamedTuple):
    """The scalars train.py logs, as 0-dim views of ``values`` (8 floats on the device, include/sgr_frame_loss.h's
    enum order): ``values.tolist()`` is the one read-back a logger needs.  A term that is off reads 0."""
    l1: torch.Tensor
    ssim: torch.Tensor
    sky: torch.Tensor
    obj: torch.Tensor
    lidar: torch.Tensor
    mse: torch.Tensor
    psnr: torch.Tensor
    loss: torch.Tensor
    values: torch.Tensor


class _FrameLoss(torch.autograd.Function):
    """train.py:100-133 as one op: the map kernel, the LiDAR select and one finishing workgroup forward, ONE kernel
    backward that writes dL/dimage, dL/dacc, dL/ddepth and dL/dacc_obj -- the four images the rasterizer's backward
    reads -- for whichever of the inputs require grad."""

    @staticmethod
    def forward(ctx, image, acc, depth, acc_obj, gt, mask, sky_mask, obj_bound, lidar, scalars):
        L = _native.lib()
        Cc, H, W = image.shape
        dev = image.device
        tensors = (image, gt, mask, acc, sky_mask, acc_obj, obj_bound, depth, lidar)
        args = _FrameLossArgs(*[None if t is None else t.data_ptr() for t in tensors], *scalars)
        values = torch.empty(8, dtype=torch.float32, device=dev)
        saved = torch.empty(L.sgr_frame_loss_saved_bytes(Cc, H, W), dtype=torch.uint8, device=dev)
        ws = torch.empty(L.sgr_frame_loss_workspace_floats(Cc, H, W), dtype=torch.float32, device=dev)
        call("sgr_frame_loss_forward", dev, Cc, H, W, C.addressof(args), values, saved, ws)
        ctx.save_for_backward(*tensors, saved, values)
        ctx.scalars = scalars
        ctx.mark_non_differentiable(values)
        return values[7], values

    @staticmethod
    def backward(ctx, upstream, _unused):
        *tensors, saved, values = ctx.saved_tensors
        image, gt, mask, acc, sky_mask, acc_obj, obj_bound, depth, lidar = tensors
        Cc, H, W = image.shape
        dev = image.device
        args = _FrameLossArgs(*[None if t is None else t.data_ptr() for t in tensors], *ctx.scalars)
        up = upstream.reshape(1).to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        grads = [torch.empty_like(t) if n and t is not None else None for t, n in zip((image, acc, depth, acc_obj), need)]
        call("sgr_frame_loss_backward", dev, Cc, H, W, C.addressof(args), values, saved, None, up, grads[0],
             grads[1], grads[2], grads[3])
        return (*grads, None, None, None, None, None, None)


def _pair(a, b, names):
    if (a is None) != (b is None):
        raise ValueError(f"{names[0]} and {names[1]} go together: pass both or neither")
    return a is not None


def frame_loss(image: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, *, lambda_dssim: float = 0.2,
               lambda_l1: float = 1.0, acc: Optional[torch.Tensor] = None, sky_mask: Optional[torch.Tensor] = None,
               lambda_sky: float = 0.0, sky_scale: float = 1.0, acc_obj: Optional[torch.Tensor] = None,
               obj_bound: Optional[torch.Tensor] = None, lambda_reg: float = 0.0, depth: Optional[torch.Tensor] = None,
               lidar_depth: Optional[torch.Tensor] = None, lambda_depth_lidar: float = 0.0, keep: float = 0.95):
    """train.py:100-133 in one op -> ``(loss, terms)``.

    ``loss`` (0-dim) = ``(1 - lambda_dssim) * lambda_l1 * l1 + lambda_dssim * (1 - ssim)`` ``+ lambda_sky * sky``
    (``acc`` with ``sky_mask``; ``sky_scale`` = ``lambda_sky_scale[cam]``) ``+ lambda_reg * obj`` (``acc_obj`` with
    ``obj_bound``) ``+ lambda_depth_lidar * lidar`` (``depth`` with ``lidar_depth``; needs ``acc``, read unclamped).  A
    term is on exactly when both tensors of its pair are passed.  It is differentiable with respect to ``image``,
    ``acc``, ``depth`` and ``acc_obj``; ``loss.backward()`` is one kernel.  ``terms`` (FrameTerms) holds the scalars
    train.py logs, plus mse and psnr, on the device: nothing here waits on the host."""
    obj = _pair(acc_obj, obj_bound, ("acc_obj", "obj_bound"))
    lidar = _pair(depth, lidar_depth, ("depth", "lidar_depth"))
    if lidar and acc is None:
        raise ValueError("depth and lidar_depth need acc: the LiDAR term divides by it")
    # acc serves the sky term and the LiDAR term: alone it is half a pair
    sky = sky_mask is not None if lidar and acc is not None else _pair(acc, sky_mask, ("acc", "sky_mask"))
    a, b = _prep(image, "image"), _prep(gt, "gt")
    if a.shape != b.shape:
        raise RuntimeError("image and gt must have the same shape")
    H, W = a.shape[1], a.shape[2]
    like = a[0]
    m = _prep_mask(mask, H, W)
    t_acc = _flat(acc, "acc", like) if acc is not None else None
    t_sky = _flat_mask(sky_mask, like) if sky else None
    t_obj = _flat(acc_obj, "acc_obj", like) if obj else None
    t_bound = _flat_mask(obj_bound, like) if obj else None
    t_depth = _flat(depth, "depth", like) if lidar else None
    t_lidar = _flat(lidar_depth, "lidar_depth", like).detach() if lidar else None
    for name, t in (("mask", m), ("sky_mask", t_sky), ("obj_bound", t_bound)):
        if t is not None:
            require_hip(f"{name} must be a HIP (cuda) tensor: there is no CPU path", t)
    scalars = ((1.0 - float(lambda_dssim)) * float(lambda_l1), float(lambda_dssim), float(lambda_sky), float(sky_scale),
               float(lambda_reg), float(lambda_depth_lidar), float(keep))
    loss, values = _FrameLoss.apply(a, t_acc, t_depth, t_obj, b.detach(), m, t_sky, t_bound, t_lidar, scalars)
    return loss, FrameTerms(*values.unbind(0), values)


def psnr(img1: torch.Tensor, img2: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """loss_utils.py:61-78: ``20 * log10(1 / sqrt(mean((img1 - img2) ** 2)))`` over the C values of the pixels selected
    by mask (1, H, W), as a 0-dim tensor -- without the host wait of the reference's ``img[mask]``.  A metric, not a
    loss: with grad mode on, an input that requires grad is refused instead of silently dropping its graph."""
    if torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad):
        raise ValueError("psnr is not differentiable: call it under torch.no_grad() or detach its inputs")
    a, b = _prep(img1, "img1"), _prep(img2, "img2")
    if a.shape != b.shape:
        raise RuntimeError("img1 and img2 must have the same shape")
    Cc, H, W = a.shape
    dev = a.device
    out = torch.empty(3, dtype=torch.float32, device=dev)
    ws = torch.empty(_native.lib().sgr_mse_workspace_floats(Cc, H, W), dtype=torch.float32, device=dev)
    call("sgr_mse_forward", dev, Cc, H, W, a, b, _prep_mask(mask, H, W), out, ws)
    return out[1]


# ---- cross-entropy on the rendered semantic head (include/sgr_semantic_loss.h) ------------------------------------------
SEMANTIC_MODES = {"logits": 0, "probabilities": 1}                              # SGR_SEM_LOGITS, SGR_SEM_PROBABILITIES
_SEM_LABEL_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}            # SGR_SEM_LABEL_U8 / I32 / I64
_SEM_LABEL_CONVERTED = (torch.int16, torch.float32)                             # one .to(torch.int32)
SEM_MAX_CHANNELS = 32                                                           # SGR_SEM_MAX_CHANNELS


class SemanticTerms(NamedTuple):
    """0-dim views of ``values`` (4 floats on the device, include/sgr_semantic_loss.h's enum order): the mean
    cross-entropy over the valid pixels, their number, the number of labels >= S that are not ``ignore_index`` (a bad
    label map shows here, without a device assert), and the share of valid pixels whose arg-max channel is the label.
    ``pred`` is the uint8 [H, W] arg-max image with ``return_pred=True``, else None."""
    loss: torch.Tensor
    n_valid: torch.Tensor
    n_out_of_range: torch.Tensor
    accuracy: torch.Tensor
    values: torch.Tensor
    pred: Optional[torch.Tensor] = None


class _SemanticLoss(torch.autograd.Function):
    """The map kernel and one finishing workgroup forward, ONE kernel backward that writes dL/dsemantics -- the image the
    rasterizer's backward reads -- with zeros on the pixels that do not count."""

    @staticmethod
    def forward(ctx, semantic, labels, label_dtype, ignore_index, mode, return_pred):
        L = _native.lib()
        S, H, W = semantic.shape
        dev = semantic.device
        values = torch.empty(4, dtype=torch.float32, device=dev)
        pred = torch.empty(H, W, dtype=torch.uint8, device=dev) if return_pred else None
        ws = torch.empty(L.sgr_semantic_loss_workspace_floats(S, H, W), dtype=torch.float32, device=dev)
        call("sgr_semantic_loss_forward", dev, S, H, W, semantic, labels, label_dtype, ignore_index, mode, values, pred, ws)
        ctx.save_for_backward(semantic, labels, values)
        ctx.scalars = (label_dtype, ignore_index, mode)
        ctx.mark_non_differentiable(values)
        if pred is not None:
            ctx.mark_non_differentiable(pred)
        return values[0], values, pred

    @staticmethod
    def backward(ctx, upstream, _values, _pred):
        semantic, labels, values = ctx.saved_tensors
        S, H, W = semantic.shape
        up = upstream.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(semantic)
        call("sgr_semantic_loss_backward", semantic.device, S, H, W, semantic, labels, *ctx.scalars, values, up, grad)
        return grad, None, None, None, None, None


def semantic_loss(semantic: torch.Tensor, labels: torch.Tensor, *, mode: str = "logits", ignore_index: int = -1,
                  return_pred: bool = False):
    """Cross-entropy of the rendered semantic head against a label map, in one op -> ``(loss, terms)``.

    ``semantic`` is the rasterizer's fifth output, ``[S, H, W]`` float32 with ``S <= 32``; ``labels`` is ``[H, W]`` or
    ``[1, H, W]``, uint8 / int32 / int64 as they are, int16 / float32 (what the reference's ``get_semantic_label``
    returns) through one ``.to(torch.int32)``.  A pixel counts when its label is in ``[0, S)`` and is not
    ``ignore_index`` (labels < 0 are invalid, lib/utils/sem_utils.py:35).  ``mode='logits'`` is
    ``F.cross_entropy``; ``mode='probabilities'`` is street_gaussian_renderer.py:261-262 (normalise the alpha-weighted
    probabilities, log with eps 1e-8) followed by ``F.nll_loss``.  ``loss`` (0-dim) is differentiable with respect to
    ``semantic`` only; ``loss.backward()`` is one kernel.  ``terms`` (SemanticTerms) lives on the device: nothing here
    waits on the host."""
    if mode not in SEMANTIC_MODES:
        raise ValueError(f"mode must be one of {sorted(SEMANTIC_MODES)}, not {mode!r}")
    if semantic.dim() != 3:
        raise ValueError("semantic must have dimensions (S, H, W)")
    S, H, W = semantic.shape
    if not 1 <= S <= SEM_MAX_CHANNELS:
        raise ValueError(f"semantic has {S} channels: the rasterizer renders 1 to {SEM_MAX_CHANNELS}")
    if labels.dim() == 3 and labels.shape[0] == 1:
        labels = labels[0]
    if tuple(labels.shape) != (H, W):
        raise ValueError(f"labels must have dimensions ({H}, {W}) or (1, {H}, {W}), not {tuple(labels.shape)}")
    if labels.dtype not in _SEM_LABEL_DTYPES and labels.dtype not in _SEM_LABEL_CONVERTED:
        raise ValueError(f"labels of dtype {labels.dtype}: uint8, int16, int32, int64 or float32 are accepted")
    require_hip("semantic and labels must be HIP (cuda) tensors: there is no CPU path", semantic, labels)
    if labels.dtype in _SEM_LABEL_CONVERTED:
        labels = labels.to(torch.int32)
    loss, values, pred = _SemanticLoss.apply(semantic.to(torch.float32).contiguous(), labels.detach().contiguous(),
                                             _SEM_LABEL_DTYPES[labels.dtype], int(ignore_index), SEMANTIC_MODES[mode],
                                             bool(return_pred))
    return loss, SemanticTerms(*values.unbind(0), values, pred)
