"""Public Python API, signature-for-signature the reference's
``diff_gaussian_rasterization`` package
(/root/reference/submodules/diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py):
``GaussianRasterizationSettings`` (:167-179), ``GaussianRasterizer`` (:181-260) and the autograd
function ``_RasterizeGaussians`` (:46-165), running on the MI355X-native kernels.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


def cpu_deep_copy_tuple(input_tuple):
    copied_tensors = [item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple]
    return tuple(copied_tensors)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, semantics, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, stats=None):
    # (grad mode is read HERE: inside an autograd Function's forward it is always off)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, semantics, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, stats, torch.is_grad_enabled())


# extension (not in the reference): the number of tile instances R of this process' most recent forward -- the reference
# keeps it inside the autograd context only (__init__.py:93); bench.py and the densify-loop test report it
_LAST = {"num_rendered": 0}


def last_num_rendered() -> int:
    return int(_LAST["num_rendered"])


# callables invoked at the end of every rasterizer backward with that view's dL/dcolour, geometry buffer and camera
# centre; empty unless a multiview.FactoredGradReducer is alive (extension, not part of the reference API)
BACKWARD_OBSERVERS = []


# callables invoked BEFORE the native backward with the call's input tensors; each may return a dict with
#   "out": {gradient name: destination tensor}   (see _C.rasterize_gaussians_backward: e.g. views of an exchange bucket),
#   "masked_color_out": [P, 3] destination of the clamp-masked colour gradient, "skip_sh_grad": True
# (extension, not part of the reference API; empty unless a multiview reducer is alive).  Entries may be weakref.WeakMethod
# objects (the reducers register themselves that way): a reducer that is dropped without close() does not stay alive -- with
# its exchange buffers -- through this list; dead entries are pruned as they are met.
BACKWARD_SINKS = []


def _live_sinks():
    import weakref
    out = []
    for s in list(BACKWARD_SINKS):
        fn = s() if isinstance(s, weakref.WeakMethod) else s
        if fn is None:
            BACKWARD_SINKS.remove(s)
        else:
            out.append(fn)
    return out


def remove_sink(method) -> None:
    """Removes `method` (or the weak reference to it) from BACKWARD_SINKS."""
    import weakref
    for s in list(BACKWARD_SINKS):
        fn = s() if isinstance(s, weakref.WeakMethod) else s
        if fn is None or fn == method:
            BACKWARD_SINKS.remove(s)


_COLOR_EVENTS = {}


def _color_event(device):
    """One event per device, created (first record) here so that the native side only re-records it."""
    ev = _COLOR_EVENTS.get(device)
    if ev is None:
        ev = torch.cuda.Event()
        with torch.cuda.device(device):
            ev.record()
        _COLOR_EVENTS[device] = ev
    return ev


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, semantics, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, stats=None, grad_mode=True, frame=None):
        # argument order of the native entry point (reference __init__.py:62-83)
        args = (raster_settings.bg, means3D, colors_precomp, semantics, opacities, scales, rotations,
                raster_settings.scale_modifier, cov3Ds_precomp, raster_settings.viewmatrix, raster_settings.projmatrix,
                raster_settings.tanfovx, raster_settings.tanfovy, raster_settings.image_height,
                raster_settings.image_width, sh, raster_settings.sh_degree, raster_settings.campos,
                raster_settings.prefiltered, raster_settings.debug)
        # (extension) a backward will follow and the colour comes from SH: the forward also stores the colour Jacobian
        # for it (sgr_forward_extras.color_jacobian).  Inference renders do not ask
        want_jac = bool(grad_mode) and any(ctx.needs_input_grad) and isinstance(sh, torch.Tensor) and sh.numel() != 0
        if raster_settings.debug:
            cpu_args = cpu_deep_copy_tuple(args)  # copy them before they can be corrupted
            try:
                (num_rendered, color, depth, alpha, semantic, radii, geomBuffer, binningBuffer,
                 imgBuffer) = _C.rasterize_gaussians(*args, color_jacobian=want_jac)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise ex
        else:
            (num_rendered, color, depth, alpha, semantic, radii, geomBuffer, binningBuffer,
             imgBuffer) = _C.rasterize_gaussians(*args, color_jacobian=want_jac)

        _LAST["num_rendered"] = num_rendered
        ctx.raster_settings = raster_settings
        ctx.stats = stats  # extension: densification statistics updated by the backward (GaussianRasterizer.stats_sink)
        ctx.num_rendered = num_rendered
        # (extension) identity of the opacity input, which the reference does not save: a BACKWARD_SINKS provider matches its
        # parameters against the call's inputs by storage address
        ctx.opacities_key = (opacities.data_ptr(), tuple(opacities.shape)) if isinstance(opacities, torch.Tensor) else None
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                              binningBuffer, imgBuffer, alpha, semantics)
        if frame is not None:
            # (extension) the frame's finished buffers, handed to a second head over the same lists
            # (GaussianRasterizer.forward_with_object_alpha); nothing of this call changes
            frame.update(num_rendered=num_rendered, radii=radii, geomBuffer=geomBuffer, binningBuffer=binningBuffer,
                         imgBuffer=imgBuffer)
        ctx.mark_non_differentiable(radii)
        # autograd would otherwise hand the backward a zero-filled gradient for EVERY output it has none for, radii
        # included (a P-element fill kernel per step); the backward below fills in only the ones it reads
        ctx.set_materialize_grads(False)
        return color, radii, depth, alpha, semantic

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha, grad_semantic):
        num_rendered = ctx.num_rendered
        raster_settings = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer, imgBuffer,
         alpha, semantics) = ctx.saved_tensors
        if grad_color is None:
            grad_color = torch.zeros((3,) + alpha.shape[1:], dtype=alpha.dtype, device=alpha.device)
        if grad_depth is None:
            grad_depth = torch.zeros_like(alpha)
        if grad_alpha is None:
            grad_alpha = torch.zeros_like(alpha)
        if grad_semantic is None:
            ns = semantics.shape[1] if semantics is not None and semantics.dim() == 2 else 0
            grad_semantic = torch.zeros((ns,) + alpha.shape[1:], dtype=alpha.dtype, device=alpha.device)
        args = (raster_settings.bg, means3D, radii, colors_precomp, scales, rotations, raster_settings.scale_modifier,
                cov3Ds_precomp, raster_settings.viewmatrix, raster_settings.projmatrix, raster_settings.tanfovx,
                raster_settings.tanfovy, grad_color, grad_depth, grad_alpha, grad_semantic, sh,
                raster_settings.sh_degree, raster_settings.campos, geomBuffer, num_rendered, binningBuffer, imgBuffer,
                alpha, semantics, raster_settings.debug)
        stats = ctx.stats
        # view-sharded training: the observers want dL/dcolour as early as it exists -- an event recorded between the row
        # sum and the per-Gaussian stage (sgr_backward_extras.color_ready_event)
        color_event = None
        if BACKWARD_OBSERVERS and means3D.is_cuda:
            color_event = _color_event(means3D.device)
        kw = {}
        if cov3Ds_precomp is None or cov3Ds_precomp.numel() == 0:
            kw["skip_cov3d_grad"] = True  # scales / rotations are used: nobody receives dL/dcov3D
        if BACKWARD_SINKS and means3D.is_cuda:  # (weakly held reducers: see BACKWARD_SINKS)
            inputs = {"means3D": means3D, "scales": scales, "rotations": rotations, "sh": sh, "semantics": semantics,
                      "colors": colors_precomp, "cov3D": cov3Ds_precomp}
            for sink in _live_sinks():
                d = sink(inputs=inputs, opacities_key=ctx.opacities_key, num_points=means3D.shape[0])
                if d:
                    if d.get("out"):
                        kw.setdefault("out", {}).update(d["out"])
                    if d.get("masked_color_out") is not None:
                        kw["masked_color_out"] = d["masked_color_out"]
                    if d.get("skip_sh_grad"):
                        kw["skip_sh_grad"] = True
        if raster_settings.debug:
            cpu_args = cpu_deep_copy_tuple(args)
            try:
                (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
                 grad_scales, grad_rotations, grad_semantics) = _C.rasterize_gaussians_backward(*args, stats=stats,
                                                                                                 color_event=color_event, **kw)
            except Exception as ex:
                torch.save(cpu_args, "snapshot_bw.dump")
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                raise ex
        else:
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations, grad_semantics) = _C.rasterize_gaussians_backward(*args, stats=stats,
                                                                                             color_event=color_event, **kw)

        for observer in list(BACKWARD_OBSERVERS):  # view-sharded training (multiview.FactoredGradReducer)
            observer(grad_colors=grad_colors_precomp, geomBuffer=geomBuffer, campos=raster_settings.campos,
                     sh_degree=raster_settings.sh_degree, num_points=means3D.shape[0], means3D=means3D,
                     color_ready=color_event)

        # same order as the reference (__init__.py:152-163); gradients of inputs that do not take part in
        # autograd (None / empty placeholders) are dropped instead of returned and ignored
        need = ctx.needs_input_grad
        grads = (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_semantics, grad_opacities,
                 grad_scales, grad_rotations, grad_cov3Ds_precomp, None, None, None, None)
        grads = tuple(g if (g is not None and need[i]) else None for i, g in enumerate(grads[:len(need)]))
        return grads  # (one per argument apply() was given: stats, grad_mode and frame are optional)


class _ObjectAlpha(torch.autograd.Function):
    """The object-alpha head (include/sgr_object_alpha.h): the alpha image of Gaussians [split, P) blended alone, over the
    finished buffers of a _RasterizeGaussians forward of the same frame (``frame``).  A second autograd function on the same
    input tensors, so autograd adds its gradients to the composite's.  It has no gradient for means2D, colours, SH or
    semantics and never updates a statistics sink."""

    @staticmethod
    def forward(ctx, means3D, opacities, scales, rotations, cov3Ds_precomp, raster_settings, frame, split):
        P = means3D.shape[0]
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        acc, last = _C.layer_alpha_forward(P, frame["num_rendered"], H, W, split, frame["geomBuffer"],
                                           frame["binningBuffer"], frame["imgBuffer"])
        ctx.raster_settings = raster_settings
        ctx.num_rendered = frame["num_rendered"]
        ctx.split = split
        ctx.save_for_backward(means3D, scales, rotations, cov3Ds_precomp, frame["radii"], frame["geomBuffer"],
                              frame["binningBuffer"], frame["imgBuffer"], acc, last)
        ctx.set_materialize_grads(False)
        return acc

    @staticmethod
    def backward(ctx, grad_acc):
        need = ctx.needs_input_grad
        if grad_acc is None:
            return (None,) * 8
        means3D, scales, rotations, cov3Ds_precomp, radii, geomBuffer, binningBuffer, imgBuffer, acc, last = ctx.saved_tensors
        st = ctx.raster_settings
        g_means3D, g_opacity, g_scales, g_rotations, g_cov3D = _C.layer_alpha_backward(
            ctx.num_rendered, st.image_height, st.image_width, ctx.split, means3D, scales, rotations, st.scale_modifier,
            cov3Ds_precomp, radii, geomBuffer, binningBuffer, imgBuffer, acc, last, grad_acc, st.debug)
        grads = (g_means3D, g_opacity, g_scales, g_rotations, g_cov3D, None, None, None)
        return tuple(g if (g is not None and need[i]) else None for i, g in enumerate(grads))


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class LayerImages(NamedTuple):
    """The two layer images of GaussianRasterizer.forward_layers: Gaussians [0, split) (``first``) and [split, P)
    (``rest``), each blended alone over the layer background."""
    rgb_first: torch.Tensor  # [3, H, W]
    acc_first: torch.Tensor  # [1, H, W]
    rgb_rest: torch.Tensor
    acc_rest: torch.Tensor


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings
        # extension (not in the reference): (xyz_gradient_accum [P,2], denom [P,1], max_radii2D [P]) float32 tensors that
        # the backward of the next forward updates in place with the view's densification statistics
        # (street_gaussian_model.py:551-571) -- see street_gaussians_amd.scene.FlatStats
        self.stats_sink = None

    def markVisible(self, positions):
        # Mark visible points (based on frustum culling for camera) with a boolean
        with torch.no_grad():
            raster_settings = self.raster_settings
            visible = _C.mark_visible(positions, raster_settings.viewmatrix, raster_settings.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, semantics=None):
        raster_settings = self.raster_settings

        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')

        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        if shs is None:
            shs = torch.Tensor([])
        if colors_precomp is None:
            colors_precomp = torch.Tensor([])
        if scales is None:
            scales = torch.Tensor([])
        if rotations is None:
            rotations = torch.Tensor([])
        if cov3D_precomp is None:
            cov3D_precomp = torch.Tensor([])
        if semantics is None:
            # the reference hard-codes .cuda() (reference __init__.py:218-219); same device as the Gaussians here
            semantics = torch.zeros(means3D.shape[0], 0, dtype=torch.float32, device=means3D.device)

        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, semantics, opacities, scales, rotations,
                                   cov3D_precomp, raster_settings, self.stats_sink)

    def forward_layers(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                       cov3D_precomp=None, semantics=None, *, split, layer_background=None, clamp=True):
        """Extension (not in the reference): ``forward`` plus the images of two layers of the same frame -- Gaussians
        [0, split) and [split, P), each blended alone over ``layer_background`` (default: white) with its own transmittance
        -- from one front end and one binning (sgr_forward_layers, include/sgr_layers.h).  What the reference's
        StreetGaussianRenderer.render_all gets from three forwards (lib/models/street_gaussian_renderer.py:13-72).

        Returns ``(color, radii, depth, alpha, semantics, layers)``: the first five are ``forward``'s, bit for bit; ``layers``
        is a ``LayerImages`` whose entries equal ``forward`` over the subset alone with ``bg = layer_background``.  ``clamp``
        clamps the layer colours to [0, 1] (render_kernel outside training, :242-243); the composite is never clamped.

        Inference only: no output takes part in autograd.  Under enabled grad mode an input that requires grad raises
        ValueError -- call it under ``torch.no_grad()``."""
        raster_settings = self.raster_settings

        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')

        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        if torch.is_grad_enabled():
            named = (("means3D", means3D), ("means2D", means2D), ("opacities", opacities), ("shs", shs),
                     ("colors_precomp", colors_precomp), ("scales", scales), ("rotations", rotations),
                     ("cov3D_precomp", cov3D_precomp), ("semantics", semantics), ("layer_background", layer_background))
            tracked = [n for n, t in named if isinstance(t, torch.Tensor) and t.requires_grad]
            if tracked:
                raise ValueError("forward_layers is inference only and has no backward, but " + ", ".join(tracked) +
                                 " require grad: call it under torch.no_grad() (use forward() for training)")

        with torch.no_grad():
            e = torch.Tensor([])
            z = lambda t: e if t is None else t.detach()
            if semantics is None:
                semantics = torch.zeros(means3D.shape[0], 0, dtype=torch.float32, device=means3D.device)
            if layer_background is None:
                layer_background = torch.ones(3, dtype=torch.float32, device=means3D.device)
            out = _C.rasterize_gaussians_layers(
                raster_settings.bg, means3D.detach(), z(colors_precomp), semantics.detach(), opacities.detach(), z(scales),
                z(rotations), raster_settings.scale_modifier, z(cov3D_precomp), raster_settings.viewmatrix,
                raster_settings.projmatrix, raster_settings.tanfovx, raster_settings.tanfovy, raster_settings.image_height,
                raster_settings.image_width, z(shs), raster_settings.sh_degree, raster_settings.campos,
                raster_settings.prefiltered, raster_settings.debug, int(split), layer_background.detach(), bool(clamp))
        num_rendered, color, depth, alpha, semantic, radii = out[:6]
        _LAST["num_rendered"] = num_rendered
        return color, radii, depth, alpha, semantic, LayerImages(*out[9:13])

    def forward_with_object_alpha(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                                  rotations=None, cov3D_precomp=None, semantics=None, *, split):
        """Extension (not in the reference): ``forward`` plus ``acc_object`` [1, H, W], the accumulated alpha of Gaussians
        [split, P) blended alone -- what the reference's training loop gets from a second whole render, render_object
        (train.py:114-122, lib/models/street_gaussian_renderer.py:58-72) -- from the frame's finished tile lists
        (include/sgr_object_alpha.h).

        Returns ``(color, radii, depth, alpha, semantics, acc_object)``.  The first five are ``forward``'s, bit for bit and
        with its autograd behaviour (means2D.grad, ``stats_sink``, the backward sinks of multiview).  ``acc_object`` equals
        ``forward``'s alpha over the subset alone and is differentiable with respect to rows [split, P) of means3D, opacities
        and scales / rotations (or cov3D_precomp); autograd adds its gradients to the composite's.  It never touches
        means2D, the statistics sink, colours or SH.  ``split`` outside [0, P] raises ValueError."""
        raster_settings = self.raster_settings

        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')

        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        split = int(split)
        P = means3D.shape[0]
        if split < 0 or split > P:
            raise ValueError(f"split must lie in [0, {P}], got {split}")

        e = torch.Tensor([])
        z = lambda t: e if t is None else t
        shs, colors_precomp, scales, rotations, cov3D_precomp = z(shs), z(colors_precomp), z(scales), z(rotations), z(cov3D_precomp)
        if semantics is None:
            semantics = torch.zeros(P, 0, dtype=torch.float32, device=means3D.device)

        frame = {}
        color, radii, depth, alpha, semantic = _RasterizeGaussians.apply(
            means3D, means2D, shs, colors_precomp, semantics, opacities, scales, rotations, cov3D_precomp, raster_settings,
            self.stats_sink, torch.is_grad_enabled(), frame)
        if P == 0 or split == P:  # no objects: zeros, no launch, nothing to differentiate
            acc_object = torch.zeros_like(alpha)
        else:
            acc_object = _ObjectAlpha.apply(means3D, opacities, scales, rotations, cov3D_precomp, raster_settings, frame, split)
        return color, radii, depth, alpha, semantic, acc_object

    def visible_filter(self, means3D, scales=None, rotations=None, cov3D_precomp=None):
        raster_settings = self.raster_settings
        if scales is None:
            scales = torch.Tensor([])
        if rotations is None:
            rotations = torch.Tensor([])
        if cov3D_precomp is None:
            cov3D_precomp = torch.Tensor([])
        with torch.no_grad():
            radii, means2D = _C.rasterize_gaussians_filter(
                means3D, scales, rotations, raster_settings.scale_modifier, cov3D_precomp, raster_settings.viewmatrix,
                raster_settings.projmatrix, raster_settings.tanfovx, raster_settings.tanfovy,
                raster_settings.image_height, raster_settings.image_width, raster_settings.prefiltered,
                raster_settings.debug)
        return radii, means2D
