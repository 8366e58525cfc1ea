"""Native entry points with the signatures of the reference's pybind module
``diff_gaussian_rasterization._C`` (/root/reference/submodules/diff-gaussian-rasterization/ext.cpp:15-20,
rasterize_points.h:18-88) and ``simple_knn._C`` (/root/reference/submodules/simple-knn/ext.cpp:15-17),
implemented over the C ABI of libsgr_hip.so.  PyTorch is used only for device memory and the stream.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native
from . import _alloc
from ._native import SgrError, SgrLazyError, call, check, ptr, require_hip
# _native.py's shared helpers under the names this module has exported all along: callers drive the ctypes path through
# _C._Grow and _C._stream (tests/test_gpu_tile_sort.py)
from ._native import Grow as _Grow, stream as _stream

NUM_CHANNELS = 3  # config.h:15

# Two bindings of the same C ABI: the pybind module built from csrc/ext.cpp with torch.utils.cpp_extension (what the
# reference ships, ext.cpp:15-20) and the ctypes one below (no compiler needed).  The pybind module is used for the
# five reference entry points when it has been built (street_gaussians_amd.build.build_pybind) unless
# SGR_BINDING=ctypes; everything beyond the reference's API (statistics sink, introspection, ...) is ctypes.
_ext = None
_ext_tried = False


def _pybind():
    global _ext, _ext_tried
    if not _ext_tried:
        _ext_tried = True
        import os
        if os.environ.get("SGR_BINDING", "") != "ctypes":
            _native.lib()  # libsgr_hip.so first: a missing library must raise its own, clear error
            try:
                from . import _C_pybind as m
                _ext = m
            except ImportError:
                if os.environ.get("SGR_BINDING", "") == "pybind":
                    raise
    return _ext


def binding() -> str:
    """'pybind' or 'ctypes': which binding serves the reference's entry points in this process."""
    return "pybind" if _pybind() is not None else "ctypes"


def set_binding(name: str) -> None:
    """Switch at run time (A/B of the host-side cost): 'pybind' or 'ctypes'."""
    global _ext, _ext_tried
    if name == "ctypes":
        _ext, _ext_tried = None, True
    elif name == "pybind":
        from . import _C_pybind as m
        _ext, _ext_tried = m, True
    else:
        raise ValueError(name)


def _call_ext(fn, *args):
    try:
        return fn(*args)
    except RuntimeError as ex:  # std::runtime_error of the C++ side -> the error type of the ctypes binding
        if isinstance(ex, SgrError):
            raise
        msg = str(ex).split("\n")[0]
        raise (SgrLazyError if "PREVIOUS lazy forward" in msg else SgrError)(msg) from None


class _StatSegment(C.Structure):  # sgr_stat_segment (include/sgr.h)
    _fields_ = [("src_start", C.c_int), ("count", C.c_int), ("dst_offset", C.c_int)]


class _BackwardExtras(C.Structure):  # sgr_backward_extras (include/sgr.h)
    _fields_ = [("xyz_gradient_accum", C.c_void_p), ("denom", C.c_void_p), ("max_radii2D", C.c_void_p),
                ("segments", C.POINTER(_StatSegment)), ("n_segments", C.c_int), ("color_ready_event", C.c_void_p),
                ("rows", C.c_int), ("masked_color_out", C.c_void_p), ("skip_sh_grad", C.c_int),
                ("skip_cov3d_grad", C.c_int)]


class _ForwardExtras(C.Structure):  # sgr_forward_extras (include/sgr.h)
    _fields_ = [("color_jacobian", C.c_int)]


MAX_STAT_SEGMENTS = 128  # SGR_MAX_STAT_SEGMENTS


def _dev_check(t: torch.Tensor, name: str):
    require_hip(f"{name} must be a HIP (cuda) tensor: street_gaussians_amd has no CPU path", t)
    if t.dtype != torch.float32 and t.dtype != torch.int32 and t.dtype != torch.uint8 and t.dtype != torch.bool:
        raise SgrError(f"{name} has unsupported dtype {t.dtype}")


def _means3D_check(means3D):
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _dev_check(means3D, "means3D")


def _addr(t):
    """device address of a buffer or an output as it is; None or an empty tensor -> NULL."""
    return ptr(t) if t is not None and t.numel() else None


class _Inputs:
    """The float tensors one native call reads: ``p(t, name)`` is the device address of ``t`` made contiguous -- None or an
    empty tensor -> NULL ("feature absent"), anything but float32 on the GPU an SgrError naming it -- and the
    object keeps what it made alive until the caller drops it, after the call."""

    def __init__(self):
        self.keep = []

    def __call__(self, t, name):
        if t is None or t.numel() == 0:
            return None
        _dev_check(t, name)
        if t.dtype != torch.float32:
            raise SgrError(f"{name} must be float32")
        t = t.contiguous()
        self.keep.append(t)
        return ptr(t)


def _forward(entry, alloc, tail, background, means3D, colors, semantics, opacity, scales, rotations, scale_modifier,
             cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
             prefiltered, debug):
    """The forward of sgr_forward_ex and sgr_forward_layers (``entry``): sizes, outputs, the three growable buffers and the
    one argument list.  ``alloc(shape, device)`` makes a float32 output image; ``tail(image, p)`` -- ``image(*shape)`` an
    output image, ``p`` the call's _Inputs -- returns the entry point's trailing structure (None -> NULL) and the outputs
    it holds, made once the common outputs exist.  Returns rasterize_gaussians' nine values followed by those outputs."""
    dev = means3D.device
    P, H, W = means3D.size(0), int(image_height), int(image_width)
    S = semantics.size(1) if semantics is not None and semantics.ndimension() == 2 else 0
    M = sh.size(1) if sh is not None and sh.numel() != 0 and sh.size(0) != 0 else 0
    with torch.cuda.device(dev):
        image = lambda *shape: alloc(shape, dev)
        out_color, out_depth, out_alpha = image(NUM_CHANNELS, H, W), image(1, H, W), image(1, H, W)
        out_semantic = image(S, H, W)
        p = _Inputs()
        extras, more = tail(image, p)
        # the preprocess kernel writes every element (0 for culled Gaussians): no zero fill (rasterize_points.cu:74)
        radii = (torch.empty if P else torch.zeros)((P,), dtype=torch.int32, device=dev)
        geom, binning, img = _Grow(dev), _Grow(dev), _Grow(dev)
        rendered = check(getattr(_native.lib(), entry)(
            geom.cb, None, binning.cb, None, img.cb, None, P, int(degree), M, S, p(background, "bg"), W, H,
            p(means3D, "means3D"), p(sh, "sh"), p(colors, "colors_precomp"), p(semantics, "semantics"),
            p(opacity, "opacities"), p(scales, "scales"), float(scale_modifier), p(rotations, "rotations"),
            p(cov3D_precomp, "cov3D_precomp"), p(viewmatrix, "viewmatrix"), p(projmatrix, "projmatrix"),
            p(campos, "campos"), float(tan_fovx), float(tan_fovy), int(bool(prefiltered)), ptr(out_color), ptr(out_depth),
            ptr(out_alpha), ptr(out_semantic) if S else None, ptr(radii) if P else None, int(bool(debug)), _stream(dev),
            C.byref(extras) if extras is not None else None))
    return (rendered, out_color, out_depth, out_alpha, out_semantic, radii, geom.tensor, binning.tensor, img.tensor) + more


def rasterize_gaussians(background, means3D, colors, semantics, opacity, scales, rotations, scale_modifier,
                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                        degree, campos, prefiltered, debug, color_jacobian=False):
    """RasterizeGaussiansCUDA (rasterize_points.cu:35-124).  color_jacobian (extension): a backward will follow -- the
    preprocess also stores the SH colour Jacobian for it (sgr_forward_extras.color_jacobian); same outputs."""
    _means3D_check(means3D)
    ext = _pybind()
    if ext is not None:
        e = torch.Tensor([])
        z = lambda t: e if t is None else t
        return _call_ext(ext.rasterize_gaussians, z(background), means3D, z(colors), z(semantics), z(opacity), z(scales),
                         z(rotations), float(scale_modifier), z(cov3D_precomp), z(viewmatrix), z(projmatrix),
                         float(tan_fovx), float(tan_fovy), int(image_height), int(image_width), z(sh), int(degree),
                         z(campos), bool(prefiltered), bool(debug), *((True,) if color_jacobian else ()))
    return _forward("sgr_forward_ex", lambda shape, dev: torch.empty(shape, dtype=torch.float32, device=dev),
                    lambda image, p: (_ForwardExtras(1) if color_jacobian else None, ()),
                    background, means3D, colors, semantics, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                    viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered,
                    debug)


class _LayerImages(C.Structure):  # sgr_layer_images (include/sgr_layers.h)
    _fields_ = [("split", C.c_int), ("background", C.c_void_p), ("clamp", C.c_int), ("color", C.c_void_p * 2),
                ("alpha", C.c_void_p * 2)]


def rasterize_gaussians_layers(background, means3D, colors, semantics, opacity, scales, rotations, scale_modifier,
                               cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                               degree, campos, prefiltered, debug, split, layer_background, clamp=True):
    """sgr_forward_layers (include/sgr_layers.h): rasterize_gaussians plus the colour and alpha images of Gaussians
    [0, split) and [split, P), each blended alone over ``layer_background`` -- one more launch on the same tile lists.
    Returns rasterize_gaussians' nine values followed by (color0 [3, H, W], alpha0 [1, H, W], color1, alpha1).
    Inference only; ctypes only (an entry point beyond the reference's API)."""
    _means3D_check(means3D)
    H, W = int(image_height), int(image_width)

    def tail(image, p):
        layer = (image(NUM_CHANNELS, H, W), image(1, H, W), image(NUM_CHANNELS, H, W), image(1, H, W))
        return _LayerImages(int(split), p(layer_background, "layer_background"), 1 if clamp else 0,
                            (C.c_void_p * 2)(layer[0].data_ptr(), layer[2].data_ptr()),
                            (C.c_void_p * 2)(layer[1].data_ptr(), layer[3].data_ptr())), layer
    return _forward("sgr_forward_layers", lambda shape, dev: _alloc.empty(shape, torch.float32, dev), tail,
                    background, means3D, colors, semantics, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                    viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered,
                    debug)


def layer_alpha_forward(P, R, image_height, image_width, split, geomBuffer, binningBuffer, imageBuffer):
    """sgr_layer_alpha_forward (include/sgr_object_alpha.h): the alpha image of Gaussians [split, P) blended alone, from the
    finished buffers of a rasterize_gaussians call of the same frame (R: its first return value).
    Returns (alpha [1, H, W] float32, last [H, W] int32 -- the layer's per-pixel last contributor, for the backward)."""
    require_hip("geomBuffer must be a HIP (cuda) tensor: street_gaussians_amd has no CPU path", geomBuffer)
    ext = _pybind()
    if ext is not None:
        return _call_ext(ext.layer_alpha_forward, int(P), int(R), int(image_height), int(image_width), int(split),
                         geomBuffer, binningBuffer, imageBuffer)
    dev = geomBuffer.device
    H, W = int(image_height), int(image_width)
    alpha = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    last = torch.empty((H, W), dtype=torch.int32, device=dev)
    call("sgr_layer_alpha_forward", dev, int(P), int(R), W, H, int(split), _addr(geomBuffer), _addr(binningBuffer),
         _addr(imageBuffer), alpha, last)
    return alpha, last


def layer_alpha_backward(R, image_height, image_width, split, means3D, scales, rotations, scale_modifier, cov3D_precomp,
                         radii, geomBuffer, binningBuffer, imageBuffer, layer_alpha, layer_last, dL_dlayer_alpha, debug):
    """sgr_layer_alpha_backward (include/sgr_object_alpha.h).  Returns (dL_dmeans3D [P, 3], dL_dopacity [P, 1],
    dL_dscales [P, 3], dL_drotations [P, 4], dL_dcov3D [P, 6] or None when cov3D_precomp is absent); rows [0, split) are
    zero."""
    _dev_check(means3D, "means3D")
    ext = _pybind()
    e = torch.Tensor([])
    z = lambda t: e if t is None else t
    if ext is not None:
        out = _call_ext(ext.layer_alpha_backward, int(R), int(image_height), int(image_width), int(split), means3D,
                        z(scales), z(rotations), float(scale_modifier), z(cov3D_precomp), radii, geomBuffer, binningBuffer,
                        imageBuffer, layer_alpha, layer_last, dL_dlayer_alpha, bool(debug))
        return out[:4] + (out[4] if out[4].numel() else None,)
    dev = means3D.device
    P = means3D.size(0)
    with_cov = cov3D_precomp is not None and cov3D_precomp.numel() != 0
    mk = (lambda *shape: _alloc.empty(shape, torch.float32, dev)) if P else (lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev))
    dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations = mk(P, 3), mk(P, 1), mk(P, 3), mk(P, 4)
    dL_dcov3D = mk(P, 6) if with_cov else None
    if P:
        scratch = _Grow(dev)
        p = _Inputs()
        if layer_last.dtype != torch.int32:
            raise SgrError("layer_last must be int32")
        call("sgr_layer_alpha_backward", dev, P, int(R), int(image_width), int(image_height), int(split),
             p(means3D, "means3D"), p(scales, "scales"), float(scale_modifier), p(rotations, "rotations"),
             p(cov3D_precomp, "cov3D_precomp"), _addr(radii.contiguous()), _addr(geomBuffer), _addr(binningBuffer),
             _addr(imageBuffer), p(layer_alpha, "layer_alpha"), _addr(layer_last.contiguous()),
             p(dL_dlayer_alpha, "dL_dlayer_alpha"), dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D,
             scratch.cb, None, int(bool(debug)))
    return dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                 viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_depth,
                                 dL_dout_alpha, dL_dout_semantic, sh, degree, campos, geomBuffer, R, binningBuffer,
                                 imageBuffer, alphas, semantics, debug, stats=None, color_event=None, out=None,
                                 masked_color_out=None, skip_sh_grad=False, skip_cov3d_grad=False):
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:126-220).  Returns
    (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dsemantic).
    stats (extension): (xyz_gradient_accum [P,2], denom [P,1], max_radii2D [P]) contiguous float32 tensors updated in
    place with this view's densification statistics (sgr_backward_ex); or a 4-tuple whose last element is a list of
    (src_start, count, dst_offset) segments mapping this call's Gaussians to rows of PERSISTENT statistics tensors of
    any length (a frame renders a subset of the sub-models, street_gaussian_model.py:230-250).
    color_event (extension): a torch.cuda.Event recorded on the current stream right after the row-sum stage, i.e. as
    soon as dL_dcolors is final and before the per-Gaussian stage runs (sgr_backward_extras.color_ready_event).
    out (extension): {"means3D" | "means2D" | "colors" | "opacity" | "cov3D" | "sh" | "scales" | "rotations" | "semantics":
    tensor} -- caller-supplied destinations for those gradients (contiguous float32 of the gradient's shape; e.g. views of
    a gradient-exchange bucket, street_gaussians_amd.multiview) instead of fresh allocations; they are what is returned.
    masked_color_out (extension): [P, 3] float32 destination of the clamp-masked colour gradient
    (sgr_backward_extras.masked_color_out).  skip_sh_grad (extension): dL_dsh is not computed, None is returned for it.
    skip_cov3d_grad (extension): likewise for dL_dcov3D (sgr_backward_extras.skip_cov3d_grad)."""
    _dev_check(means3D, "means3D")
    ext = _pybind()
    if ext is not None and stats is None and color_event is None and not out and masked_color_out is None and not skip_sh_grad:
        e = torch.Tensor([])
        z = lambda t: e if t is None else t
        return _call_ext(ext.rasterize_gaussians_backward, z(background), means3D, radii, z(colors), z(scales), z(rotations),
                         float(scale_modifier), z(cov3D_precomp), z(viewmatrix), z(projmatrix), float(tan_fovx),
                         float(tan_fovy), dL_dout_color, dL_dout_depth, dL_dout_alpha, z(dL_dout_semantic), z(sh),
                         int(degree), z(campos), geomBuffer, int(R), binningBuffer, imageBuffer, alphas, z(semantics),
                         bool(debug), *((True,) if skip_cov3d_grad else ()))
    dev = means3D.device
    P = means3D.size(0)
    H, W = dL_dout_color.size(1), dL_dout_color.size(2)
    S = dL_dout_semantic.size(0) if dL_dout_semantic is not None and dL_dout_semantic.numel() != 0 else 0
    M = sh.size(1) if sh is not None and sh.numel() != 0 and sh.size(0) != 0 else 0
    with torch.cuda.device(dev):
        fopt = dict(dtype=torch.float32, device=dev)
        # every element is written by the kernels (include/sgr.h), so no torch.zeros (rasterize_points.cu:166-176)
        mk0 = (lambda shape, **kw: _alloc.empty(shape, kw["dtype"], kw["device"])) if P else torch.zeros
        out = out or {}

        def mk(shape, name):
            t = out.get(name)
            if t is None:
                return mk0(shape, **fopt)
            if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
                raise SgrError(f"out[{name!r}] must be a contiguous float32 HIP tensor of shape {tuple(shape)}")
            return t
        dL_dmeans3D = mk((P, 3), "means3D")
        dL_dmeans2D = mk((P, 3), "means2D")
        dL_dcolors = mk((P, NUM_CHANNELS), "colors")
        dL_dopacity = mk((P, 1), "opacity")
        # (skipped: no allocation, NULL goes down -- unless the caller handed a destination, which is then left untouched)
        dL_dcov3D = None if (skip_cov3d_grad and P and out.get("cov3D") is None) else mk((P, 6), "cov3D")
        dL_dsh = None if (skip_sh_grad and P) else mk((P, M, 3), "sh")
        dL_dscales = mk((P, 3), "scales")
        dL_drotations = mk((P, 4), "rotations")
        dL_dsemantic = mk((P, S), "semantics")
        if P == 0:
            return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations,
                    dL_dsemantic)
        scratch = _Grow(dev)
        p = _Inputs()
        extras = None
        if stats is not None:
            acc, den, mr = stats[:3]
            segments = stats[3] if len(stats) > 3 else None
            rows = P if segments is None else den.numel()
            for t, n in ((acc, 2 * rows), (den, rows), (mr, rows)):
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
                    raise SgrError("densification statistics must be contiguous float32 HIP tensors " +
                                   ("covering all P Gaussians" if segments is None else "of one common length"))
            seg_arr, nseg = None, 0
            if segments is not None:
                nseg = len(segments)
                if nseg > MAX_STAT_SEGMENTS:
                    raise SgrError(f"at most {MAX_STAT_SEGMENTS} statistics segments per call")
                seg_arr = (_StatSegment * max(nseg, 1))()
                for k, (s0, cnt, d0) in enumerate(segments):
                    if d0 < 0 or cnt < 0 or d0 + cnt > rows:
                        raise SgrError("statistics segment outside the persistent tensors")
                    seg_arr[k] = _StatSegment(int(s0), int(cnt), int(d0))
            extras = _BackwardExtras(acc.data_ptr(), den.data_ptr(), mr.data_ptr(), seg_arr, nseg, None, int(rows), None, 0, 0)
        if color_event is not None or masked_color_out is not None or skip_sh_grad or skip_cov3d_grad:
            if extras is None:
                extras = _BackwardExtras(None, None, None, None, 0, None, 0, None, 0, 0)
            if color_event is not None:
                extras.color_ready_event = C.c_void_p(int(color_event.cuda_event))
            if masked_color_out is not None:
                m = masked_color_out
                if not (m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() and m.numel() == 3 * P):
                    raise SgrError("masked_color_out must be a contiguous float32 HIP tensor of 3 * P elements")
                extras.masked_color_out = ptr(m)
            extras.skip_sh_grad = 1 if skip_sh_grad else 0
            extras.skip_cov3d_grad = 1 if skip_cov3d_grad else 0
        check(_native.lib().sgr_backward_ex(
            P, int(degree), M, int(R), S, p(background, "bg"), W, H, p(means3D, "means3D"), p(sh, "sh"),
            p(colors, "colors_precomp"), p(semantics, "semantics"), p(alphas, "alpha"), p(scales, "scales"),
            float(scale_modifier), p(rotations, "rotations"), p(cov3D_precomp, "cov3D_precomp"),
            p(viewmatrix, "viewmatrix"), p(projmatrix, "projmatrix"), p(campos, "campos"), float(tan_fovx),
            float(tan_fovy), _addr(radii.contiguous()), _addr(geomBuffer), _addr(binningBuffer), _addr(imageBuffer),
            p(dL_dout_color, "dL_dout_color"), p(dL_dout_depth, "dL_dout_depth"), p(dL_dout_alpha, "dL_dout_alpha"),
            p(dL_dout_semantic, "dL_dout_semantic"), _addr(dL_dmeans2D), _addr(dL_dopacity), _addr(dL_dcolors), _addr(dL_dmeans3D),
            _addr(dL_dcov3D), _addr(dL_dsh), _addr(dL_dscales), _addr(dL_drotations), _addr(dL_dsemantic), scratch.cb, None,
            int(bool(debug)), _stream(dev), C.byref(extras) if extras is not None else None))
    return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations,
            dL_dsemantic)


def mark_visible(means3D, viewmatrix, projmatrix):
    """markVisible (rasterize_points.cu:222-241)."""
    _dev_check(means3D, "means3D")
    ext = _pybind()
    if ext is not None:
        return _call_ext(ext.mark_visible, means3D, viewmatrix, projmatrix)
    dev = means3D.device
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P:
        call("sgr_mark_visible", dev, P, means3D.contiguous(), viewmatrix.contiguous(), projmatrix.contiguous(), present)
    return present


def rasterize_gaussians_filter(means3D, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                               tan_fovx, tan_fovy, image_height, image_width, prefiltered, debug):
    """RasterizeGaussiansfilterCUDA (rasterize_points.cu:243-307)."""
    _means3D_check(means3D)
    ext = _pybind()
    if ext is not None:
        e = torch.Tensor([])
        z = lambda t: e if t is None else t
        return _call_ext(ext.rasterize_gaussians_filter, means3D, z(scales), z(rotations), float(scale_modifier),
                         z(cov3D_precomp), viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), int(image_height),
                         int(image_width), bool(prefiltered), bool(debug))
    dev = means3D.device
    P = means3D.size(0)
    radii = torch.zeros((P,), dtype=torch.int32, device=dev)
    means2D = torch.zeros((P, 2), dtype=torch.float32, device=dev)
    if P:
        p = _Inputs()
        call("sgr_visible_filter", dev, P, int(image_width), int(image_height), p(means3D, "means3D"), p(scales, "scales"),
             float(scale_modifier), p(rotations, "rotations"), p(cov3D_precomp, "cov3D_precomp"),
             p(viewmatrix, "viewmatrix"), p(projmatrix, "projmatrix"), float(tan_fovx), float(tan_fovy),
             int(bool(prefiltered)), radii, means2D, int(bool(debug)))
    return radii, means2D


def distCUDA2(points):
    """distCUDA2 (simple-knn/spatial.cu:16-26)."""
    _dev_check(points, "points")
    ext = _pybind()
    if ext is not None:
        return _call_ext(ext.distCUDA2, points)
    dev = points.device
    P = points.size(0)
    means = torch.zeros((P,), dtype=torch.float32, device=dev)
    if P:
        pts = points.contiguous()
        if pts.dtype != torch.float32:
            raise SgrError("points must be float32")
        scratch = _Grow(dev)
        call("sgr_knn", dev, P, pts, means, scratch.cb, None)
        torch.cuda.current_stream(dev).synchronize()  # scratch must outlive the kernels
    return means


_EXPORT = {"depths": (0, torch.float32, lambda P, R, N, T: (P,)), "clamped": (1, torch.uint8, lambda P, R, N, T: (P, 3)),
           "means2D": (2, torch.float32, lambda P, R, N, T: (P, 2)), "cov3D": (3, torch.float32, lambda P, R, N, T: (P, 6)),
           "conic_opacity": (4, torch.float32, lambda P, R, N, T: (P, 4)), "rgb": (5, torch.float32, lambda P, R, N, T: (P, 3)),
           "tiles_touched": (6, torch.int32, lambda P, R, N, T: (P,)), "point_offsets": (7, torch.int32, lambda P, R, N, T: (P,)),
           "point_list": (8, torch.int32, lambda P, R, N, T: (R,)), "keys": (9, torch.int64, lambda P, R, N, T: (R,)),
           "ranges": (12, torch.int32, lambda P, R, N, T: (T, 2)), "n_contrib": (13, torch.int32, lambda P, R, N, T: (N,)),
           "extents": (14, torch.float32, lambda P, R, N, T: (P, 2)), "hits": (15, torch.uint8, lambda P, R, N, T: (R,)),
           "tile_rect": (16, torch.int32, lambda P, R, N, T: (P, 4)),
           "num_rendered_reference": (17, torch.int32, lambda P, R, N, T: (1,)),
           "tile_mask": (18, torch.int64, lambda P, R, N, T: (P,)),
           "hit_list": (19, torch.int32, lambda P, R, N, T: (R,)), "n_contrib_k": (20, torch.int32, lambda P, R, N, T: (N,))}


def masked_color_grad(geomBuffer, grad_colors, P):
    """sgr_masked_color_grad: dL/dcolour with the channels the forward clamped set to zero -> [P, 3]."""
    _dev_check(grad_colors, "grad_colors")
    dev = grad_colors.device
    out = torch.empty((int(P), 3), dtype=torch.float32, device=dev)
    call("sgr_masked_color_grad", dev, int(P), geomBuffer, grad_colors.contiguous(), out)
    return out


def sh_grad_from_views(means3D, campos, drgb, degree, M):
    """sgr_sh_grad_from_views: sum_v Y(normalize(means3D - campos[v])) (x) drgb[v] -> dL/dSH [P, M, 3].
    campos [V, 3], drgb [V, P, 3]."""
    _dev_check(means3D, "means3D")
    dev = means3D.device
    P, V = means3D.size(0), campos.size(0)
    if drgb.shape != (V, P, 3):
        raise RuntimeError("drgb must have dimensions (num_views, num_points, 3)")
    out = torch.empty((P, int(M), 3), dtype=torch.float32, device=dev)
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    means3D, campos, drgb = f32(means3D), f32(campos), f32(drgb)
    call("sgr_sh_grad_from_views", dev, P, int(degree), int(M), V, means3D, campos, drgb, out)
    return out


def sh_grad_from_rows(P, degree, M, V, means_ptr, means_stride, campos_ptr, campos_stride, drgb_ptr, drgb_stride, device):
    """sgr_sh_grad_from_views_ex on raw device addresses + per-view strides (in floats): the rebuild of
    multiview.FactoredGradReducer reads its inputs straight out of the all-gathered payload rows.  -> [P, M, 3]."""
    out = torch.empty((int(P), int(M), 3), dtype=torch.float32, device=device)
    call("sgr_sh_grad_from_views_ex", device, int(P), int(degree), int(M), int(V), C.c_void_p(means_ptr),
         int(means_stride), C.c_void_p(campos_ptr), int(campos_stride), C.c_void_p(drgb_ptr), int(drgb_stride), out)
    return out


def has_variants() -> bool:
    """True when the loaded library also holds the rejected A/B designs (USE_V2, USE_ONESWEEP, USE_SW, USE_RS_WAVE): a
    tools/build_variant.py build with -DSGR_WITH_VARIANTS=1.  The shipped library ignores those switches."""
    return bool(_native.lib().sgr_has_variants())


def set_lazy(on: bool) -> bool:
    """sgr_set_lazy: the forward without a host wait (include/sgr.h).  Returns the previous setting."""
    return bool(_native.lib().sgr_set_lazy(1 if on else 0))


def lazy_status():
    """sgr_lazy_status of the calling thread -> (num_rendered, capacity, flags); synchronise the stream first."""
    r, c, f = C.c_int(0), C.c_int(0), C.c_int(0)
    check(_native.lib().sgr_lazy_status(C.byref(r), C.byref(c), C.byref(f)))
    return r.value, c.value, f.value


# sgr_test_switches bits, in bit order: the SGR_SW_* enum of include/sgr.h (same names without the prefix)
NO_CULL = 1 << 0  # blend kernels: no quadrant cull
NO_DPP = 1 << 1  # blend backward: no DPP wave reduction
NO_DET = 1 << 2  # blend backward: no deterministic LDS combine
NO_HITS = 1 << 3  # blend backward ignores the forward's hit record and redoes the cull
USE_V2 = 1 << 4  # S = 0 blend backward: transposed-accumulation kernel (variant build)
USE_ONESWEEP = 1 << 5  # radix sorts in their one-sweep form (variant build)
PRE_STAGE_SH = 1 << 6  # preprocess stages SH rows through LDS whatever P
EXACT = 1 << 7  # parity mode of the blend kernels and the per-Gaussian backward
USE_SW = 1 << 8  # S = 0 blend backward: scalar-walk kernel (variant build)
USE_RS_WAVE = 1 << 9  # per-Gaussian row sum: wave-cooperative form (variant build)
REF_RECT = 1 << 10  # emit every Gaussian for the reference's whole tile rect (default: cut down to where alpha >= 1/255 is possible)
NO_TILE_MASK = 1 << 11  # bounding-box rects without the per-tile mask (A/B)
TILE_SORT = 1 << 12  # binning chain A/B: index-order emission + per-tile LDS radix sort by depth (csrc/sgr_tile_sort.hip)
REF_RECT_PLAIN = 1 << 13  # with REF_RECT: the reference's rects WITHOUT the dead-instance marks (A/B)
LPT = 1 << 14  # blend launches ALWAYS walk the tiles longest list first (default: decided per frame, longest list > 2.5 x the mean)
NO_LPT = 1 << 15  # ... never: the XCD-aware supertile order without looking at the lists
NO_HLIST = 1 << 16  # the blend backward steps through list POSITIONS instead of the forward's compact list of hit instances (A/B)
HLIST_ALWAYS = 1 << 17  # the forward writes the compact list in every mode (default: with REF_RECT only)
KEY32 = 1 << 18  # 32-bit tile keys in the instance list (default: 16-bit whenever the frame has fewer than 65535 tiles; A/B)


def test_switches(mask: int = -1) -> int:
    """sgr_test_switches: A/B switches of the blend kernels (tests and tools only); returns the previous mask."""
    return int(_native.lib().sgr_test_switches(int(mask)))


def color_jacobian_view(geomBuffer, P):
    """The [P, 9] float32 colour Jacobian inside a forward's geometry buffer, as a VIEW (sgr_geometry_jac_offset): rows of
    Gaussians with radii > 0 are defined, and only when the forward ran with color_jacobian=True."""
    P = int(P)
    off = int(_native.lib().sgr_geometry_jac_offset(P))
    pad = (-geomBuffer.data_ptr()) % 256
    return geomBuffer[pad + off:pad + off + 36 * P].view(torch.float32).view(P, 9)


def geometry_header(geomBuffer):
    """The 64 header words of a forward's geometry buffer (int32 view): word 8 = the forward stored the colour Jacobian."""
    pad = (-geomBuffer.data_ptr()) % 256
    return geomBuffer[pad:pad + 256].view(torch.int32)


def export_internal(name, P, R, image_height, image_width, geomBuffer, binningBuffer, imageBuffer, scales=None,
                    rotations=None, scale_modifier=1.0):
    """Parity-test introspection (sgr_export_internal): dense copy of one internal array.  "cov3D" is the one array the
    buffers do not hold; it is recomputed from ``scales`` / ``rotations`` / ``scale_modifier`` (sgr_export_cov3d)."""
    which, dtype, shp = _EXPORT[name]
    H, W = int(image_height), int(image_width)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    dev = geomBuffer.device
    out = torch.zeros(shp(P, R, H * W, T), dtype=dtype, device=dev)
    if name == "cov3D":
        if scales is None or rotations is None:
            raise SgrError("cov3D is not kept in the buffers: pass the forward's scales and rotations")
        _dev_check(scales, "scales")
        _dev_check(rotations, "rotations")
        sc, rot = scales.detach().float().contiguous(), rotations.detach().float().contiguous()
        if sc.shape != (P, 3) or rot.shape != (P, 4):
            raise RuntimeError("scales must have dimensions (num_points, 3), rotations (num_points, 4)")
        call("sgr_export_cov3d", dev, int(P), _addr(sc), float(scale_modifier), _addr(rot), _addr(out))
    else:
        call("sgr_export_internal", dev, which, P, R, W, H, _addr(geomBuffer), _addr(binningBuffer), _addr(imageBuffer),
             _addr(out))
    torch.cuda.current_stream(dev).synchronize()
    return out
