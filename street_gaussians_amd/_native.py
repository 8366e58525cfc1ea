"""ctypes loader of libsgr_hip.so (the C ABI declared in include/sgr.h).

The product path has NO fallback: if the library is missing, or a tensor is not on a HIP device,
this module raises -- it never routes to a CPU implementation (the oracle lives in oracle/ and is
test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _alloc

_HERE = os.path.dirname(os.path.abspath(__file__))
# SGR_LIB: another BUILD of the same library (tools/gpu_ab.sh variants built with other -D switches); never a fallback
LIB_PATH = os.environ.get("SGR_LIB") or os.path.join(_HERE, "libsgr_hip.so")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)

_lib = None


def _signatures():
    vp, f, d, i, u32, i64, sz = C.c_void_p, C.c_float, C.c_double, C.c_int, C.c_uint32, C.c_int64, C.c_size_t
    i64p = C.POINTER(C.c_int64)
    bwd = [i, i, i, i, i, vp, i, i, vp, vp, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, f, f, vp, vp, vp, vp, vp, vp, vp, vp,
           vp, vp, vp, vp, vp, vp, vp, vp, vp, ALLOC_FN, vp, i, vp]
    fwd = [ALLOC_FN, vp, ALLOC_FN, vp, ALLOC_FN, vp, i, i, i, i, vp, i, i, vp, vp, vp, vp, vp, vp, f, vp, vp, vp, vp, vp, f, f, i,
           vp, vp, vp, vp, vp, i, vp]
    return {
        "sgr_last_error": (C.c_char_p, []),
        "sgr_version": (i, []),
        "sgr_forward": (i, fwd),
        "sgr_forward_ex": (i, fwd + [vp]),
        "sgr_forward_layers": (i, fwd + [vp]),
        "sgr_layer_alpha_forward": (i, [i, i, i, i, i, vp, vp, vp, vp, vp, vp]),
        "sgr_layer_alpha_backward": (i, [i, i, i, i, i, vp, vp, f, vp, vp, vp] + [vp] * 11 + [ALLOC_FN, vp, i, vp]),
        "sgr_backward": (i, bwd),
        "sgr_backward_ex": (i, bwd + [vp]),
        "sgr_mark_visible": (i, [i, vp, vp, vp, vp, vp]),
        "sgr_visible_filter": (i, [i, i, i, vp, vp, f, vp, vp, vp, vp, f, f, i, vp, vp, i, vp]),
        "sgr_knn": (i, [i, vp, vp, ALLOC_FN, vp, vp]),
        "sgr_geometry_bytes": (sz, [i]),
        "sgr_binning_bytes": (sz, [i]),
        "sgr_image_bytes": (sz, [i, i]),
        "sgr_partial_row_floats": (i, [i]),
        "sgr_geometry_jac_offset": (sz, [i]),
        "sgr_export_internal": (i, [i, i, i, i, i, vp, vp, vp, vp, vp]),
        "sgr_export_cov3d": (i, [i, vp, f, vp, vp, vp]),
        "sgr_test_scan": (i, [vp, vp, sz, i, vp, vp]),
        "sgr_test_sort": (i, [vp, vp, vp, vp, u32, i, vp, vp, vp]),
        "sgr_test_sort32": (i, [vp, vp, vp, vp, u32, i, i, vp, vp, vp]),
        "sgr_test_sort_hist_words": (sz, [u32]),
        "sgr_test_scan_tmp_words": (sz, [sz]),
        "sgr_test_wave_sum": (i, [vp, vp, vp, i, vp]),
        "sgr_test_exact_math": (i, [i, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_test_lds_atomic_order": (i, [vp, vp, i, vp]),
        "sgr_test_switches": (i, [i]),
        "sgr_has_variants": (i, []),
        "sgr_set_lazy": (i, [i]),
        "sgr_lazy_status": (i, [vp, vp, vp]),
        "sgr_profile_host_wait_us": (i, [i]),
        "sgr_profile_enable": (i, [i]),
        "sgr_profile_select": (i, [i]),
        "sgr_profile_sample": (i, [i]),
        "sgr_profile_read": (i, [vp, vp]),
        "sgr_masked_color_grad": (i, [i, vp, vp, vp, vp]),
        "sgr_sh_grad_from_views": (i, [i, i, i, i, vp, vp, vp, vp, vp]),
        "sgr_sh_grad_from_views_ex": (i, [i, i, i, i, vp, sz, vp, sz, vp, sz, vp, vp]),
        "sgr_scene_compose_forward": (i, [i, vp, i, i, vp, vp, vp, vp, vp, vp, ALLOC_FN, vp, vp]),
        "sgr_scene_compose_backward": (i, [i, vp, vp, i, i, vp, vp, vp, vp, vp, vp, ALLOC_FN, vp, vp]),
        "sgr_scene_compose_forward_ex": (i, [i, vp, i, i, vp, vp, vp, vp, vp, vp, vp, ALLOC_FN, vp, vp]),
        "sgr_scene_compose_backward_ex": (i, [i, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, ALLOC_FN, vp, vp]),
        "sgr_scene_compose_backward_step": (i, [i, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, d, d, f, ALLOC_FN, vp, vp]),
        "sgr_scene_densification_stats": (i, [i, vp, vp, vp, ALLOC_FN, vp, vp]),
        "sgr_ssim_workspace_floats": (sz, [i, i, i]),
        "sgr_ssim_forward": (i, [i, i, i, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_ssim_backward": (i, [i, i, i, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_l1_workspace_floats": (sz, [i, i, i]),
        "sgr_l1_forward": (i, [i, i, i, vp, vp, vp, vp, vp, vp]),
        "sgr_l1_backward": (i, [i, i, i, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_color_loss_backward": (i, [i, i, i, vp, vp, vp, vp, vp, f, f, vp, vp, vp]),
        "sgr_bce_forward": (i, [i, i, vp, vp, vp, vp, vp]),
        "sgr_bce_backward": (i, [i, i, vp, vp, vp, vp, vp]),
        "sgr_lidar_work_bytes": (sz, [i]),
        "sgr_lidar_depth_forward": (i, [i, vp, vp, vp, vp, d, vp, vp, vp]),
        "sgr_lidar_depth_backward": (i, [i, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_frame_loss_saved_bytes": (sz, [i, i, i]),
        "sgr_frame_loss_workspace_floats": (sz, [i, i, i]),
        "sgr_frame_loss_finish_span": (i, []),
        "sgr_frame_loss_forward": (i, [i, i, i, vp, vp, vp, vp, vp]),
        "sgr_frame_loss_backward": (i, [i, i, i] + [vp] * 10),
        "sgr_semantic_loss_workspace_floats": (sz, [i, i, i]),
        "sgr_semantic_loss_block_pixels": (i, []),
        "sgr_semantic_loss_finish_span": (i, []),
        "sgr_semantic_loss_forward": (i, [i, i, i, vp, vp, i, i, i, vp, vp, vp, vp]),
        "sgr_semantic_loss_backward": (i, [i, i, i, vp, vp, i, i, i, vp, vp, vp, vp]),
        "sgr_mse_workspace_floats": (sz, [i, i, i]),
        "sgr_mse_forward": (i, [i, i, i, vp, vp, vp, vp, vp, vp]),
        "sgr_densify_work_bytes": (sz, [i]),
        "sgr_densify_plan": (i, [i, vp, vp, vp, vp, vp, vp, i64p, vp]),
        "sgr_densify_map": (i, [i, vp, vp, vp, vp, vp, vp]),
        "sgr_densify_gather": (i, [i, i, vp, vp, vp, i, vp, vp]),
        "sgr_densify_split_children": (i, [i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_densify_prune_mask": (i, [i, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, i64p, vp]),
        "sgr_densify_compact": (i, [i, vp, vp, vp, i64p, vp]),
        "sgr_reset_opacity": (i, [i, vp, vp, vp, vp]),
        "sgr_densify_scene_work_bytes": (sz, [i, i]),
        "sgr_densify_scene_plan": (i, [i, i] + [vp] * 7 + [i64p, vp]),
        "sgr_densify_scene_layout": (i, [i, vp, i64p, i64p]),
        "sgr_densify_scene_map": (i, [i, i] + [vp] * 7),
        "sgr_densify_scene_prune": (i, [i, i] + [vp] * 14 + [i64p, vp]),
        "sgr_densify_scene_gather_ragged": (i, [i, vp, vp, i64p, vp, i, vp, vp, vp, i, vp, vp]),
        "sgr_texture_cube_workspace_bytes": (sz, [i, i, i, i, i64]),
        "sgr_texture_cube_forward": (i, [i, i, i, i, i64, vp, vp, vp, vp]),
        "sgr_texture_cube_backward": (i, [i, i, i, i, i64, vp, vp, vp, vp, vp]),
        "sgr_adam_span_elems": (i, []),
        "sgr_adam_max_blocks": (i, []),
        "sgr_adam_max_records": (i, []),
        "sgr_adam_step": (i, [vp, i, vp, i, i64, d, d, vp]),
        "sgr_sky_workspace_bytes": (sz, [i, i, i, i, i]),
        "sgr_sky_forward": (i, [i, i, i, i] + [vp] * 9 + [i, vp, vp, vp]),
        "sgr_sky_backward": (i, [i, i, i, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_sky_step_block_texels": (i, []),
        "sgr_sky_step_workspace_bytes": (sz, [i, i, i]),
        "sgr_sky_backward_deferred": (i, [i, i, i, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sgr_sky_adam_step": (i, [i, vp, vp, vp, vp, vp, f, f, f, d, d, vp]),
        "sgr_sky_test_rays": (i, [i, i, vp, vp, vp, vp, i, vp, vp, vp]),
        "sgr_actor_pose_forward": (i, [i, vp, i] + [vp] * 7 + [vp]),
        "sgr_actor_pose_backward_max_blocks": (i, []),
        "sgr_actor_pose_backward": (i, [i, vp, i] + [vp] * 9 + [vp]),
        "sgr_test_sort32_count": (i, [vp, vp, vp, vp, u32, i, i, vp, vp, vp, vp]),
    }


# name -> (restype, argtypes) of every function include/*.h declares; the tests check each against its prototype and that
# the library exports all of them
SIGNATURES = _signatures()
SYMBOLS = list(SIGNATURES)


class SgrError(RuntimeError):
    pass


class SgrLazyError(SgrError):
    """-SGR_E_LAZY (lazy mode, sgr_set_lazy): the PREVIOUS lazy forward of this thread was invalid (list capacity overflow,
    prefilter violation, a depth beyond the narrow depth sort) -- ITS outputs and the gradients computed from them must be
    discarded (redo that step; do not apply its optimiser update).  The call that raised this rendered nothing; the thread's
    next forward is a blocking one that re-seeds the capacity.  Check ``_C.lazy_status()`` after a synchronisation and BEFORE
    applying gradients when a one-step-late report is not acceptable."""


SGR_E_LAZY = 5


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SgrError(f"{LIB_PATH} not found: build it with `python -m street_gaussians_amd.build` "
                           "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise (SgrLazyError if rc == -SGR_E_LAZY else SgrError)(lib().sgr_last_error().decode())
    return rc


def stream(device) -> C.c_void_p:
    """The current HIP stream of ``device``, as the C ABI takes it."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device address of tensor ``t`` as the C ABI takes it; None (NULL) for None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def launch(name: str, stream_, *args) -> int:
    """The stream-taking entry point ``name`` on ``stream_``: tensors go down as their device addresses (``ptr``; None stays
    NULL), every other argument as it is, the stream is appended as the last argument and the return code goes through
    ``check``.  Nothing is copied or converted: a tensor the kernel needs contiguous or float32 is made so by the caller.
    For a block of launches under one device guard and one stream lookup; a single launch is ``call``."""
    return check(getattr(lib(), name)(*[ptr(a) if isinstance(a, torch.Tensor) else a for a in args], stream_))


def call(name: str, device, *args) -> int:
    """One ``launch`` with ``device`` current, on its current stream."""
    with torch.cuda.device(device):
        return launch(name, stream(device), *args)


def require_hip(message: str, *tensors) -> None:
    """SgrError with the caller's ``message`` unless every tensor is a HIP (cuda) tensor: there is no CPU path."""
    if not all(t.is_cuda for t in tensors):
        raise SgrError(message)


class Grow:
    """Growable byte buffer handed to the C side (resizeFunctional, rasterize_points.cu:27-33).

    The callback closes over a one-element holder, NOT over this object: a bound method (`ALLOC_FN(self._alloc)`) made
    `Grow -> callback -> method -> Grow` a reference cycle, and the buffer -- hundreds of MB of backward scratch per
    call -- stayed allocated until Python's cyclic collector ran (round 5, tools/densify_gc_trace.py: +1.25 GB per
    iteration at 5 M Gaussians for ~10 iterations in a row; the densify loop's "device allocations in the region")."""

    def __init__(self, device):
        holder = [torch.empty(0, dtype=torch.uint8, device=device)]

        def alloc(nbytes, _user, holder=holder, device=device):
            # (a larger block than asked for is fine -- the native side carves what it needs -- and ladder sizes repeat
            # when the number of Gaussians drifts: _alloc.py)
            holder[0] = torch.empty(_alloc.ladder(int(nbytes)), dtype=torch.uint8, device=device)
            return holder[0].data_ptr()

        self._holder = holder
        self.cb = ALLOC_FN(alloc)

    @property
    def tensor(self):
        return self._holder[0]
