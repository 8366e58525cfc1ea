"""CPU tests of the sky cube map's optimiser (include/sgr_sky_step.h, street_gaussians_amd.sky.SkyAdam): the lemma that
lets the step skip untouched elements, the host scalars, and the C ABI against its binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import torch_ref_optim as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
STEPS = (1, 2, 1000, 30000)
LRS = (0.01, 1.6e-4)
# +-0, denormals, ordinary values, the ends of the range
P_VALUES = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-38, 1e-3, 0.999, -5.0, 3.4e38, -3.4e38], dtype=f32)


def _bytes_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("step", STEPS)
def test_an_untouched_element_is_left_bitwise_unchanged(step, lr):
    """g = m = v = 0: m and v stay +0 and p keeps its bytes (its sign of zero and its denormals included), at every step
    count and learning rate -- so a step that skips such elements equals the dense one."""
    z = np.zeros_like(P_VALUES)
    assert (P_VALUES[2:6] != 0).all()  # the denormals are denormals, not flushed
    p, m, v = ro.adam_step(P_VALUES, z, z, z, lr, step)
    assert _bytes_equal(p, P_VALUES)
    assert _bytes_equal(m, z) and _bytes_equal(v, z)  # +0, not -0


def test_a_touched_element_keeps_moving_without_a_gradient():
    """Why activity is sticky: after one gradient, g = 0 still changes p in the next step, and in many after it (the
    move shrinks like 0.9^k from about lr; at p = 0.5, one ulp 3e-8, it stays visible for more than 50 steps)."""
    p, m, v = ro.adam_step(f32([0.5]), f32([0.25]), f32([0]), f32([0]), 0.01, 1)
    assert m[0] != 0 and v[0] != 0
    trace = [p[0]]
    for step in range(2, 402):
        p, m, v = ro.adam_step(p, f32([0]), m, v, 0.01, step)
        trace.append(p[0])
    assert trace[1] != trace[0]
    assert sum(a != b for a, b in zip(trace, trace[1:])) >= 50
    assert m[0] != 0 and v[0] != 0  # the moments are still there after 400 steps: the block stays active


@pytest.mark.parametrize("lr", LRS + (0.0,))
@pytest.mark.parametrize("step", STEPS)
def test_host_scalars_match_the_restatement(step, lr):
    from street_gaussians_amd.sky import adam_scalars
    ss, bc2s = adam_scalars(lr, step)
    want_ss, want_bc2s = ro.host_scalars(lr, step)
    assert _bytes_equal([ss], [want_ss]) and _bytes_equal([bc2s], [want_bc2s])
    assert f32(ss) == ss and f32(bc2s) == bc2s  # already float32 values: what the kernel receives


def test_skyadam_refuses_what_breaks_the_lemma():
    """eps = 0 (0 / 0 on an untouched element) is refused before any tensor is looked at more closely."""
    import torch
    from street_gaussians_amd._native import SgrError
    from street_gaussians_amd.sky import SkyAdam
    with pytest.raises(ValueError):
        SkyAdam(torch.zeros(6, 4, 3, 3), 0.01)  # not square
    with pytest.raises((SgrError, ValueError)):
        SkyAdam(torch.zeros(6, 4, 4, 3), 0.01)  # a CPU tensor: there is no CPU path


# ---- ABI --------------------------------------------------------------------------------------------------------------
PROTO = re.compile(r"^(int|size_t)\s*(sgr_\w+)\s*\(([^)]*)\)", re.M)
NAMES = ("sgr_sky_step_block_texels", "sgr_sky_step_workspace_bytes", "sgr_sky_backward_deferred", "sgr_sky_adam_step")
KINDS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}


@pytest.fixture(scope="module")
def lib():
    from street_gaussians_amd import _native, build
    build.build()
    return C.CDLL(_native.LIB_PATH)


def _header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgr_sky_step.h")).read(), flags=re.S)
    out = {}
    for ret, name, params in PROTO.findall(text):
        params = [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
        out[name] = (KINDS[ret], [C.c_void_p if "*" in p else KINDS[" ".join(p.split()[:-1])] for p in params])
    return out


def test_header_and_binding_agree(lib):
    from street_gaussians_amd import _native
    protos = _header_prototypes()
    assert set(protos) == set(NAMES)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert _native.SIGNATURES[name] == protos[name], name
    # the deferred backward takes sgr_sky_backward's arguments with dL_dcube replaced by (cube_work, active)
    bwd = list(_native.SIGNATURES["sgr_sky_backward"][1])
    assert _native.SIGNATURES["sgr_sky_backward_deferred"][1] == bwd[:12] + [C.c_void_p, C.c_void_p] + bwd[13:]


def test_block_size_and_workspace_bytes_on_the_host(lib):
    lib.sgr_sky_step_workspace_bytes.restype = C.c_size_t
    lib.sgr_sky_step_workspace_bytes.argtypes = [C.c_int] * 3
    lib.sgr_sky_workspace_bytes.restype = C.c_size_t
    lib.sgr_sky_workspace_bytes.argtypes = [C.c_int] * 5
    block = lib.sgr_sky_step_block_texels()
    assert block > 0 and block % 64 == 0
    for H, W, R in [(0, 16, 8), (16, 0, 8), (16, 16, 0), (-1, 16, 8), (16, 16, -3), (65536, 65536, 8)]:
        assert lib.sgr_sky_step_workspace_bytes(H, W, R) == 0, (H, W, R)
    small, large = lib.sgr_sky_step_workspace_bytes(12, 16, 8), lib.sgr_sky_step_workspace_bytes(1280, 1920, 1024)
    assert 0 < small < large
    # sorted keys and values (16 B), a record (8 B) and the upstream (12 B) per pixel, a start per cell
    assert large >= 36 * 1280 * 1920 + 4 * 6 * 1025 * 1025
    # the deferred backward's scratch leaves the texture stages' buffers out
    assert 0 < lib.sgr_sky_workspace_bytes(1280, 1920, 1024, 3, 2) < lib.sgr_sky_workspace_bytes(1280, 1920, 1024, 3, 1)
    assert lib.sgr_sky_workspace_bytes(1280, 1920, 1024, 3, 3) == 0
