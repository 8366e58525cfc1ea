"""The forward blend step's weight from ONE select (street_gaussians_amd/csrc/sgr_math.h: sgr_blend_weight), on the host.

The parity-mode forward needs ae = "this lane blends ? alpha : 0" for its unfused depth and channel sums and
w = "blends ? alpha * T : 0" for the fused ones.  It selects ae and forms w = ae * T.  That has the bits of selecting the
product: on a blending lane it IS the product; on the others it is 0 * T = +0 for every T a transmittance can be (finite,
positive: T starts at 1, is multiplied by 1 - alpha >= 0.01 and never stored below 1e-4).  A NaN alpha (it passes the
kernels' !(alpha < thr) test) gives NaN in both forms -- compared as bytes, so the payload counts too.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_math", "blend_step_host.hip")
HDR = os.path.join(HERE, "..", "street_gaussians_amd", "csrc", "sgr_math.h")
LIB = os.path.join(HERE, "_build", "libsgr_blend_step_host.so")


@pytest.fixture(scope="module")
def bs():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-std=c++17",
                               SRC, "-o", LIB])
    return C.CDLL(LIB)


def _weights(bs, alpha, T, blends):
    alpha, T = np.ascontiguousarray(alpha, np.float32), np.ascontiguousarray(T, np.float32)
    blends = np.ascontiguousarray(blends, np.uint8)
    one, two = np.empty_like(alpha), np.empty_like(alpha)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bs.bs_weights(alpha.size, p(alpha), p(T), p(blends), p(one), p(two))
    return one.view(np.uint32), two.view(np.uint32)


def test_one_select_weight_has_the_bits_of_the_selected_product(bs):
    rng = np.random.default_rng(17)
    n = 1_000_000
    lo, hi = np.float32(1.0 / 255.0), np.float32(0.99)
    alpha = rng.uniform(lo, hi, n).astype(np.float32)
    # T in (1e-4, 1]: log-uniform (a pixel spends most of its list near either end), the ends themselves, and their neighbours
    T = np.exp(rng.uniform(np.log(1e-4), 0.0, n)).astype(np.float32)
    T = np.clip(T, np.nextafter(np.float32(1e-4), np.float32(1)), np.float32(1))
    edge_a = np.array([lo, np.nextafter(lo, hi), hi, np.nextafter(hi, lo), np.nan], np.float32)
    edge_T = np.array([1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1e-4), np.float32(1)), 0.5], np.float32)
    ea, eT = np.meshgrid(edge_a, edge_T, indexing="ij")
    alpha = np.concatenate([ea.reshape(-1), alpha])
    T = np.concatenate([eT.reshape(-1), T])
    assert np.isnan(alpha).sum() == edge_T.size and T.min() > 1e-4 and T.max() == 1.0
    for state in (0, 1):  # both lane states for every (alpha, T)
        one, two = _weights(bs, alpha, T, np.full(alpha.size, state, np.uint8))
        assert np.array_equal(one, two), int((one != two).sum())
        if state == 0:
            assert not one.any(), "a lane that does not blend has weight +0 (sign bit clear)"
        else:
            nan = np.isnan(alpha)
            assert np.array_equal(one[~nan], (alpha[~nan] * T[~nan]).view(np.uint32)) and np.isnan(one.view(np.float32)[nan]).all()
    # mixed states, as a wave has them
    blends = rng.integers(0, 2, alpha.size).astype(np.uint8)
    one, two = _weights(bs, alpha, T, blends)
    assert np.array_equal(one, two)
