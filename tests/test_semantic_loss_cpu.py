"""CPU tests of the semantic cross-entropy (losses.semantic_loss, include/sgr_semantic_loss.h): the per-pixel arithmetic the
gfx950 kernels run (street_gaussians_amd/csrc/sgr_semantic.h), compiled for the host, against the float64 restatement
tests/torch_ref_semantic_loss.py; the C ABI is declared, bound and exported; the Python argument checks need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torch_ref_semantic_loss as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_math", "semantic_host.hip")
HDR = os.path.join(ROOT, "street_gaussians_amd", "csrc", "sgr_semantic.h")
LIB = os.path.join(HERE, "_build", "libsgr_semantic_host.so")
FUNCTIONS = ("sgr_semantic_loss_workspace_floats", "sgr_semantic_loss_block_pixels", "sgr_semantic_loss_finish_span",
             "sgr_semantic_loss_forward", "sgr_semantic_loss_backward")
MODES = {"logits": 0, "probabilities": 1}
DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}


@pytest.fixture(scope="module")
def sh():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-std=c++17",
                               SRC, "-o", LIB])
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_op(sh, x, labels, mode, ignore_index, upstream=1.0):
    """The header's arithmetic over an image -> (loss, n_valid, n_out_of_range, accuracy, pred, gradient); the sums a
    kernel makes per block are made here in float64."""
    S, H, W = x.shape
    xs = np.ascontiguousarray(x.numpy(), dtype=np.float32)
    lab = np.ascontiguousarray(labels.numpy())
    loss_p, pred, cls = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    sh.sh_forward(S, H, W, _p(xs), _p(lab), DTYPES[labels.dtype], ignore_index, MODES[mode], _p(loss_p), _p(pred), _p(cls))
    valid = cls == 1
    n_valid = int(valid.sum())
    grad = np.full((S, H, W), np.nan, np.float32)
    sh.sh_backward(S, H, W, _p(xs), _p(lab), DTYPES[labels.dtype], ignore_index, MODES[mode],
                   C.c_float(np.float32(upstream) / np.float32(max(n_valid, 1))), _p(grad))
    loss = loss_p.astype(np.float64).sum() / n_valid if n_valid else float("nan")
    acc = ((pred == lab.astype(np.int64)) & valid).sum() / n_valid if n_valid else float("nan")
    return loss, n_valid, int((cls == 2).sum()), acc, pred, grad


CASES = [(mode, shape, dt, ign) for mode in MODES for shape in ref.SHAPES[1:]
         for dt, ign in ((torch.int64, -1), (torch.int32, -1), (torch.uint8, 255))]


@pytest.mark.parametrize("mode,shape,dtype,ignore_index", CASES,
                         ids=[f"{m}-{'x'.join(map(str, s))}-{str(d)[6:]}" for m, s, d, _ in CASES])
def test_header_arithmetic_matches_the_oracle(sh, mode, shape, dtype, ignore_index):
    x = ref.make_semantic(mode, *shape)
    labels = ref.make_labels(*shape, dtype=dtype, ignore_index=ignore_index)
    o64, g64, loss_bound, grad_bound, gscale = ref.bounds(x, labels, mode=mode, ignore_index=ignore_index, upstream=0.7)
    loss, n_valid, n_oor, acc, pred, grad = host_op(sh, x, labels, mode, ignore_index, upstream=0.7)
    assert n_valid == o64["n_valid"].item() and n_oor == o64["n_out_of_range"].item()
    assert 0 < n_valid < shape[1] * shape[2] and (n_oor > 0) == (shape[1] * shape[2] >= 40)
    loss_dev, grad_dev = abs(loss - o64["loss"].item()), np.abs(grad.astype(np.float64) - g64.numpy()).max()
    print(f"loss {loss_dev / loss_bound:.3f} of its bound {loss_bound:.3g}; gradient {grad_dev / grad_bound:.3f} of "
          f"its bound {grad_bound / gscale:.3g} of the largest element")
    assert loss_dev <= loss_bound
    assert grad_dev <= grad_bound
    assert (grad[:, ~o64["valid"].numpy()] == 0).all()
    free = ref.near_ties(x).numpy()
    assert free.mean() <= 0.001
    assert np.array_equal(pred[~free], o64["pred"].numpy().astype(np.uint8)[~free])
    assert abs(acc - o64["accuracy"].item()) <= 1e-12


def test_single_channel_and_no_valid_pixel(sh):
    x = ref.make_semantic("logits", 1, 1, 1)
    loss, n_valid, _, acc, pred, grad = host_op(sh, x, torch.zeros(1, 1, dtype=torch.int64), "logits", -1)
    assert loss == 0.0 and n_valid == 1 and acc == 1.0 and pred[0, 0] == 0 and grad[0, 0, 0] == 0.0
    x = ref.make_semantic("logits", 2, 5, 7)
    for labels in (torch.full((5, 7), -1), torch.full((5, 7), 2), torch.full((5, 7), 1)):
        ign = 1 if labels[0, 0] == 1 else -1
        loss, n_valid, n_oor, _, _, grad = host_op(sh, x, labels, "logits", ign)
        assert np.isnan(loss) and n_valid == 0 and n_oor == (35 if labels[0, 0] == 2 else 0) and (grad == 0).all()
        o, g = ref.loss_and_grad(x, labels, torch.float64, mode="logits", ignore_index=ign)
        assert torch.isnan(o["loss"]) and (g == 0).all()  # what the header promises is what torch gives


def test_first_maximum_wins_a_tie(sh):
    x = torch.zeros(5, 2, 3)
    x[3], x[1] = 2.0, 2.0
    x[4, 0, 0] = 2.0
    _, _, _, acc, pred, _ = host_op(sh, x, torch.ones(2, 3, dtype=torch.int64), "logits", -1)
    assert (pred == 1).all() and acc == 1.0 and (np.argmax(x.numpy(), axis=0) == pred).all()


def test_semantic_loss_abi_is_declared_bound_and_exported():
    from street_gaussians_amd import _native, build
    decl = open(os.path.join(ROOT, "include", "sgr_semantic_loss.h")).read()
    assert sorted(re.findall(r"^(?:int|size_t) (sgr_\w+)\(", decl, re.M)) == sorted(FUNCTIONS)
    for n in FUNCTIONS:
        assert n in _native.SIGNATURES, n
    for cite in ("street_gaussian_renderer.py:261-262", "gaussian_model.py:243-247", "sem_utils.py:35", "sem_utils.py:22"):
        assert cite in decl, cite
    assert re.findall(r"SGR_SEM_(LOSS|N_VALID|N_OUT_OF_RANGE|ACCURACY|TERMS) = (\d+)", decl) == \
        [("LOSS", "0"), ("N_VALID", "1"), ("N_OUT_OF_RANGE", "2"), ("ACCURACY", "3"), ("TERMS", "4")]
    assert "sgr_semantic_loss.hip" in build.SOURCES and "sgr_semantic.h" in build.HEADERS
    assert any(h.endswith("sgr_semantic_loss.h") for h in build.HEADERS)
    build.build()  # hipcc cross-compiles for gfx950; a no-op when the objects are up to date
    L = C.CDLL(_native.LIB_PATH)
    for n in FUNCTIONS:
        assert hasattr(L, n), n
    # the size queries are host code: four partials per block of the map kernel
    L.sgr_semantic_loss_workspace_floats.restype = C.c_size_t
    bp, span = L.sgr_semantic_loss_block_pixels(), L.sgr_semantic_loss_finish_span()
    assert bp > 0 and bp % 64 == 0 and span > 0
    assert L.sgr_semantic_loss_workspace_floats(19, 1280, 1920) == 4 * (-(-1280 * 1920 // bp))
    assert L.sgr_semantic_loss_workspace_floats(2, 1, 1) == 4
    # argument errors answer before any HIP call (SGR_E_INVALID = 1): S past the rasterizer's limit, unknown dtype and mode
    one = C.c_void_p(256)
    for S, dt, mode in ((33, 0, 0), (0, 0, 0), (3, 3, 0), (3, 0, 2)):
        assert L.sgr_semantic_loss_forward(S, 4, 4, one, one, dt, -1, mode, one, None, one, None) == -1
        assert L.sgr_semantic_loss_backward(S, 4, 4, one, one, dt, -1, mode, one, one, one, None) == -1


def test_python_argument_checks_need_no_device():
    from street_gaussians_amd import losses
    from street_gaussians_amd._native import SgrError
    x, lab = torch.rand(3, 8, 8), torch.zeros(8, 8, dtype=torch.int64)
    for args, kw in (((torch.rand(33, 8, 8), lab), {}), ((x, torch.zeros(8, 7, dtype=torch.int64)), {}),
                     ((x, torch.zeros(2, 8, 8, dtype=torch.int64)), {}), ((x[0], lab), {}), ((x, lab), dict(mode="softmax")),
                     ((x, lab.to(torch.float64)), {}), ((x, lab.to(torch.bool)), {}), ((x, lab.to(torch.int8)), {})):
        with pytest.raises(ValueError):
            losses.semantic_loss(*args, **kw)
    for labels in (lab, lab[None], lab.to(torch.uint8), lab.to(torch.int16), lab.to(torch.int32), lab.to(torch.float32)):
        with pytest.raises(SgrError, match="no CPU path"):
            losses.semantic_loss(x, labels)
    assert losses.SemanticTerms._fields == ref.NAMES + ("values", "pred")
    assert losses.SEM_MAX_CHANNELS == 32 and losses.SEMANTIC_MODES == MODES
