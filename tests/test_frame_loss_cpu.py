"""CPU tests of the fused frame loss (losses.frame_loss, include/sgr_frame_loss.h): the fixture is what the reference's
own text returns, the restatement tests/torch_ref_frame_loss.py reproduces its float32 numbers bit for bit, the C ABI is
exported and bound, and the Python argument checks that need no device hold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torch_ref_frame_loss as ref
from golden import make_frame_loss_fixture as mk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FUNCTIONS = ("sgr_frame_loss_saved_bytes", "sgr_frame_loss_workspace_floats", "sgr_frame_loss_finish_span", "sgr_frame_loss_forward",
             "sgr_frame_loss_backward", "sgr_mse_workspace_floats", "sgr_mse_forward")


@pytest.fixture(scope="module")
def pins():
    return mk.load()


def restate(d, name, dt):
    """tests/torch_ref_frame_loss.py on one fixture case in dtype dt -> (dict of its eight scalars, the four leaves)."""
    c = mk.case(d, name)
    t = lambda k: torch.from_numpy(d[k])  # noqa: E731
    leaves = {k: t(k).to(dt).requires_grad_(True) for k in ("image", "acc", "depth", "acc_obj")}
    mask = t("mask") if c["masked"] else torch.ones_like(t("mask"))  # the all-True mask the reference's loop carries
    out = ref.frame_loss(leaves["image"], t("gt").to(dt), mask, lambda_dssim=float(d["lambda_dssim"]),
                         lambda_l1=float(d["lambda_l1"]), acc=leaves["acc"], sky_mask=t("sky_mask"),
                         lambda_sky=float(d["lambda_sky"]), sky_scale=None if np.isnan(c["sky_scale"]) else float(c["sky_scale"]),
                         acc_obj=leaves["acc_obj"], obj_bound=t("obj_bound"), lambda_reg=float(d["lambda_reg"]),
                         depth=leaves["depth"], lidar_depth=t("lidar").to(dt), lambda_depth_lidar=float(d["lambda_depth_lidar"]))
    return out, leaves


PIN_OF = {"l1": "l1_loss", "ssim": "ssim", "sky": "sky_loss", "obj": "obj_acc_loss", "lidar": "lidar_depth_loss", "mse": "mse",
          "psnr": "psnr", "loss": "loss"}


@pytest.mark.skipif(not os.path.exists(os.path.join(mk.REF, "train.py")), reason="needs the reference checkout")
def test_fixture_is_what_the_reference_text_returns(pins):
    fresh = mk.build()
    assert sorted(fresh) == sorted(pins)
    for k, v in fresh.items():
        assert v.dtype == pins[k].dtype and v.shape == pins[k].shape and np.array_equal(v, pins[k], equal_nan=v.dtype.kind == "f"), k


def test_fixture_covers_what_it_says(pins):
    assert list(pins["names"]) == ["masked", "scaled_nomask"]
    assert pins["image"].shape == (3, 41, 57) and (pins["acc"][0, :3] == 0).all() and (pins["acc"][0, 3:5] == 1).all()
    a, b = mk.case(pins, "masked"), mk.case(pins, "scaled_nomask")
    assert a["masked"] and np.isnan(a["sky_scale"]) and not b["masked"] and b["sky_scale"] == 1.3
    for c in (a, b):
        for k in mk.SCALARS + mk.GRADS:
            assert c[k + "32"].dtype == np.float32 and c[k + "64"].dtype == np.float64
        assert (c["d_acc64"][0, :3] == 0).all() and np.abs(c["d_acc64"][0, 3:5]).max() > 0  # sky clamp / LiDAR term alone
    assert (a["d_image64"][:, ~pins["mask"][0]] == 0).all()
    for k in mk.SCALARS + mk.GRADS:
        assert 0 < float(pins["e_ref_" + k]) < 1e-4, k
    assert os.path.getsize(mk.OUT) < 700 * 1024


@pytest.mark.parametrize("name", list(mk.CASES))
def test_restatement_matches_the_float32_pins(pins, name):
    """Bit for bit, scalars and gradients; `loss` within rtol 1e-6 (train.py accumulates it with +=, the restatement
    builds a new tensor per term: the pin of tests/test_loss_cpu.py uses the same bound)."""
    out, leaves = restate(pins, name, torch.float32)
    out["loss"].backward()
    c = mk.case(pins, name)
    for k, pk in PIN_OF.items():
        got, want = out[k].detach().numpy(), c[pk + "32"]
        if k == "loss":
            assert np.allclose(got, want, rtol=1e-6, atol=0), (k, got, want)
        else:
            assert got == want, (k, got, want)
    for k in ("image", "acc", "depth", "acc_obj"):
        got, want = leaves[k].grad.numpy(), c[f"d_{k}32"]
        assert np.array_equal(got, want), (k, np.abs(got - want).max())


@pytest.mark.parametrize("name", list(mk.CASES))
def test_restatement_in_float64_is_within_e_ref_of_the_float64_pins(pins, name):
    """The float64 restatement is the oracle of the GPU tests at other shapes: on the fixture it must sit on the float64
    pins far inside the reference's own float32 error."""
    out, leaves = restate(pins, name, torch.float64)
    out["loss"].backward()
    c = mk.case(pins, name)
    for k, pk in PIN_OF.items():
        want = c[pk + "64"]
        assert abs(out[k].item() - want) <= 0.01 * float(pins["e_ref_" + pk]) * abs(want), k
    for k in ("image", "acc", "depth", "acc_obj"):
        want = c[f"d_{k}64"]
        assert np.abs(leaves[k].grad.numpy() - want).max() <= 0.01 * float(pins["e_ref_d_" + k]) * np.abs(want).max(), k


def test_frame_loss_abi_is_declared_bound_and_exported():
    from street_gaussians_amd import _native, build
    decl = open(os.path.join(ROOT, "include", "sgr_frame_loss.h")).read()
    names = re.findall(r"^(?:int|size_t) (sgr_\w+)\(", decl, re.M)
    assert sorted(names) == sorted(FUNCTIONS)
    for n in FUNCTIONS:
        assert n in _native.SIGNATURES, n
    for cite in ("train.py:100-133", "loss_utils.py:21-37", "loss_utils.py", ":61-78", ":80-125"):
        assert cite in decl, cite
    enum = re.findall(r"SGR_FL_(\w+) = (\d+)", decl)
    assert enum == [("L1", "0"), ("SSIM", "1"), ("SKY", "2"), ("OBJ", "3"), ("LIDAR", "4"), ("MSE", "5"), ("PSNR", "6"),
                    ("LOSS", "7"), ("TERMS", "8")]
    assert "sgr_frame_loss.hip" in build.SOURCES and any(h.endswith("sgr_frame_loss.h") for h in build.HEADERS)
    assert "sgr_frame_loss.hip" not in build.PER_FILE_FLAGS
    build.build()  # hipcc cross-compiles for gfx950; a no-op when the objects are up to date
    L = C.CDLL(_native.LIB_PATH)
    for n in FUNCTIONS:
        assert hasattr(L, n), n
    # the size queries are host code: the workspace holds six sums per 16x16 tile, the saved block the three partial maps
    L.sgr_frame_loss_workspace_floats.restype = L.sgr_frame_loss_saved_bytes.restype = L.sgr_mse_workspace_floats.restype = C.c_size_t
    assert L.sgr_frame_loss_workspace_floats(3, 320, 480) == 6 * 20 * 30
    assert L.sgr_frame_loss_workspace_floats(3, 5, 7) == 6
    assert L.sgr_frame_loss_saved_bytes(3, 41, 57) >= 4 * (3 * 3 + 1) * 41 * 57
    assert L.sgr_mse_workspace_floats(3, 41, 57) == 2 * 10


def test_argument_struct_matches_the_header():
    """The ctypes mirror of sgr_frame_loss_args: same fields, same order, and the layout a C compiler gives it."""
    from street_gaussians_amd import losses
    decl = open(os.path.join(ROOT, "include", "sgr_frame_loss.h")).read()
    body = decl[decl.index("typedef struct sgr_frame_loss_args {"):decl.index("} sgr_frame_loss_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(const float\*|const uint8_t\*|float|double) (\w+);", body, re.M)
    kinds = {"const float*": C.c_void_p, "const uint8_t*": C.c_void_p, "float": C.c_float, "double": C.c_double}
    assert [(n, kinds[t]) for t, n in fields] == list(losses._FrameLossArgs._fields_)
    assert len(fields) == 16 and C.sizeof(losses._FrameLossArgs) == 9 * 8 + 6 * 4 + 8
    assert losses._FrameLossArgs.keep.offset == 96


def test_python_argument_checks_need_no_device():
    from street_gaussians_amd import losses
    from street_gaussians_amd._native import SgrError
    x, m = torch.rand(3, 8, 8), torch.rand(1, 8, 8)
    for kw in (dict(acc=m), dict(sky_mask=m > 0.5), dict(acc_obj=m), dict(obj_bound=m > 0.5), dict(depth=m, acc=m, sky_mask=m > 0.5),
               dict(lidar_depth=m), dict(depth=m, lidar_depth=m)):
        with pytest.raises(ValueError):
            losses.frame_loss(x, x, **kw)
    with pytest.raises(SgrError, match="no CPU path"):
        losses.frame_loss(x, x)
    with pytest.raises(SgrError, match="no CPU path"):
        losses.psnr(x, x)
    with pytest.raises(ValueError, match="not differentiable"):
        losses.psnr(x.clone().requires_grad_(True), x)
    assert losses.FrameTerms._fields == ref.NAMES + ("values",)
