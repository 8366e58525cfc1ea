"""CPU tests for the colour-loss row: the torch restatement is pinned against the reference's own
l1_loss / ssim (extracted from its source, which cannot be imported whole) and the C ABI must be exported."""
import ctypes as C
import os
import re

import pytest
import torch

import torch_ref_loss as ref
from golden.refpin import Pin, reference_path

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LU = "lib/utils/loss_utils.py"  # under the reference checkout (golden/refpin.py)


def _reference_namespace():
    src = open(reference_path(LU)).read()
    ns = {"torch": torch, "F": torch.nn.functional, "exp": __import__("math").exp, "Variable": lambda t: t}
    for name in ("l1_loss", "gaussian", "create_window", "ssim", "_ssim"):  # the reference's own source, executed in place
        m = re.search(rf"^def {name}\(.*?(?=^def |\Z)", src, re.S | re.M)
        exec(m.group(0), ns)
    return ns


@pytest.mark.parametrize("masked", [False, True])
def test_restated_losses_match_the_reference(masked):
    pin = Pin(f"loss_cpu.losses.masked={masked}", LU)
    ns = _reference_namespace() if pin.live else None
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(3, 37, 53, generator=g), torch.rand(3, 37, 53, generator=g)
    mask = (torch.rand(1, 37, 53, generator=g) < 0.7) if masked else None
    pin.equal("l1_loss", ref.l1_loss(a, b, mask), lambda: ns["l1_loss"](a, b, mask))
    pin.equal("ssim", ref.ssim(a, b, mask=mask), lambda: ns["ssim"](a, b, mask=mask))
    pin.close()


def test_loss_abi_symbols_are_exported():
    from street_gaussians_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libsgr_hip.so not built")
    L = C.CDLL(_native.LIB_PATH)
    decl = open(os.path.join(ROOT, "include", "sgr_loss.h")).read()
    names = re.findall(r"^(?:int|size_t) (sgr_\w+)\(", decl, re.M)
    assert len(names) == 12
    for n in names:
        assert hasattr(L, n), n


TRAIN = "train.py"


def test_restated_sky_object_lidar_terms_match_train_py():
    """The sky / object-accumulation / LiDAR-depth terms are INLINE code of the reference's training loop (train.py, from
    `# sky loss` to `# color correction loss`), not functions: the block is cut out of the file by its comment markers and
    executed on stub objects; the restatements of tests/torch_ref_loss.py (the oracle of losses.sky_loss / obj_acc_loss /
    lidar_depth_loss) must give the same scalars bit for bit."""
    import textwrap
    import types
    pin = Pin("loss_cpu.train_py_terms", TRAIN)
    g = torch.Generator().manual_seed(9)
    H, W = 41, 57
    acc = torch.rand(1, H, W, generator=g)
    acc[0, :3] = 0.0  # clamp active at both ends
    acc[0, 3:5] = 1.0
    acc_obj = torch.rand(1, H, W, generator=g)
    depth = torch.rand(1, H, W, generator=g) * 30
    lidar = torch.rand(1, H, W, generator=g) * 30 * (torch.rand(1, H, W, generator=g) < 0.4)
    mask = torch.rand(1, H, W, generator=g) < 0.8
    sky_mask = torch.rand(1, H, W, generator=g) < 0.2
    obj_bound = torch.rand(1, H, W, generator=g) < 0.3
    ns = {"torch": torch, "acc": acc.clone(), "sky_mask": sky_mask, "obj_bound": obj_bound, "lidar_depth": lidar, "mask": mask,
          "depth": depth, "render_pkg": {"acc": acc.clone()}, "scalar_dict": {}, "loss": torch.zeros(()), "iteration": 10,
          "optim_args": types.SimpleNamespace(lambda_sky=0.05, lambda_sky_scale=[], lambda_reg=0.1, densify_until_iter=5,
                                              lambda_depth_lidar=0.1),
          "gaussians": types.SimpleNamespace(include_sky=True, include_obj=True),
          "viewpoint_cam": types.SimpleNamespace(meta={"cam": 0}),
          "gaussians_renderer": types.SimpleNamespace(render_object=lambda *a, **k: {"rgb": None, "acc": acc_obj.clone()})}
    if pin.live:
        src = open(reference_path(TRAIN)).read()
        a, b = src.index("        # sky loss"), src.index("        # color correction loss")
        exec(textwrap.dedent(src[a:b]), ns)
    sd = ns["scalar_dict"]
    assert pin.get("sky_loss", lambda: sd["sky_loss"]) == ref.sky_loss(acc, sky_mask).item()
    assert pin.get("obj_acc_loss", lambda: sd["obj_acc_loss"]) == ref.obj_acc_loss(acc_obj, obj_bound).item()
    pin.equal("lidar_depth_loss", ref.lidar_depth_loss(depth, acc, lidar, mask), lambda: sd["lidar_depth_loss"])
    want = 0.05 * ref.sky_loss(acc, sky_mask) + 0.1 * ref.obj_acc_loss(acc_obj, obj_bound) + 0.1 * ref.lidar_depth_loss(depth, acc, lidar, mask)
    assert torch.allclose(pin.get("loss", lambda: ns["loss"]), want, rtol=1e-6)
    pin.close()
