"""CPU pins of the sky composite's restatement (torch_ref_sky.py) to the reference's own code, cut out of its source and
executed (their recorded outputs, tests/golden/sky/pins.npz, where the reference checkout is absent): get_rays_torch
(lib/utils/graphics_utils.py:186-207), SkyCubeMap.forward (lib/models/sky_cubemap.py:77-123, with a stub cfg and self,
its device moves rewritten to the CPU and the restatement's lookup standing in for nvdiffrast) and ColorCorrection.forward
(lib/models/color_correction.py:129-132).  Also the refusals of street_gaussians_amd.sky.composite_sky, all decided
before any device is touched."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import torch_ref_sky as rs
import torch_ref_texture as tr
from golden.refpin import reference_path

GRAPHICS = "lib/utils/graphics_utils.py"
SKY = "lib/models/sky_cubemap.py"
CC = "lib/models/color_correction.py"
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sky", "pins.npz")


def _cut(path, pattern):
    src = open(reference_path(path)).read()
    m = re.search(pattern, src, re.S | re.M)
    assert m, f"{pattern} not found in {path}"
    return m.group(0)


def _dedent_method(text):
    lines = text.splitlines()
    ind = len(lines[0]) - len(lines[0].lstrip())
    return "\n".join(l[ind:] if l.strip() else "" for l in lines) + "\n"


def _camera(H, W, t_norm, seed):
    g = torch.Generator().manual_seed(seed)
    f = 0.9 * W
    K = torch.tensor([[f, 0.0, 0.5 * W + 1.25], [0.0, 1.01 * f, 0.5 * H - 0.75], [0.0, 0.0, 1.0]])
    a = math.radians(35.0 + seed)
    Rm = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    T = torch.randn(3, generator=g, dtype=torch.float64)
    T = (T / T.norm() * t_norm).float()
    return K, Rm, T


RAY_CASES = [(perturb, t) for perturb in (True, False) for t in (0.0, 1.0, 20.0, 200.0)]
SKY_CASES = [(train, has_mask, white, H) for train in (True, False) for has_mask in (True, False) for white in (True, False)
             for H in (24, 64)]


def _ray_inputs(perturb, t_norm):
    H, W = 13, 21
    K, Rm, T = _camera(H, W, t_norm, int(t_norm))
    return H, W, K, Rm, T


def _sky_inputs(train, has_mask, white, H):
    W, R = 16, 4
    g = torch.Generator().manual_seed(H + 2 * train + 4 * has_mask + 8 * white)
    acc = torch.rand(1, H, W, generator=g)
    acc[:, : H // 3] *= 1e-3
    sky_mask = (torch.rand(1, H, W, generator=g) < 0.3) if has_mask else None
    cube = torch.rand(6, R, R, 3, generator=g) * 1.4 - 0.2
    K, Rm, T = _camera(H, W, 3.0, H)
    w2c = torch.eye(4)
    w2c[:3, :3], w2c[:3, 3] = Rm, T
    return H, W, acc, sky_mask, cube, K, w2c


def _live_outputs():
    """What the reference's code returns on the cases above (None where the checkout is absent)."""
    if not os.path.exists(reference_path(GRAPHICS)):
        return None
    ns = {"torch": torch, "np": np}
    exec(_cut(GRAPHICS, r"^def get_rays_torch\(.*?(?=^\S|\Z)"), ns)
    get_rays_torch = ns["get_rays_torch"]
    out = {}
    for perturb, t in RAY_CASES:
        H, W, K, Rm, T = _ray_inputs(perturb, t)
        torch.manual_seed(5)
        o, d = get_rays_torch(H, W, K, Rm, T, perturb=perturb)
        out[f"rays/{perturb}/{t}/o"] = o[0, 0].numpy()  # the origin, broadcast over the image
        out[f"rays/{perturb}/{t}/d"] = d.numpy()

    src = _dedent_method(_cut(SKY, r"^    def forward\(self, camera: Camera, acc=None\):.*?(?=^    \S|^\S|\Z)"))
    src = src.replace(".to('cuda', non_blocking=True)", "").replace(".cuda()", "")
    for train, has_mask, white, H in SKY_CASES:
        Hh, W, acc, sky_mask, cube, K, w2c = _sky_inputs(train, has_mask, white, H)
        cam = types.SimpleNamespace(guidance={"sky_mask": sky_mask.clone()} if has_mask else {},
                                    world_view_transform=w2c.T.contiguous(), image_height=Hh, image_width=W, K=K)
        cfg = types.SimpleNamespace(mode="train" if train else "evaluate")
        dr = types.SimpleNamespace(texture=lambda tex, uv, filter_mode, boundary_mode: tr.texture_ref(tex, uv).float())
        stub = types.SimpleNamespace(cfg=types.SimpleNamespace(white_background=white), sky_cube_map=cube,
                                     sky_color=torch.zeros(1080, 1920, 3))
        ns = {"torch": torch, "cfg": cfg, "dr": dr, "get_rays_torch": get_rays_torch, "Camera": object}
        exec(src, ns)
        torch.manual_seed(9)
        sky = ns["forward"](stub, cam, acc)
        key = f"sky/{train}/{has_mask}/{white}/{H}"
        out[key] = sky.numpy()
        if has_mask:  # the reference writes the forced rows into the camera's mask in place (train only)
            out[key + "/mask_after"] = cam.guidance["sky_mask"].numpy()

    src = _dedent_method(_cut(CC, r"^    def forward\(self, camera: Camera, image: torch.Tensor, use_sky=False\):.*?(?=^    \S|^\S|\Z)"))
    ns = {"torch": torch, "Camera": object}
    exec(src, ns)
    g = torch.Generator().manual_seed(3)
    A = torch.cat([torch.eye(3) + 0.1 * torch.randn(3, 3, generator=g), 0.05 * torch.randn(3, 1, generator=g)], 1)
    img = torch.rand(3, 11, 17, generator=g)
    stub = types.SimpleNamespace(get_affine_trans=lambda camera, use_sky=False: A)
    out["cc/A"], out["cc/img"], out["cc/out"] = A.numpy(), img.numpy(), ns["forward"](stub, None, img).numpy()
    return out


@pytest.fixture(scope="module")
def ref_out():
    live = _live_outputs()
    if live is not None:
        if os.environ.get("SGR_RECORD_REFERENCE_OUTPUTS") == "1":
            os.makedirs(os.path.dirname(RECORD), exist_ok=True)
            np.savez_compressed(RECORD, **live)
        with np.load(RECORD) as rec:  # the record must still describe what the reference returns
            for k, v in live.items():
                assert np.array_equal(rec[k], v, equal_nan=True), k
        return {k: torch.from_numpy(v) for k, v in live.items()}
    with np.load(RECORD) as rec:
        return {k: torch.from_numpy(rec[k]) for k in rec.files}


@pytest.mark.parametrize("perturb,t_norm", RAY_CASES)
def test_rays_restatement_matches_get_rays_torch(ref_out, perturb, t_norm):
    H, W, K, Rm, T = _ray_inputs(perturb, t_norm)
    torch.manual_seed(5)
    p = torch.stack([torch.rand(H, W), torch.rand(H, W)]) if perturb else None
    d = rs.rays(H, W, K, Rm, T, p)
    want = ref_out[f"rays/{perturb}/{t_norm}/d"]
    bound = 8 * 2.0 ** -24 * (1 + t_norm)
    assert (d - want).abs().max().item() <= bound
    d64 = rs.rays(H, W, K.double(), Rm.double(), T.double(), p)
    assert (d64 - want.double()).abs().max().item() <= bound
    assert torch.allclose(ref_out[f"rays/{perturb}/{t_norm}/o"], -(Rm.T @ T), atol=1e-6 * (1 + t_norm))


@pytest.mark.parametrize("train,has_mask,white,H", SKY_CASES)
def test_sky_restatement_matches_sky_cubemap_forward(ref_out, train, has_mask, white, H):
    Hh, W, acc, sky_mask, cube, K, w2c = _sky_inputs(train, has_mask, white, H)
    keep = sky_mask.clone() if has_mask else None
    torch.manual_seed(9)
    p = torch.stack([torch.rand(Hh, W), torch.rand(Hh, W)]) if train else None
    mask = rs.sky_mask_of(acc, sky_mask, train)
    d = rs.rays(Hh, W, K, w2c[:3, :3], w2c[:3, 3], p)
    sky = rs.sky_color(cube, d, mask, white)
    want = ref_out[f"sky/{train}/{has_mask}/{white}/{H}"]
    assert sky.shape == want.shape
    assert torch.equal(sky, want)
    if has_mask:
        assert torch.equal(sky_mask, keep)  # the restatement leaves the caller's mask alone
        after = ref_out[f"sky/{train}/{has_mask}/{white}/{H}/mask_after"]
        if train:  # the reference's in-place write is what the restatement's mask is
            assert torch.equal(after[0], mask)


def test_color_correction_restatement_matches_the_reference(ref_out):
    out = rs.color_correct(ref_out["cc/A"], ref_out["cc/img"])
    assert torch.equal(out, ref_out["cc/out"])


def test_render_step2_restatement_eval_has_no_1080_row_limit():
    H, W = 1100, 8
    g = torch.Generator().manual_seed(0)
    out = rs.render_step2(torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g), torch.rand(6, 2, 2, 3, generator=g),
                          torch.tensor([[8.0, 0, 4], [0, 8.0, 550], [0, 0, 1]]), torch.eye(4), train=False, clamp_output=True)
    assert out.shape == (3, H, W) and out.min() >= 0 and out.max() <= 1


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _args(H=4, W=5, R=2, Cc=3):
    return [torch.rand(3, H, W), torch.rand(1, H, W), torch.rand(6, R, R, Cc), torch.eye(3), torch.eye(4)]


@pytest.mark.parametrize("case", ["rgb_shape", "acc_shape", "cube_shape", "cube_batch", "C4", "K_shape", "w2c_shape",
                                  "rgb_dtype", "cube_dtype", "affine_shape", "mask_dtype", "mask_shape", "perturb_shape",
                                  "empty"])
def test_refusals_before_any_device(case):
    from street_gaussians_amd.sky import composite_sky
    a = _args()
    kw = {}
    exc = ValueError
    if case == "rgb_shape":
        a[0] = torch.rand(4, 4, 5)
    elif case == "acc_shape":
        a[1] = torch.rand(4, 5)
    elif case == "cube_shape":
        a[2] = torch.rand(6, 2, 3, 3)
    elif case == "cube_batch":
        a[2] = torch.rand(2, 6, 2, 2, 3)
    elif case == "C4":
        a[2] = torch.rand(6, 2, 2, 4)
    elif case == "K_shape":
        a[3] = torch.eye(4)
    elif case == "w2c_shape":
        a[4] = torch.eye(3)
    elif case == "rgb_dtype":
        a[0], exc = a[0].double(), TypeError
    elif case == "cube_dtype":
        a[2], exc = a[2].half(), TypeError
    elif case == "affine_shape":
        kw["affine"] = torch.rand(3, 3)
    elif case == "mask_dtype":
        kw["sky_mask"], exc = torch.rand(1, 4, 5), TypeError
    elif case == "mask_shape":
        kw["sky_mask"] = torch.ones(2, 4, 5, dtype=torch.bool)
    elif case == "perturb_shape":
        kw["perturb"] = torch.rand(4, 5)
    elif case == "empty":
        a = _args(H=0)
    with pytest.raises(exc):
        composite_sky(*a, **kw)


def test_cpu_tensors_are_refused():
    from street_gaussians_amd._native import SgrError
    from street_gaussians_amd.sky import composite_sky
    with pytest.raises(SgrError, match="no CPU path"):
        composite_sky(*_args())
    with pytest.raises(SgrError, match="no CPU path"):
        composite_sky(*_args(), affine=torch.rand(3, 4), sky_mask=torch.ones(4, 5, dtype=torch.bool))
