"""The SSIM steps the gfx950 loss kernels run (street_gaussians_amd/csrc/sgr_ssim.h), compiled for the host and run lane by
lane over the 16x16 tiles by tests/host_math/host_math.hip (hm_ssim_tiles), against tests/torch_ref_loss.py::ssim in float64
with autograd for the gradient.  Shapes, inputs and bounds are those of tests/test_gpu_loss.py::_l1_and_ssim.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import torch_ref_loss as ref
from test_host_math import _p, hm  # noqa: F401  (hm: the module-scoped fixture that builds and loads the host library)


# (3, 5, 7): smaller than the halo, padding on all four sides; (1, 16, 16): exactly one tile; (3, 131, 77): several tiles,
# ragged both ways
@pytest.mark.parametrize("C_,H,W,masked", [(3, 5, 7, True), (1, 16, 16, False), (3, 131, 77, True)])
def test_ssim_tiles_match_reference(hm, C_, H, W, masked):
    g = torch.Generator().manual_seed(H * 1000 + W)
    a = torch.rand(C_, H, W, generator=g)
    b = (a + 0.2 * torch.randn(C_, H, W, generator=g)).clamp(0, 1)
    mask = (torch.rand(1, H, W, generator=g) < 0.8) if masked else None
    a64 = a.double().requires_grad_(True)
    ss_ref = ref.ssim(a64, b.double(), mask=mask)
    ss_ref.backward()
    an, bn = a.numpy(), b.numpy()
    mn = None if mask is None else np.ascontiguousarray(mask[0].numpy(), dtype=np.uint8)
    partials = np.zeros((3, C_, H, W), np.float32)
    grad = np.full((C_, H, W), np.nan, np.float32)
    ss = C.c_double(0.0)
    hm.hm_ssim_tiles(C_, H, W, _p(an), _p(bn), None if mn is None else _p(mn), _p(partials), C.byref(ss), _p(grad))
    gr, gg = a64.grad, torch.from_numpy(grad).double()
    scale = float(gr.abs().max())
    err_v, err_g = abs(ss.value - ss_ref.item()), float((gg - gr).abs().max())
    print(f"({C_}, {H}, {W}) masked={masked}: ssim {ss.value:.9g} ref {ss_ref.item():.9g} err {err_v:.3g} = "
          f"{err_v / 5e-6:.3f} of the bound; grad err {err_g:.3g} of max |ref| {scale:.3g} = {err_g / (2e-5 * scale):.3f} of the bound")
    assert err_v <= 5e-6
    assert err_g <= 2e-5 * scale
    if masked:
        assert float(gg[:, ~mask[0]].abs().max()) == 0.0


def _ssim_map_value(m1, m2, s11, s22, s12):
    """torch_ref_loss.ssim's map expression from the five windowed means."""
    c1, c2 = ref.K1 ** 2, ref.K2 ** 2
    m1m1, m2m2, m1m2 = m1.pow(2), m2.pow(2), m1 * m2
    return ((2 * m1m2 + c1) * (2 * (s12 - m1m2) + c2)) / ((m1m1 + m2m2 + c1) * ((s11 - m1m1) + (s22 - m2m2) + c2))


def test_ssim_point_on_flat_windows(hm):
    """ssim_point alone where its partials are largest: flat windows, s11 = m1^2, s22 = m2^2, s12 = m1 m2, so D = C2 = 9e-4
    and |dM/dsigma1^2| = val / C2 reaches 1111.  The function gets the float32 products; its own float32 products of the same
    factors cancel them exactly (the host build does not contract), so it sees D = C2 like the float64 reference, which is
    the map expression with autograd at the exactly flat window.  Bounds: the value within the project's 5e-6 (it is A / Cc,
    a few float32 roundings of a number <= 1); each partial within 2e-5 of the largest reference partial."""
    rng = np.random.default_rng(0)
    grid = np.linspace(0.0, 1.0, 33)
    pts = np.concatenate([np.stack(np.meshgrid(grid, grid), -1).reshape(-1, 2), rng.uniform(0, 1, (2000, 2))]).astype(np.float32)
    m1, m2 = pts[:, 0], pts[:, 1]
    m = np.ascontiguousarray(np.stack([m1, m2, m1 * m1, m2 * m2, m1 * m2], 1), dtype=np.float32)
    n = len(m)
    val, part = np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    hm.hm_ssim_point(n, _p(m), _p(val), _p(part))
    t1, t2 = torch.from_numpy(m1).double(), torch.from_numpy(m2).double()
    leaves = [t.clone().requires_grad_(True) for t in (t1, t2, t1 * t1, t2 * t2, t1 * t2)]
    want = _ssim_map_value(*leaves)
    want.sum().backward()
    want_part = torch.stack([leaves[0].grad, leaves[2].grad, leaves[4].grad], 1).numpy()
    scale = float(np.abs(want_part).max())
    assert scale > 1000.0  # the flat windows do reach the large partials
    err_v = float(np.abs(val - want.detach().numpy()).max())
    err_p = np.abs(part - want_part).max(axis=0)
    print(f"flat windows: value err {err_v:.3g} = {err_v / 5e-6:.3f} of the bound; partial errs {err_p} of max |ref| {scale:.6g} = "
          f"{err_p / (2e-5 * scale)} of the bound")
    assert err_v <= 5e-6
    assert (err_p <= 2e-5 * scale).all()
