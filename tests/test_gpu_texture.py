"""The HIP cube-map lookup (nvdiffrast.torch.texture drop-in, include/sgr_texture.h) against the float64 restatement
(torch_ref_texture.py): forward values, the texture gradient, its sum invariant, write-once, bit-reproducibility, and
the reference's exact call shapes and keyword arguments (sky_cubemap.py:99-120, :178-191)."""
import ctypes as C
import math

import pytest
import torch

import torch_ref_texture as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _special_dirs():
    """Directions exactly on face edges, cube corners and axis ties, on texel boundaries, plus zero, NaN, huge, tiny."""
    d = []
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            d.append((sx, sy, 0.3)); d.append((sx, 0.3, sy)); d.append((0.3, sx, sy))  # |a| = |b| ties
            for sz in (-1.0, 1.0):
                d.append((sx, sy, sz))  # cube corners
                d.append((0.5 * sx, 0.5 * sy, 0.5 * sz))
            d.append((sx, sy, 0.0)); d.append((sx, 0.0, sy)); d.append((0.0, sx, sy))  # edge midpoints
    for a in (-1.0, 1.0):
        d.append((a, 0.0, 0.0)); d.append((0.0, a, 0.0)); d.append((0.0, 0.0, a))
        for t in (-0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1 - 2 ** -20, -1 + 2 ** -20):  # texel boundaries of R = 2, 4, 8
            d.append((a, t, 0.2)); d.append((t, a, -0.6)); d.append((0.4, t, a))
            d.append((a, t, 1.0)); d.append((t, 1.0, a))
    d += [(0.0, 0.0, 0.0), (float("nan"), 1.0, 0.0), (1.0, float("nan"), 0.5), (1e30, -3e29, 2e29), (-2e-30, 1e-30, 5e-31),
          (3e20, 3e20, 1e20)]
    return torch.tensor(d, dtype=torch.float32)


def _dirs(n, seed, near_edges=True):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    if near_edges:  # a third of them within a hair of a face edge
        k = n // 3
        sgn = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
        d[:k, 1] = sgn * d[:k, 0].abs() * (1 + 1e-4 * torch.randn(k, generator=g))
    return d


def _uv(B, shape, seed):
    """[B, H, W, 3] (or the masked [1, 1, N, 3] form when shape is an int) with the special directions mixed in."""
    sp = _special_dirs()
    out = []
    for b in range(B):
        n = shape if isinstance(shape, int) else shape[0] * shape[1]
        d = _dirs(n, seed + b)
        d[: min(n, sp.shape[0])] = sp[: min(n, sp.shape[0])]
        out.append(d[torch.randperm(n, generator=torch.Generator().manual_seed(seed + 7))])
    uv = torch.stack(out)
    uv = uv.reshape(B, 1, shape, 3) if isinstance(shape, int) else uv.reshape(B, shape[0], shape[1], 3)
    return uv.to(DEV)


def _check(tex, uv, dout):
    """HIP forward and texture gradient against the restatement, with the bounds of the contract."""
    import nvdiffrast.torch as dr
    R = tex.shape[2]
    t = tex.clone().requires_grad_(True)
    out = dr.texture(t, uv, filter_mode="linear", boundary_mode="cube")
    t64 = tex.double().requires_grad_(True)
    ref = tr.texture_ref(t64, uv)
    err = (out.double() - ref).abs().max().item() if out.numel() else 0.0
    tol = 2e-7 * R * tex.abs().max().item() + 1e-6
    assert torch.isfinite(out).all()
    assert err <= tol, f"forward |err| {err:.3e} > {tol:.3e}"
    out.backward(dout)
    ref.backward(dout.double())
    S = tr.grad_scale(uv, dout, tex.shape)
    gerr = (t.grad.double() - t64.grad).abs()
    bound = (5e-7 * R + 1e-6) * S
    bad = gerr > bound
    assert not bad.any(), f"gradient: {int(bad.sum())} elements over the bound, worst excess " \
                          f"{(gerr - bound).max().item():.3e}"
    # sum invariant: over valid samples the bilinear weights sum to 1
    _, _, valid = tr.tap_weights(uv, tex.shape[0], R)
    Cc = tex.shape[-1]
    want = dout.reshape(-1, Cc)[valid].double().sum(0)
    got = t.grad.double().reshape(-1, Cc).sum(0)
    scale = dout.reshape(-1, Cc)[valid].double().abs().sum(0) + 1e-12
    assert ((got - want).abs() <= 1e-5 * scale).all(), (got, want)
    return t.grad


CASES = [(R, Cc, 1, 1) for R in (1, 2, 5, 64, 1024) for Cc in (1, 3, 4, 7)] + \
        [(R, Cc, Bt, 2) for R in (1, 5, 64, 1024) for Cc in (3, 4) for Bt in (1, 2)]


@pytest.mark.parametrize("R,Cc,Bt,B", CASES)
def test_image_lookup_matches_the_restatement(R, Cc, Bt, B):
    g = torch.Generator().manual_seed(R * 100 + Cc * 10 + Bt)
    tex = torch.randn(Bt, 6, R, R, Cc, generator=g).to(DEV)
    uv = _uv(B, (24, 40), seed=R + Cc)
    dout = torch.randn(B, 24, 40, Cc, generator=g).to(DEV)
    _check(tex, uv, dout)


@pytest.mark.parametrize("R", [1, 2, 5, 64, 1024])
def test_masked_list_lookup_matches_the_restatement(R):
    """The masked form of sky_cubemap.py:117: the sky pixels as a [1, 1, N, 3] list."""
    g = torch.Generator().manual_seed(R)
    tex = torch.rand(1, 6, R, R, 3, generator=g).to(DEV)
    uv = _uv(1, 3001, seed=R)
    dout = torch.randn(1, 1, 3001, 3, generator=g).to(DEV)
    _check(tex, uv, dout)


def test_dense_samples_per_cell():
    """Many samples per texel cell (a full view at low R) and a full view at R = 64: long runs in the gather."""
    for R, H, W in ((2, 96, 128), (64, 192, 256)):
        g = torch.Generator().manual_seed(R)
        tex = torch.rand(1, 6, R, R, 3, generator=g).to(DEV)
        uv = _uv(1, (H, W), seed=3 * R)
        dout = torch.randn(1, H, W, 3, generator=g).to(DEV)
        _check(tex, uv, dout)


def _raw_backward(tex_shape, uv, dout, grad):
    from street_gaussians_amd import _native
    L = _native.lib()
    Bt, _, R, _, Cc = tex_shape
    B, H, W, _ = uv.shape
    work = torch.empty(L.sgr_texture_cube_workspace_bytes(Bt, B, R, Cc, H * W), dtype=torch.uint8, device=DEV)
    rc = L.sgr_texture_cube_backward(Bt, B, R, Cc, H * W, C.c_void_p(uv.data_ptr()), C.c_void_p(dout.data_ptr()),
                                     C.c_void_p(grad.data_ptr()), C.c_void_p(work.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc)


@pytest.mark.parametrize("R,Cc,Bt,B", [(1, 3, 1, 2), (5, 7, 2, 2), (64, 3, 1, 1), (1024, 1, 1, 1)])
def test_backward_writes_every_gradient_element(R, Cc, Bt, B):
    """Through the C ABI into a NaN-prefilled buffer: no NaN survives (untouched texels are written 0)."""
    uv = _uv(B, (16, 16), seed=R)
    dout = torch.randn(B, 16, 16, Cc, device=DEV)
    grad = torch.full((Bt, 6, R, R, Cc), float("nan"), device=DEV)
    _raw_backward(grad.shape, uv, dout, grad)
    torch.cuda.synchronize()
    assert not torch.isnan(grad).any()


def test_gradient_is_bit_reproducible():
    R, Cc = 64, 3
    uv = _uv(2, (96, 128), seed=11)
    dout = torch.randn(2, 96, 128, Cc, device=DEV)
    first = torch.empty(1, 6, R, R, Cc, device=DEV)
    _raw_backward(first.shape, uv, dout, first)
    for _ in range(10):
        again = torch.empty_like(first)
        _raw_backward(first.shape, uv, dout, again)
        assert torch.equal(again, first)


def test_no_host_synchronisation():
    import nvdiffrast.torch as dr
    tex = torch.rand(1, 6, 32, 32, 3, device=DEV, requires_grad=True)
    uv = _uv(1, (32, 48), seed=5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dr.texture(tex, uv, filter_mode="linear", boundary_mode="cube")
        out.permute(0, 3, 1, 2).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert tex.grad is not None


def test_reference_call_sites():
    """sky_cubemap.py's three calls with its exact keyword arguments and shapes; the upstream gradient arrives
    non-contiguous through `.permute(2, 0, 1).clamp(0, 1)`."""
    import nvdiffrast.torch as dr
    R, H, W = 16, 40, 56
    g = torch.Generator().manual_seed(1)
    base = (torch.rand(6, R, R, 3, generator=g) * 1.2 - 0.1).to(DEV)
    sky = torch.nn.Parameter(base.clone())
    rays_d = _uv(1, (H, W), seed=2)[0]
    gt = torch.rand(3, H, W, device=DEV)
    # unmasked (:99-101)
    color = dr.texture(sky[None, ...], rays_d[None, ...], filter_mode='linear', boundary_mode='cube')
    color = color[0].permute(2, 0, 1).clamp(0., 1.)
    ((color - gt) ** 2).sum().backward()
    t64 = base.double().requires_grad_(True)
    ref = tr.texture_ref(t64[None], rays_d[None])[0].permute(2, 0, 1).clamp(0., 1.)
    ((ref - gt.double()) ** 2).sum().backward()
    assert (color.double() - ref).abs().max().item() < 2e-7 * R * 1.1 + 1e-6
    assert (sky.grad.double() - t64.grad).abs().max().item() < 1e-5 * (1 + t64.grad.abs().max().item())
    # masked (:115-120)
    mask = torch.rand(H, W, generator=g).to(DEV) < 0.3
    sky.grad = None
    sel = rays_d[mask]
    sc = dr.texture(sky[None, ...], sel[None, None, ...], filter_mode='linear', boundary_mode='cube')
    sc = sc.squeeze(0).squeeze(0)
    out = torch.zeros(H, W, 3, device=DEV)
    out[mask] = sc
    out = out.permute(2, 0, 1).clamp(0., 1.)
    ((out - gt) ** 2).sum().backward()
    t64.grad = None
    r = tr.texture_ref(t64[None], sel[None, None])[0, 0]
    o64 = torch.zeros(H, W, 3, dtype=torch.float64, device=DEV)
    o64[mask] = r
    ((o64.permute(2, 0, 1).clamp(0., 1.) - gt.double()) ** 2).sum().backward()
    assert (sky.grad.double() - t64.grad).abs().max().item() < 1e-5 * (1 + t64.grad.abs().max().item())
    # cubemap_to_latlong (:178-191)
    res = [R, 2 * R]
    gy, gx = torch.meshgrid(torch.linspace(0.0 + 1.0 / res[0], 1.0 - 1.0 / res[0], res[0], device=DEV),
                            torch.linspace(-1.0 + 1.0 / res[1], 1.0 - 1.0 / res[1], res[1], device=DEV), indexing='ij')
    st, ct = torch.sin(gy * math.pi), torch.cos(gy * math.pi)
    sp, cp = torch.sin(gx * math.pi), torch.cos(gx * math.pi)
    reflvec = torch.stack((st * sp, ct, -st * cp), dim=-1)
    ll = dr.texture(sky[None, ...], reflvec[None, ...].contiguous(), filter_mode='linear', boundary_mode='cube')[0]
    ref = tr.texture_ref(base.double()[None], reflvec[None])[0]
    assert ll.shape == (R, 2 * R, 3)
    assert (ll.double() - ref).abs().max().item() < 2e-7 * R * 1.1 + 1e-6
