"""The fused sky composite and colour correction (street_gaussians_amd.sky.composite_sky, include/sgr_sky.h) against
the reference's formulation: its rays, its forward bit for bit against texture() + torch ops on those rays, the cube-map
gradient bit for bit against texture()'s backward on the mask pixels, the other gradients against the float64
restatement (torch_ref_sky.py), the mask rules, the RNG stream, no host sync, reproducibility, the device-count sort,
and the reference's call site at full frame."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import torch_ref_sky as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TRAIN, WHITE, CLAMP = 1, 2, 4


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from street_gaussians_amd import _native
    return _native.lib(), _native.check


def _camera(H, W, yaw_deg=30.0, t_norm=5.0, seed=0):
    """K (pinhole, principal point off centre) and w2c (a yaw and a little pitch, translation of norm t_norm)."""
    g = torch.Generator().manual_seed(seed)
    f = 0.9 * W
    K = torch.tensor([[f, 0.0, 0.5 * W + 3.25], [0.0, 1.02 * f, 0.5 * H - 2.5], [0.0, 0.0, 1.0]])
    a, b = math.radians(yaw_deg), math.radians(7.0)
    Ry = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    T = torch.randn(3, generator=g, dtype=torch.float64)
    T = (T / T.norm() * t_norm).float()
    w2c = torch.eye(4)
    w2c[:3, :3] = (Rx @ Ry).float()
    w2c[:3, 3] = T
    return K.to(DEV), w2c.to(DEV)


def _inputs(H, W, R, seed, sky_frac=0.3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(3, H, W, generator=g) * 0.8
    acc = torch.rand(1, H, W, generator=g)
    acc[:, : int(sky_frac * H)] = torch.rand(1, int(sky_frac * H), W, generator=g) * 0.5 * 1e-3  # sky: 1 - acc > 1e-3
    cube = torch.rand(6, R, R, 3, generator=g) * 1.4 - 0.2  # some texels outside [0, 1]: the sky clamp matters
    affine = torch.cat([torch.eye(3) + 0.1 * torch.randn(3, 3, generator=g), 0.05 * torch.randn(3, 1, generator=g)], 1)
    perturb = torch.rand(2, H, W, generator=g)
    return [t.to(DEV) for t in (rgb, acc, cube, affine, perturb)]


def _op_rays(H, W, K, w2c, perturb=None):
    L, check = _lib()
    rays = torch.empty(H, W, 3, device=DEV)
    kinv = torch.empty(3, 3, device=DEV)
    px, py = (perturb[0].contiguous(), perturb[1].contiguous()) if perturb is not None else (None, None)
    check(L.sgr_sky_test_rays(H, W, _vp(K), _vp(w2c.contiguous()), _vp(px), _vp(py), TRAIN if perturb is not None else 0,
                              _vp(rays), _vp(kinv), _stream()))
    return rays, kinv


def _composed(rgb, acc, cube, rays, mask, white, affine=None, clamp_output=False):
    """The reference's Step 2 as torch ops on the op's rays, with our texture() for the lookup."""
    import nvdiffrast.torch as dr
    H, W = mask.shape
    sky = torch.full((H, W, 3), 1.0 if white else 0.0, device=DEV)
    if bool(mask.any()):
        sky[mask] = dr.texture(cube[None], rays[mask][None, None].contiguous(), filter_mode="linear",
                               boundary_mode="cube")[0, 0]
    sky = sky.permute(2, 0, 1).clamp(0.0, 1.0)
    out = rgb + sky * (1 - acc)
    if affine is not None:
        out = torch.einsum("ij,jhw->ihw", affine[:3, :3], out) + affine[:3, 3].unsqueeze(-1).unsqueeze(-1)
    if clamp_output:
        out = out.clamp(0.0, 1.0)
    return out


def _sky(*a, **k):
    from street_gaussians_amd.sky import composite_sky
    return composite_sky(*a, **k)


# ---- 1. rays --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_norm", [0.0, 3.0, 50.0, 200.0])
@pytest.mark.parametrize("train", [True, False])
def test_rays_match_the_restatement(t_norm, train):
    H, W = 61, 97
    K, w2c = _camera(H, W, yaw_deg=40.0, t_norm=t_norm, seed=int(t_norm))
    perturb = torch.rand(2, H, W, device=DEV) if train else None
    rays, kinv = _op_rays(H, W, K, w2c, perturb)
    ref = rs.rays(H, W, K.double(), w2c.double()[:3, :3], w2c.double()[:3, 3], perturb)
    bound = 8 * 2.0 ** -24 * (1 + t_norm)
    err = (rays.double() - ref).abs().max().item()
    assert err <= bound, f"ray |err| {err:.3e} > {bound:.3e}"
    kinv_t = torch.inverse(K)
    assert ((kinv - kinv_t).abs() <= 2 * 2.0 ** -24 * kinv_t.abs().max()).all(), (kinv, kinv_t)


# ---- 2. forward, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [True, False])
def test_forward_bitwise_against_texture_on_the_mask(white):
    H, W, R = 72, 120, 16
    rgb, acc, cube, affine, perturb = _inputs(H, W, R, seed=1)
    K, w2c = _camera(H, W, seed=1)
    rays, _ = _op_rays(H, W, K, w2c, perturb)
    mask = rs.sky_mask_of(acc, None, True)
    out = _sky(rgb, acc, cube, K, w2c, white_background=white, perturb=perturb)
    ref = _composed(rgb, acc, cube, rays, mask, white)
    assert torch.equal(out, ref)
    # with colour correction: bit for bit against the contract's order in numpy float32, within 2 ulp of einsum
    out_a = _sky(rgb, acc, cube, K, w2c, white_background=white, affine=affine, perturb=perturb)
    c = out.cpu().numpy()
    A = affine.cpu().numpy()
    want = np.stack([((A[i, 0] * c[0] + A[i, 1] * c[1]) + A[i, 2] * c[2]) + A[i, 3] for i in range(3)]).astype(np.float32)
    assert np.array_equal(out_a.cpu().numpy(), want)
    # einsum sums in its own order: 2 ulp of the size of its terms, sum_j |A_ij c_j| + |b_i| (a cancelling sum's result
    # can be far smaller than its terms)
    ein = _composed(rgb, acc, cube, rays, mask, white, affine=affine)
    terms = torch.einsum("ij,jhw->ihw", affine[:, :3].abs(), out.abs()) + affine[:, 3].abs()[:, None, None]
    assert ((out_a - ein).abs() <= 2 * torch.finfo(torch.float32).eps * terms).all()


# ---- 3. cube-map gradient, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 16, 64])
def test_cube_gradient_bitwise_against_texture_backward(R):
    import nvdiffrast.torch as dr
    H, W = 80, 112
    rgb, acc, cube, _, perturb = _inputs(H, W, R, seed=R)
    K, w2c = _camera(H, W, yaw_deg=45.0, seed=R)
    g = torch.randn(3, H, W, device=DEV)
    cube_p = cube.clone().requires_grad_(True)
    out = _sky(rgb, acc, cube_p, K, w2c, perturb=perturb)
    out.backward(g)
    rays, _ = _op_rays(H, W, K, w2c, perturb)
    mask = rs.sky_mask_of(acc, None, True)
    uv = rays[mask][None, None].contiguous()
    t = cube[None].clone().requires_grad_(True)
    raw = dr.texture(t, uv, filter_mode="linear", boundary_mode="cube")
    up = (g * (1 - acc)).permute(1, 2, 0)[mask]
    up = torch.where((raw[0, 0] >= 0) & (raw[0, 0] <= 1), up, torch.zeros_like(up))
    (want,) = torch.autograd.grad(raw, t, up[None, None])
    assert torch.equal(cube_p.grad, want[0])


# ---- 4. the other gradients -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_affine", [True, False])
def test_gradients_against_the_float64_restatement(with_affine):
    H, W, R = 64, 96, 8
    rgb, acc, cube, affine, perturb = _inputs(H, W, R, seed=7)
    K, w2c = _camera(H, W, seed=7)
    g = torch.randn(3, H, W, device=DEV)
    ins = [rgb.clone(), acc.clone(), affine.clone()]
    for t in ins:
        t.requires_grad_(True)
    out = _sky(ins[0], ins[1], cube, K, w2c, affine=ins[2] if with_affine else None, perturb=perturb)
    out.backward(g)
    rays, _ = _op_rays(H, W, K, w2c, perturb)
    ref_ins = [t.double().requires_grad_(True) for t in (rgb, acc, affine)]
    ref = rs.render_step2(ref_ins[0], ref_ins[1], cube.double(), K, w2c, affine=ref_ins[2] if with_affine else None,
                          perturb=perturb, d=rays.double())
    assert (out.double() - ref).abs().max().item() <= 1e-5
    ref.backward(g.double())
    A = affine.double() if with_affine else torch.cat([torch.eye(3, device=DEV), torch.zeros(3, 1, device=DEV)], 1).double()
    gs = (A[:, :3].abs().T @ g.double().abs().reshape(3, -1)).reshape(3, H, W)  # |A|^T |g|
    assert ((ins[0].grad.double() - ref_ins[0].grad).abs() <= 1e-6 * gs + 1e-30).all()
    assert ((ins[1].grad.double() - ref_ins[1].grad).abs() <= 1e-5 * gs.sum(0, keepdim=True) + 1e-30).all()
    if with_affine:
        c = (rgb.double() + 1.5).abs()  # |c| <= |rgb| + |sky| <= |rgb| + 1
        S = torch.einsum("ihw,jhw->ij", g.double().abs(), torch.cat([c, torch.ones(1, H, W, device=DEV)], 0).double())
        assert ((ins[2].grad.double() - ref_ins[2].grad).abs() <= 1e-6 * S).all()


# ---- 5. masks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [37, 90])
def test_sky_mask_rule_and_the_callers_mask_is_untouched(H):
    W, R = 64, 8
    rgb, acc, cube, affine, perturb = _inputs(H, W, R, seed=H)
    K, w2c = _camera(H, W, seed=H)
    sm = torch.rand(1, H, W, device=DEV) < 0.3
    keep = sm.clone()
    rays, _ = _op_rays(H, W, K, w2c, perturb)
    for m in (sm, sm[0]):
        out = _sky(rgb, acc, cube, K, w2c, sky_mask=m, perturb=perturb)
        assert torch.equal(out, _composed(rgb, acc, cube, rays, rs.sky_mask_of(acc, m, True), True))
        assert torch.equal(sm, keep)
    if H < 50:  # every row is forced on
        assert rs.sky_mask_of(acc, sm, True).all()
    # eval: the sky mask is not used, the acc rule is
    out = _sky(rgb, acc, cube, K, w2c, sky_mask=sm, train=False)
    rays_c, _ = _op_rays(H, W, K, w2c, None)
    assert torch.equal(out, _composed(rgb, acc, cube, rays_c, rs.sky_mask_of(acc, None, False), True))


def test_acc_mask_at_the_threshold():
    H, W, R = 16, 64, 4
    rgb, acc, cube, _, perturb = _inputs(H, W, R, seed=3)
    # no float32 acc makes 1 - acc exactly 1e-3f (1 - acc is a multiple of 2^-24 there): the floats of acc next to the
    # threshold on both sides, one ulp apart
    base = np.float32(1) - np.float32(1e-3)
    vals = base + np.arange(-40, 41, dtype=np.float32) * np.float32(2.0 ** -24)
    d = np.float32(1) - vals
    assert (d > np.float32(1e-3)).any() and (d < np.float32(1e-3)).any()
    acc = acc.clone()
    acc.view(-1)[: vals.size] = torch.from_numpy(vals).to(DEV)
    K, w2c = _camera(H, W, seed=3)
    rays, _ = _op_rays(H, W, K, w2c, perturb)
    for white in (True, False):
        out = _sky(rgb, acc, cube, K, w2c, white_background=white, perturb=perturb)
        assert torch.equal(out, _composed(rgb, acc, cube, rays, (1 - acc[0]) > 1e-3, white))


def _raw_call(rgb, acc, cube, K, w2c, flags, perturb, g):
    """Forward and backward through the C ABI, the cube gradient into a NaN-prefilled buffer."""
    L, check = _lib()
    _, H, W = rgb.shape
    R = cube.shape[1]
    saved = torch.empty(L.sgr_sky_workspace_bytes(H, W, R, 3, 0), dtype=torch.uint8, device=DEV)
    scratch = torch.empty(L.sgr_sky_workspace_bytes(H, W, R, 3, 1), dtype=torch.uint8, device=DEV)
    out = torch.full((3, H, W), float("nan"), device=DEV)
    px, py = perturb[0].contiguous(), perturb[1].contiguous()
    check(L.sgr_sky_forward(H, W, R, 3, _vp(rgb), _vp(acc), _vp(cube), _vp(K), _vp(w2c), None, _vp(px), _vp(py), None,
                            flags, _vp(out), _vp(saved), _stream()))
    drgb, dacc = torch.full_like(rgb, float("nan")), torch.full_like(acc, float("nan"))
    dcube = torch.full_like(cube, float("nan"))
    check(L.sgr_sky_backward(H, W, R, 3, _vp(g), _vp(rgb), _vp(acc), None, flags, _vp(saved), _vp(drgb), _vp(dacc),
                             _vp(dcube), None, _vp(scratch), _stream()))
    return out, drgb, dacc, dcube


@pytest.mark.parametrize("white", [True, False])
def test_empty_mask_and_all_sky(white):
    H, W, R = 40, 56, 8
    rgb, _, cube, _, perturb = _inputs(H, W, R, seed=11)
    K, w2c = _camera(H, W, seed=11)
    g = torch.randn(3, H, W, device=DEV)
    flags = TRAIN | (WHITE if white else 0)
    fill = 1.0 if white else 0.0
    acc = torch.ones(1, H, W, device=DEV)  # every pixel solid: no sky pixel
    out, drgb, dacc, dcube = _raw_call(rgb, acc, cube, K, w2c, flags, perturb, g)
    assert torch.equal(out, rgb + fill * (1 - acc))
    assert torch.equal(dcube, torch.zeros_like(cube))  # written, over the NaN prefill
    assert torch.equal(drgb, g)
    assert torch.equal(dacc[0], -((g[0] * fill + g[1] * fill) + g[2] * fill))
    # all sky
    acc0 = torch.zeros(1, H, W, device=DEV)
    out, drgb, dacc, dcube = _raw_call(rgb, acc0, cube, K, w2c, flags, perturb, g)
    rays, _ = _op_rays(H, W, K, w2c, perturb)
    assert torch.equal(out, _composed(rgb, acc0, cube, rays, torch.ones(H, W, dtype=torch.bool, device=DEV), white))
    assert not torch.isnan(dcube).any() and not torch.isnan(drgb).any() and not torch.isnan(dacc).any()


@pytest.mark.parametrize("with_affine", [True, False])
def test_clamp_output_and_its_gradient(with_affine):
    import nvdiffrast.torch as dr  # noqa: F401
    H, W, R = 48, 64, 8
    rgb, acc, cube, affine, perturb = _inputs(H, W, R, seed=5)
    rgb = rgb * 1.6 - 0.3  # outputs on both sides of [0, 1]
    K, w2c = _camera(H, W, seed=5)
    g = torch.randn(3, H, W, device=DEV)
    aff = affine if with_affine else None
    x = rgb.clone().requires_grad_(True)
    out = _sky(x, acc, cube, K, w2c, affine=aff, clamp_output=True, perturb=perturb)
    assert out.min() >= 0 and out.max() <= 1
    out.backward(g)
    unclamped = _sky(rgb, acc, cube, K, w2c, affine=aff, perturb=perturb)
    assert torch.equal(out, unclamped.clamp(0, 1))
    gp = torch.where((unclamped >= 0) & (unclamped <= 1), g, torch.zeros_like(g))
    want = torch.einsum("ij,ihw->jhw", aff[:, :3], gp) if with_affine else gp
    assert ((x.grad - want).abs() <= 1e-6 * (want.abs() + g.abs().sum(0))).all()


# ---- 6. RNG -----------------------------------------------------------------------------------------------------------
def test_rng_stream_matches_get_rays_torch():
    H, W, R = 33, 47, 8
    rgb, acc, cube, affine, _ = _inputs(H, W, R, seed=2)
    K, w2c = _camera(H, W, seed=2)
    torch.manual_seed(1234)
    out = _sky(rgb, acc, cube, K, w2c, affine=affine)
    after_op = torch.cuda.get_rng_state()
    torch.manual_seed(1234)
    px = torch.rand(H, W, device=DEV)
    py = torch.rand(H, W, device=DEV)
    after_two = torch.cuda.get_rng_state()
    assert torch.equal(after_op, after_two)
    assert torch.equal(out, _sky(rgb, acc, cube, K, w2c, affine=affine, perturb=torch.stack([px, py])))
    before = torch.cuda.get_rng_state()
    _sky(rgb, acc, cube, K, w2c, affine=affine, train=False)
    assert torch.equal(before, torch.cuda.get_rng_state())


# ---- 7. no host sync, 8. reproducibility ------------------------------------------------------------------------------
def test_no_host_sync_and_bitwise_reproducible():
    H, W, R = 96, 128, 32
    rgb, acc, cube, affine, _ = _inputs(H, W, R, seed=9)
    K, w2c = _camera(H, W, yaw_deg=45.0, seed=9)
    g = torch.randn(3, H, W, device=DEV)
    res = []
    for rep in range(2):
        ins = [t.clone().requires_grad_(True) for t in (rgb, acc, cube, affine)]
        torch.manual_seed(77)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = _sky(ins[0], ins[1], ins[2], K, w2c, affine=ins[3])
            out.backward(g)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        res.append([out.detach()] + [t.grad for t in ins])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.fixture
def sort_mode():
    """Selects the radix sort's form (three launches per pass / the one-sweep A/B form) for one test."""
    from street_gaussians_amd import _C
    prev = _C.test_switches()

    def set_mode(one_sweep):
        if one_sweep and not _C.has_variants():
            pytest.skip("the one-sweep sort is an A/B design outside the shipped library (tools/build_variant.py)")
        _C.test_switches((prev & ~_C.USE_ONESWEEP) | (_C.USE_ONESWEEP if one_sweep else 0))
    yield set_mode
    _C.test_switches(prev)


@pytest.mark.parametrize("n,count,end_bit,max_bits", [(1, 0, 14, 8), (1, 1, 14, 8), (4097, 2048, 14, 8),
                                                      (4097, 4096, 27, 9), (100_000, 61_234, 25, 8),
                                                      (2_500_000, 600_001, 32, 8), (3_500_000, 3_100_000, 27, 9)])
@pytest.mark.parametrize("one_sweep", [False, True])
def test_device_count_sort_equals_the_host_count_sort_of_the_prefix(n, count, end_bit, max_bits, one_sweep, sort_mode):
    L, check = _lib()
    sort_mode(one_sweep)
    rng = np.random.default_rng(n + count)
    keys = rng.integers(0, 1 << end_bit, n, dtype=np.uint64).astype(np.uint32)
    keys[: count // 2] = keys[: count // 2] & 0xFF  # duplicates: stability matters
    SENT = np.int32(-559038737)  # 0xDEADBEEF
    k0 = torch.from_numpy(keys.view(np.int32)).cuda()
    k0[count:] = SENT
    v0 = torch.arange(n, dtype=torch.int32, device=DEV) * 3 + 1
    v0[count:] = SENT
    k1, v1 = torch.full_like(k0, SENT), torch.full_like(v0, SENT)
    hist = torch.zeros(L.sgr_test_sort_hist_words(n), dtype=torch.int32, device=DEV)
    tmp = torch.zeros(L.sgr_test_scan_tmp_words(hist.numel()), dtype=torch.int32, device=DEV)
    dn = torch.tensor([count], dtype=torch.int32, device=DEV)
    cur = check(L.sgr_test_sort32_count(_vp(k0), _vp(k1), _vp(v0), _vp(v1), n, end_bit, max_bits, _vp(dn), _vp(hist),
                                        _vp(tmp), _stream()))
    torch.cuda.synchronize()
    for t in (k0, k1, v0, v1):
        assert (t[count:] == SENT).all()
    if count:
        hk0 = torch.from_numpy(keys[:count].view(np.int32)).cuda()
        hv0 = torch.arange(count, dtype=torch.int32, device=DEV) * 3 + 1
        hk1, hv1 = torch.zeros_like(hk0), torch.zeros_like(hv0)
        hh = torch.zeros(L.sgr_test_sort_hist_words(count), dtype=torch.int32, device=DEV)
        ht = torch.zeros(L.sgr_test_scan_tmp_words(hh.numel()), dtype=torch.int32, device=DEV)
        hc = check(L.sgr_test_sort32(_vp(hk0), _vp(hk1), _vp(hv0), _vp(hv1), count, end_bit, max_bits, _vp(hh), _vp(ht),
                                     _stream()))
        torch.cuda.synchronize()
        assert torch.equal((k1 if cur else k0)[:count], (hk1 if hc else hk0))
        assert torch.equal((v1 if cur else v0)[:count], (hv1 if hc else hv0))
        order = np.argsort(keys[:count], kind="stable")
        assert np.array_equal((k1 if cur else k0)[:count].cpu().numpy().view(np.uint32), keys[:count][order])


# ---- 9. the reference's call site -------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1280, 1920), (1066, 1600)])
def test_reference_call_site_at_full_frame(H, W):
    R = 1024
    g = torch.Generator().manual_seed(H)
    rgb = (torch.rand(3, H, W, generator=g) * 0.8).to(DEV)
    acc = torch.rand(1, H, W, generator=g).to(DEV)
    sky_mask = torch.zeros(1, H, W, dtype=torch.bool)
    sky_mask[:, : H // 4] = True
    sky_mask = sky_mask.to(DEV)
    acc[sky_mask] = 0.0
    cube = torch.rand(6, R, R, 3, generator=g).to(DEV)
    affine = torch.cat([torch.eye(3) + 0.05 * torch.randn(3, 3, generator=g), 0.02 * torch.randn(3, 1, generator=g)],
                       1).to(DEV)
    perturb = torch.rand(2, H, W, generator=g).to(DEV)
    t_norm = 5.0
    K, w2c = _camera(H, W, yaw_deg=45.0, t_norm=t_norm, seed=H)  # the view straddles the +x / +z face edge
    out = _sky(rgb, acc, cube, K, w2c, sky_mask=sky_mask, affine=affine, perturb=perturb)
    ref = rs.render_step2(rgb.double(), acc.double(), cube.double(), K, w2c, sky_mask=sky_mask, affine=affine,
                          perturb=perturb)
    ray = 8 * 2.0 ** -24 * (1 + t_norm)
    tol = (2e-7 * R + 2 * math.sqrt(3) * R * ray) * affine[:, :3].abs().sum(1).max().item() + 1e-5
    err = (out.double() - ref).abs()
    assert err.max().item() <= tol, f"|err| {err.max().item():.3e} > {tol:.3e}"
    # the non-sky pixels do not see the lookup at all: tight there
    assert err[:, ~rs.sky_mask_of(acc, sky_mask, True)].max().item() <= 1e-6
