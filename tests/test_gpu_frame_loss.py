"""`-m gpu` tests of losses.frame_loss / losses.psnr (csrc/sgr_frame_loss.hip) against the float64 pins of
tests/golden/frame_loss/pins.npz, the float64 CPU restatement tests/torch_ref_frame_loss.py and the composition of the
stand-alone GPU ops.  Bounds are those of tests/test_gpu_loss.py for the same terms: values 5e-6 relative, SSIM 5e-6
absolute, gradients 3e-5 x max |want|.  PSNR: mse is held to 5e-6 relative, which moves 20 log10(1 / sqrt(mse)) by
(10 / ln 10) * 5e-6 = 2.2e-5 dB; plus one float32 ulp at 40 dB (3.8e-6) and rounded up: 5e-5 dB.

No kernel of sgr_frame_loss.hip caps its grid or walks a grid-stride loop over pixels (one workgroup per tile, one lane
per pixel).  The finishing workgroups loop over the block sums, sgr_frame_loss_finish_span() of them per trip, four per
lane: (3, 320, 480) (600 tiles / 600 pixel blocks) gives a lane several sums and a clamped load past the end, and the
past-the-span cases, sized from that constant, give the loop its second trip."""
import numpy as np
import pytest
import torch

import torch_ref_frame_loss as ref
from golden import make_frame_loss_fixture as mk
from street_gaussians_amd import losses

pytestmark = pytest.mark.gpu

REL, SSIM_ABS, GRAD, PSNR_DB = 5e-6, 5e-6, 3e-5, 5e-5
W8 = dict(lambda_dssim=0.2, lambda_l1=1.0, lambda_sky=0.05, lambda_reg=0.1, lambda_depth_lidar=0.1)
LEAVES = ("image", "acc", "depth", "acc_obj")


def check_scalar(name, got, want):
    got, want = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (got, want))
    print(f"  {name}: got {got!r} want {want!r} |diff| {abs(got - want):.3e}")
    if np.isnan(want):
        assert np.isnan(got), name
    elif name == "ssim":
        assert abs(got - want) <= SSIM_ABS, name
    elif name == "psnr":
        assert abs(got - want) <= PSNR_DB, name
    else:
        assert abs(got - want) <= REL * abs(want), name


def check_grad(name, got, want):
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    got = got.detach().cpu().double().reshape(-1)
    scale, err = float(want.abs().max()), float((got - want).abs().max())
    print(f"  d_{name}: max err {err:.3e} = {err / scale if scale else 0.0:.3e} x max |want|")
    assert err <= GRAD * scale, name


def make_inputs(C, H, W, seed, masked=True):
    """Seeded CPU inputs with both clamps of acc active (rows 0-1 at 0, rows 2-3 at 1) and no LiDAR return where nothing
    was accumulated.  (5 rows at least.)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    image = r(C, H, W)
    gt = (image + 0.2 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
    acc = r(1, H, W) * 0.95 + 0.05
    acc[0, :2], acc[0, 2:4] = 0.0, 1.0
    lidar = torch.where(r(1, H, W) < 0.4, r(1, H, W) * 60, torch.zeros(1, H, W))
    lidar[0, :2] = 0.0
    return dict(image=image, gt=gt, acc=acc, acc_obj=r(1, H, W), depth=r(1, H, W) * 40, lidar=lidar,
                mask=(r(1, H, W) < 0.8) if masked else None, sky_mask=r(1, H, W) < 0.3, obj_bound=r(1, H, W) < 0.3)


def kwargs_of(inp, terms, leaves, to):
    """frame_loss keyword arguments for the term subset `terms` (of 'sky', 'obj', 'lidar')."""
    kw = dict(lambda_dssim=W8["lambda_dssim"], lambda_l1=W8["lambda_l1"])
    if "sky" in terms:
        kw.update(acc=leaves["acc"], sky_mask=to(inp["sky_mask"]), lambda_sky=W8["lambda_sky"])
    if "obj" in terms:
        kw.update(acc_obj=leaves["acc_obj"], obj_bound=to(inp["obj_bound"]), lambda_reg=W8["lambda_reg"])
    if "lidar" in terms:
        kw.update(acc=leaves["acc"], depth=leaves["depth"], lidar_depth=to(inp["lidar"]), lambda_depth_lidar=W8["lambda_depth_lidar"])
    return kw


def run_gpu(inp, terms=("sky", "obj", "lidar"), sky_scale=None, requires=LEAVES):
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    leaves = {k: inp[k].cuda().requires_grad_(k in requires) for k in LEAVES}
    kw = kwargs_of(inp, terms, leaves, dev)
    if sky_scale is not None:
        kw["sky_scale"] = sky_scale
    loss, t = losses.frame_loss(leaves["image"], dev(inp["gt"]), dev(inp["mask"]), **kw)
    loss.backward()
    return loss, t, leaves


def run_ref(inp, terms=("sky", "obj", "lidar"), sky_scale=None):
    """The float64 restatement on the CPU."""
    f64 = lambda t: t.double() if t.is_floating_point() else t  # noqa: E731
    leaves = {k: inp[k].double().requires_grad_(True) for k in LEAVES}
    out = ref.frame_loss(leaves["image"], inp["gt"].double(), inp["mask"], sky_scale=sky_scale, **kwargs_of(inp, terms, leaves, f64))
    out["loss"].backward()
    return out, leaves


def used(terms):
    return ("image",) + (("acc",) if {"sky", "lidar"} & set(terms) else ()) + (("depth",) if "lidar" in terms else ()) + \
        (("acc_obj",) if "obj" in terms else ())


def compare(inp, terms=("sky", "obj", "lidar"), sky_scale=None):
    loss, t, leaves = run_gpu(inp, terms, sky_scale)
    want, wl = run_ref(inp, terms, sky_scale)
    vals = t.values.tolist()  # the one read-back
    assert vals[7] == loss.item() and t._fields[:8] == ref.NAMES
    for i, k in enumerate(ref.NAMES):
        check_scalar(k, vals[i], want[k])
        assert getattr(t, k).dim() == 0 and not getattr(t, k).requires_grad
    for k in LEAVES:
        if k in used(terms):
            check_grad(k, leaves[k].grad, wl[k].grad)
        else:
            assert leaves[k].grad is None, k
    if inp["mask"] is not None:
        assert float(leaves["image"].grad[:, ~inp["mask"][0].cuda()].abs().max()) == 0.0
    if "sky" in terms and "lidar" not in terms:
        assert float(leaves["acc"].grad[0, :4].abs().max()) == 0.0  # both clamps active: exactly zero
    if "sky" in terms:
        assert float(leaves["acc"].grad[0, :2].abs().max()) == 0.0  # acc = 0: clamp active and no LiDAR return
    return loss, t, leaves


# ---- the fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mk.CASES))
def test_fixture_cases_against_the_float64_pins(name):
    d = mk.load()
    c = mk.case(d, name)
    inp = {k: torch.from_numpy(d[k]) for k in ("image", "gt", "acc", "acc_obj", "depth", "lidar", "mask", "sky_mask", "obj_bound")}
    if not c["masked"]:
        inp["mask"] = None
    loss, t, leaves = run_gpu(inp, sky_scale=None if np.isnan(c["sky_scale"]) else float(c["sky_scale"]))
    vals = t.values.tolist()
    pin_of = {"l1": "l1_loss", "ssim": "ssim", "sky": "sky_loss", "obj": "obj_acc_loss", "lidar": "lidar_depth_loss", "mse": "mse",
              "psnr": "psnr", "loss": "loss"}
    for i, k in enumerate(ref.NAMES):
        want = float(c[pin_of[k] + "64"])
        print(f"  {k}: needs {abs(vals[i] - want) / (float(d['e_ref_' + pin_of[k]]) * abs(want)):.2f} x e_ref")
        check_scalar(k, vals[i], want)
    for k in LEAVES:
        want = c[f"d_{k}64"]
        err = np.abs(leaves[k].grad.cpu().double().numpy() - want).max()
        print(f"  d_{k}: needs {err / (float(d['e_ref_d_' + k]) * np.abs(want).max()):.2f} x e_ref")
        check_grad(k, leaves[k].grad, want)
    assert float(leaves["acc"].grad[0, :3].abs().max()) == 0.0
    if c["masked"]:
        assert float(leaves["image"].grad[:, ~inp["mask"][0].cuda()].abs().max()) == 0.0


# ---- shapes where the tile kernels can go wrong -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,masked", [(3, 5, 7, True), (1, 16, 16, False), (3, 131, 77, True), (3, 320, 480, True)])
def test_all_terms_match_the_float64_restatement(C, H, W, masked):
    if (H, W) == (320, 480):  # more block sums than lanes: a finishing lane adds several, the last of its loads past the end
        assert 2 * 256 < _lib().sgr_frame_loss_workspace_floats(C, H, W) // 6 < 3 * 256
    compare(make_inputs(C, H, W, H * 1000 + W, masked))


def _lib():
    from street_gaussians_amd import _native
    return _native.lib()


def test_all_terms_past_the_finishing_span():
    """The smallest image (33 tiles wide, ragged both ways) whose tiles give the finishing workgroup's loop a second trip."""
    span, gx = _lib().sgr_frame_loss_finish_span(), 33
    gy = -(-(span + 1) // gx)
    H, W = 16 * gy - 3, 16 * gx - 15
    tiles = _lib().sgr_frame_loss_workspace_floats(1, H, W) // 6
    assert span < tiles <= span + gx, (span, tiles)  # were the span raised, this says so instead of passing for nothing
    compare(make_inputs(1, H, W, 77, True))


@pytest.mark.parametrize("masked", [False, True])
def test_psnr_past_the_finishing_span(masked):
    span = _lib().sgr_frame_loss_finish_span()
    H, W = 2 * span + 3, 128  # 256-pixel blocks: span + 2 of them, the last one ragged
    blocks = _lib().sgr_mse_workspace_floats(3, H, W) // 2
    assert span < blocks <= span + 2, (span, blocks)
    inp = make_inputs(3, H, W, 23, masked)
    want = ref.psnr(inp["image"].double(), inp["gt"].double(), inp["mask"])
    check_scalar("psnr", losses.psnr(inp["image"].cuda(), inp["gt"].cuda(), None if inp["mask"] is None else inp["mask"].cuda()), want)


@pytest.mark.parametrize("terms,masked", [((), True), (("sky",), True), (("obj",), True), (("lidar",), False),
                                           (("sky", "obj", "lidar"), True)])
def test_term_subsets(terms, masked):
    inp = make_inputs(3, 67, 45, 11, masked)
    loss, t, leaves = compare(inp, terms, sky_scale=1.3 if "sky" in terms else None)
    vals = t.values.tolist()
    for i, k in ((2, "sky"), (3, "obj"), (4, "lidar")):
        assert (vals[i] != 0.0) == (k in terms), k  # a term that is off is written as 0
    if not terms:  # colour only: the fused colour op, to the same bounds
        x = inp["image"].cuda().requires_grad_(True)
        want, l1 = losses.color_loss(x, inp["gt"].cuda(), inp["mask"].cuda(), lambda_dssim=0.2, return_l1=True)
        want.backward()
        check_scalar("loss", loss, want)
        check_scalar("l1", t.l1, l1)
        check_grad("image", leaves["image"].grad, x.grad.cpu())


def test_matches_the_composition_of_the_stand_alone_ops():
    inp = make_inputs(3, 131, 77, 5)
    loss, t, leaves = run_gpu(inp, sky_scale=0.7)
    dev = {k: (v.cuda() if v is not None else None) for k, v in inp.items()}
    lv = {k: dev[k].clone().requires_grad_(True) for k in LEAVES}
    sky = losses.sky_loss(lv["acc"], dev["sky_mask"]) * 0.7
    obj = losses.obj_acc_loss(lv["acc_obj"], dev["obj_bound"])
    lidar = losses.lidar_depth_loss(lv["depth"], lv["acc"], dev["lidar"], dev["mask"])
    col, l1 = losses.color_loss(lv["image"], dev["gt"], dev["mask"], lambda_dssim=0.2, return_l1=True)
    want = col + W8["lambda_sky"] * sky + W8["lambda_reg"] * obj + W8["lambda_depth_lidar"] * lidar
    want.backward()
    for k, w in (("l1", l1), ("sky", sky), ("obj", obj), ("lidar", lidar), ("loss", want)):
        check_scalar(k, getattr(t, k), w)
    for k in LEAVES:
        check_grad(k, leaves[k].grad, lv[k].grad.cpu())


# ---- gradient subsets ------------------------------------------------------------------------------------------------------
def test_only_the_inputs_that_require_grad_get_one():
    inp = make_inputs(3, 37, 53, 3)
    _, _, every = run_gpu(inp)
    _, _, only_image = run_gpu(inp, requires=("image",))
    assert torch.equal(only_image["image"].grad, every["image"].grad)
    assert all(only_image[k].grad is None for k in ("acc", "depth", "acc_obj"))
    _, _, only_acc = run_gpu(inp, requires=("acc",))
    assert torch.equal(only_acc["acc"].grad, every["acc"].grad)  # sky + LiDAR, both through acc
    assert all(only_acc[k].grad is None for k in ("image", "depth", "acc_obj"))
    # acc appears in both terms: its gradient is the sum of the two single-term gradients
    _, _, sky = run_gpu(inp, terms=("sky",))
    _, _, lidar = run_gpu(inp, terms=("lidar",))
    both = sky["acc"].grad.double() + lidar["acc"].grad.double()
    check_grad("acc", every["acc"].grad, both.cpu())
    assert float(sky["acc"].grad[0, :4].abs().max()) == 0.0
    assert float(lidar["acc"].grad[0, 2:4].abs().max()) > 0.0
    assert float(every["image"].grad[:, ~inp["mask"][0].cuda()].abs().max()) == 0.0
    # nothing requires grad: no graph, same numbers
    dev = lambda t: t.cuda()  # noqa: E731
    loss, t = losses.frame_loss(dev(inp["image"]), dev(inp["gt"]), dev(inp["mask"]), acc=dev(inp["acc"]), sky_mask=dev(inp["sky_mask"]),
                                lambda_sky=W8["lambda_sky"])
    assert not loss.requires_grad and float(t.sky) > 0


# ---- edge behaviour -----------------------------------------------------------------------------------------------------------
def test_edge_behaviour_of_the_terms():
    z = torch.zeros(1, 8, 8, device="cuda")
    x = torch.rand(3, 8, 8, device="cuda")
    # an empty mask: l1, mse and psnr are NaN (the mean of nothing); no LiDAR pixel: lidar is NaN
    _, t = losses.frame_loss(x, x.flip(0), z > 1, acc=z + 1, depth=z + 1, lidar_depth=z, lambda_depth_lidar=0.1)
    v = t.values.tolist()
    assert np.isnan(v[0]) and np.isnan(v[4]) and np.isnan(v[5]) and np.isnan(v[7])
    # every error is exactly 2: the mean is 2 and the ties share the slots, so the gradient sums to one
    d = (z + 3.0).requires_grad_(True)
    loss, t = losses.frame_loss(x, x, None, lambda_dssim=0.2, acc=z + 1, depth=d, lidar_depth=z + 1, lambda_depth_lidar=1.0)
    assert t.lidar.item() == pytest.approx(2.0) and t.l1.item() == 0.0 and t.ssim.item() == pytest.approx(1.0, abs=1e-6)
    assert loss.item() == pytest.approx(2.0, rel=1e-6)
    loss.backward()
    assert float(d.grad.sum()) == pytest.approx(1.0, rel=1e-5)
    # int(0.95 * 100) == 95 in double (0.95f * 100 would truncate to 94): errors 1..100 -> the mean of the 95 smallest is 48
    for n, k in ((100, 95), (20, 19), (40, 38), (2000, 1900)):
        err = torch.arange(1, n + 1, dtype=torch.float32, device="cuda")[torch.randperm(n, device="cuda")]
        depth, lidar = (err + 10.0).reshape(1, 1, n), torch.full((1, 1, n), 10.0, device="cuda")
        img = torch.rand(3, 1, n, device="cuda")
        _, t = losses.frame_loss(img, img, None, acc=torch.ones_like(depth), depth=depth, lidar_depth=lidar, lambda_depth_lidar=0.1)
        assert int(0.95 * n) == k and t.lidar.item() == pytest.approx((k + 1) / 2.0, rel=1e-6), n


def test_no_host_wait_and_bit_reproducible():
    inp = make_inputs(3, 131, 77, 9)
    dev = {k: (v.cuda() if v is not None else None) for k, v in inp.items()}
    runs = []
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            lv = {k: dev[k].clone().requires_grad_(True) for k in LEAVES}
            loss, t = losses.frame_loss(lv["image"], dev["gt"], dev["mask"], acc=lv["acc"], sky_mask=dev["sky_mask"], lambda_sky=0.05,
                                        sky_scale=1.3, acc_obj=lv["acc_obj"], obj_bound=dev["obj_bound"], lambda_reg=0.1,
                                        depth=lv["depth"], lidar_depth=dev["lidar"], lambda_depth_lidar=0.1)
            loss.backward()
            with torch.no_grad():
                p = losses.psnr(lv["image"], dev["gt"], dev["mask"])
            runs.append((t.values, p, [lv[k].grad for k in LEAVES]))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    (v0, p0, g0), (v1, p1, g1) = runs
    assert torch.equal(v0, v1) and torch.equal(p0, p1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert abs(p0.item() - v0[6].item()) <= PSNR_DB  # the same number from the two entry points


# ---- psnr ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("C,H,W", [(3, 5, 7), (3, 320, 480)])
def test_psnr_matches_the_float64_reference(C, H, W, masked):
    inp = make_inputs(C, H, W, 21, masked)
    want = ref.psnr(inp["image"].double(), inp["gt"].double(), inp["mask"])
    got = losses.psnr(inp["image"].cuda(), inp["gt"].cuda(), None if inp["mask"] is None else inp["mask"].cuda())
    assert got.dim() == 0
    check_scalar("psnr", got, want)


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from street_gaussians_amd._native import SgrError
    x, m = torch.rand(3, 8, 8, device="cuda"), torch.rand(1, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        losses.frame_loss(x, x, acc=m)
    with pytest.raises(ValueError):
        losses.frame_loss(x, x, depth=m, lidar_depth=m)  # no acc
    with pytest.raises(RuntimeError, match="same shape"):
        losses.frame_loss(x, x[:, :4])
    with pytest.raises(RuntimeError):
        losses.frame_loss(x, x, acc=m[:, :4], sky_mask=m[:, :4] > 0.5)
    with pytest.raises(RuntimeError):
        losses.frame_loss(x, x, torch.ones(2, 8, 8, device="cuda") > 0)
    with pytest.raises(SgrError, match="no CPU path"):
        losses.frame_loss(x, x, acc=m.cpu(), sky_mask=m > 0.5)
    with pytest.raises(ValueError, match="not differentiable"):
        losses.psnr(x.clone().requires_grad_(True), x)
    with pytest.raises(RuntimeError, match="same shape"):
        losses.psnr(x, x[:, :4])
    assert float(losses.psnr(x, x)) == float("inf")
    # the C ABI refuses half a pair too
    import ctypes as C
    from street_gaussians_amd import _native
    a = losses._FrameLossArgs(x.data_ptr(), x.data_ptr(), None, m.data_ptr(), None, None, None, None, None, 0.8, 0.2, 0, 1, 0, 0, 0.95)
    rc = _native.lib().sgr_frame_loss_forward(3, 8, 8, C.addressof(a), 1, 1, 1, None)
    assert rc < 0 and b"acc" in _native.lib().sgr_last_error()
