"""sgr_backward_extras.skip_cov3d_grad: a caller that rasterizes from scales and rotations has no cov3D_precomp for
dL/dcov3D to reach, so the per-Gaussian backward need not write it (24 B per Gaussian).  P = 1027 (no multiple of the
workgroup), 160 x 96, both bindings: with the flag every other gradient is bit-identical, a destination the caller handed
over is left untouched, no destination at all (NULL) is accepted; the autograd wrapper sets the flag exactly when
cov3D_precomp is absent, and its leaves' gradients equal the raw entry point's."""
import numpy as np
import pytest
import torch

from gpu_utils import GRAD_NAMES, dev, raw_backward, raw_forward, settings
from helpers import oracle_kwargs
from oracle import oracle
from street_gaussians_amd import _C
from street_gaussians_amd import synthetic as syn
from jacobian_utils import asking_for_jacobian, backward_with as _backward, jacobian_flag

pytestmark = pytest.mark.gpu

P, W, H = 1027, 160, 96


def _scene():
    cam = syn.make_camera(W, H, fx=170.0, yaw_deg=3.0, translation=(0.05, -0.02, 0.1))
    sc = syn.make_scene(P, cam, S=0, seed=21, margin=1.4, zmin=1.0, zmax=20.0, scale_px=0.01)
    return cam, sc, syn.loss_weights(cam, S=0)


@pytest.fixture(params=["ctypes", "pybind"])
def binding(request):
    prev = _C.binding()
    _C.set_binding(request.param)
    try:
        yield request.param
    finally:
        _C.set_binding(prev)


def test_skip_cov3d_grad_changes_nothing_else(binding):
    cam, sc, wts = _scene()
    kw = oracle_kwargs(cam, sc)
    res, _ = raw_forward(kw)
    g = raw_backward(kw, res, wts)
    assert g["cov3D"].shape == (P, 6) and float(g["cov3D"].abs().max()) > 0  # the raw entry point keeps returning it
    gs = _backward(kw, res, wts, skip_cov3d_grad=True)  # no destination: NULL goes down
    torch.cuda.synchronize()
    assert gs["cov3D"] is None or gs["cov3D"].numel() == 0
    for k in GRAD_NAMES:
        if k != "cov3D":
            assert torch.equal(g[k], gs[k]), k


def test_a_destination_handed_over_is_left_untouched():
    cam, sc, wts = _scene()
    kw = oracle_kwargs(cam, sc)
    prev = _C.binding()
    _C.set_binding("ctypes")  # caller-supplied destinations are an extension of the ctypes binding
    try:
        res, _ = raw_forward(kw)
        g = raw_backward(kw, res, wts)
        sentinel = torch.full((P, 6), -12345.5, device="cuda")
        gs = _backward(kw, res, wts, skip_cov3d_grad=True, out={"cov3D": sentinel})
        torch.cuda.synchronize()
    finally:
        _C.set_binding(prev)
    assert gs["cov3D"] is sentinel and bool((sentinel == -12345.5).all())
    for k in GRAD_NAMES:
        if k != "cov3D":
            assert torch.equal(g[k], gs[k]), k


def _leaves(sc, names):
    return {k: dev(getattr(sc, k)).requires_grad_(True) for k in names}


def _loss(outs, wts):
    color, radii, depth, alpha, sem = outs
    return (color * dev(wts["color"])).sum() + (depth * dev(wts["depth"])).sum() + (alpha * dev(wts["alpha"])).sum()


def test_wrapper_with_scales_and_rotations_matches_the_raw_entry_point(binding):
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc, wts = _scene()
    t = _leaves(sc, ["means3D", "scales", "rotations", "opacities", "shs"])
    m2d = torch.zeros(P, 3, device="cuda", requires_grad=True)
    outs = GaussianRasterizer(settings(cam))(t["means3D"], m2d, t["opacities"], shs=t["shs"], scales=t["scales"],
                                              rotations=t["rotations"])
    _loss(outs, wts).backward()
    # the raw entry points on the same inputs: a forward that asks for the colour Jacobian, as the wrapper's does
    kw = oracle_kwargs(cam, sc)
    kw["bg"] = torch.zeros(3)
    with asking_for_jacobian():
        res, _ = raw_forward(kw)
    g = raw_backward(kw, res, wts)
    torch.cuda.synchronize()
    pairs = [("means3D", t["means3D"]), ("scales", t["scales"]), ("rotations", t["rotations"]), ("sh", t["shs"]), ("means2D", m2d)]
    for k, leaf in pairs:
        assert torch.equal(leaf.grad, g[k].reshape(leaf.shape)), k
    assert torch.equal(t["opacities"].grad.reshape(-1), g["opacity"].reshape(-1))


def test_wrapper_with_cov3D_precomp_still_gets_its_gradient(binding):
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc, wts = _scene()
    fw0 = oracle.forward(**oracle_kwargs(cam, sc))
    cov6 = torch.from_numpy(np.asarray(fw0.cov3D).copy()).float()
    fw0.free()
    t = _leaves(sc, ["means3D", "opacities", "shs"])
    cov = dev(cov6).requires_grad_(True)
    outs = GaussianRasterizer(settings(cam))(t["means3D"], None, t["opacities"], shs=t["shs"], cov3D_precomp=cov)
    _loss(outs, wts).backward()
    kw = oracle_kwargs(cam, sc, use_cov_precomp=True, cov3D=cov6)
    with asking_for_jacobian():
        res, _ = raw_forward(kw)
    g = raw_backward(kw, res, wts)
    torch.cuda.synchronize()
    assert cov.grad is not None and float(cov.grad.abs().max()) > 0
    assert torch.equal(cov.grad, g["cov3D"])
    assert torch.equal(t["means3D"].grad, g["means3D"])


def test_wrapper_asks_for_the_jacobian_only_when_a_backward_can_follow():
    """Inference renders (no_grad, or no input that requires grad) leave header word 8 at zero; a training render sets it."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from street_gaussians_amd import rasterizer as rz
    cam, sc, wts = _scene()
    seen = []
    orig = _C.rasterize_gaussians

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(jacobian_flag(out[6]))
        return out
    rz._C.rasterize_gaussians = spy
    try:
        rast = GaussianRasterizer(settings(cam))
        t = _leaves(sc, ["means3D", "scales", "rotations", "opacities", "shs"])
        call = lambda d: rast(d["means3D"], None, d["opacities"], shs=d["shs"], scales=d["scales"], rotations=d["rotations"])
        call(t)                                       # training render
        with torch.no_grad():
            call(t)                                   # grad mode off
        call({k: v.detach() for k, v in t.items()})   # nothing requires grad
        torch.cuda.synchronize()
    finally:
        rz._C.rasterize_gaussians = orig
    assert seen == [1, 0, 0], seen
