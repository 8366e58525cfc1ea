"""CPU tests of the object-alpha head (include/sgr_object_alpha.h, GaussianRasterizer.forward_with_object_alpha): the two
entry points are declared, bound in both bindings and exported; they refuse bad arguments before they touch the GPU or the
allocation callback; the Python method raises what ``forward`` raises; and the arithmetic the header states for the
backward -- the alpha part of the reference's backward over the subset's own lists -- is pinned in float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import oracle_kwargs, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGR_E_INVALID = 1  # include/sgr.h
NAMES = ("sgr_layer_alpha_forward", "sgr_layer_alpha_backward")


@pytest.fixture(scope="module")
def native():
    from street_gaussians_amd import _native, build
    build.build()  # hipcc cross-compiles for gfx950; a no-op when the objects are up to date
    return _native


def test_entry_points_are_declared_bound_and_exported(native):
    text = open(os.path.join(ROOT, "include", "sgr_object_alpha.h")).read()
    for n in NAMES:
        assert re.search(r"^int\s+" + n + r"\s*\(", text, re.M), n
    # the header states the arithmetic against the reference's lines
    for ref in ("train.py:114-122", "street_gaussian_renderer.py:58-72", "forward.cu:431-445", "backward.cu:505-640"):
        assert ref in text, ref
    lib = C.CDLL(native.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in native.SIGNATURES, n
    lib.sgr_version.restype = C.c_int
    assert lib.sgr_version() >= 105
    # the source is part of the library's build, and both bindings carry both calls
    from street_gaussians_amd import _C, build
    assert "sgr_object_alpha.hip" in build.SOURCES
    assert callable(_C.layer_alpha_forward) and callable(_C.layer_alpha_backward)
    ext = open(os.path.join(ROOT, "street_gaussians_amd", "csrc", "ext.cpp")).read()
    for n in NAMES:
        assert n + "(" in ext, n
    assert 'm.def("layer_alpha_forward"' in ext and 'm.def("layer_alpha_backward"' in ext
    build.build_pybind()
    from street_gaussians_amd import _C_pybind
    assert hasattr(_C_pybind, "layer_alpha_forward") and hasattr(_C_pybind, "layer_alpha_backward")


# addresses that are never dereferenced: every call below must return before it reaches the GPU
A = [C.c_void_p(0x1000 * (k + 1)) for k in range(16)]


def _forward(native, P=8, R=4, W=32, H=32, split=4, geom=A[0], binning=A[1], image=A[2], out_alpha=A[3], out_last=A[4]):
    return native.lib().sgr_layer_alpha_forward(P, R, W, H, split, geom, binning, image, out_alpha, out_last, None)


def _backward(native, calls, P=8, R=4, W=32, H=32, split=4, means3D=A[0], scales=A[1], rotations=A[2], cov3D=None,
              geom=A[3], binning=A[4], image=A[5], layer_alpha=A[6], layer_last=A[7], dL=A[8], d_mean=A[9], d_opa=A[10],
              d_scale=A[11], d_rot=A[12], with_cb=True):
    def alloc(nbytes, _user):
        calls.append(int(nbytes))
        return None
    cb = native.ALLOC_FN(alloc) if with_cb else native.ALLOC_FN()
    return native.lib().sgr_layer_alpha_backward(P, R, W, H, split, means3D, scales, 1.0, rotations, cov3D, None, geom, binning,
                                                 image, layer_alpha, layer_last, dL, d_mean, d_opa, d_scale, d_rot, None, cb,
                                                 None, 0, None)


def test_bad_arguments_are_refused_before_anything_runs(native):
    err = lambda: native.lib().sgr_last_error().decode()
    fwd_cases = [(dict(split=-1), "split"), (dict(split=9), "split"), (dict(out_alpha=None), "out_alpha"),
                 (dict(out_last=None), "out_last"), (dict(geom=None), "buffers"), (dict(image=None), "buffers"),
                 (dict(binning=None), "buffers"), (dict(W=0), "width"), (dict(P=-1), "P")]
    for kw, word in fwd_cases:
        rc = _forward(native, **kw)
        assert rc == -SGR_E_INVALID, (kw, rc)
        assert word in err(), (kw, err())
    bwd_cases = [(dict(split=-1), "split"), (dict(split=9), "split"), (dict(means3D=None), "means3D"),
                 (dict(layer_alpha=None), "layer_alpha"), (dict(layer_last=None), "layer_last"), (dict(dL=None), "dL_dlayer_alpha"),
                 (dict(d_mean=None), "dL_dmean3D"), (dict(d_opa=None), "dL_dopacity"), (dict(d_scale=None), "dL_dscale"),
                 (dict(d_rot=None), "dL_drot"), (dict(geom=None), "buffers"), (dict(binning=None), "buffers"),
                 (dict(scales=None), "exactly one"), (dict(cov3D=A[13]), "exactly one"), (dict(with_cb=False), "scratch")]
    for kw, word in bwd_cases:
        calls = []
        rc = _backward(native, calls, **kw)
        assert rc == -SGR_E_INVALID, (kw, rc)
        assert word in err(), (kw, err())
        assert calls == [], kw
    # an empty set of Gaussians is not an error and asks for nothing
    calls = []
    assert _backward(native, calls, P=0, R=0, split=0, geom=None, binning=None, image=None) == 0
    assert calls == []


def test_forward_with_object_alpha_raises_what_forward_raises():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from street_gaussians_amd._native import SgrError
    assert hasattr(GaussianRasterizer, "forward_with_object_alpha")
    st = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False)
    z = torch.zeros
    rast = GaussianRasterizer(st)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        rast.forward_with_object_alpha(z(4, 3), None, z(4, 1), scales=z(4, 3), rotations=z(4, 4), split=2)
    with pytest.raises(Exception, match="scale/rotation pair"):
        rast.forward_with_object_alpha(z(4, 3), None, z(4, 1), shs=z(4, 1, 3), scales=z(4, 3), split=2)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="split"):
            rast.forward_with_object_alpha(z(4, 3), None, z(4, 1), shs=z(4, 1, 3), scales=z(4, 3), rotations=z(4, 4), split=bad)
    # CPU tensors: there is no CPU path -- the error and its message are forward's
    args = dict(shs=z(4, 1, 3), scales=z(4, 3), rotations=z(4, 4))
    with pytest.raises(SgrError) as want:
        rast(z(4, 3), None, z(4, 1), **args)
    with pytest.raises(SgrError) as got:
        rast.forward_with_object_alpha(z(4, 3), None, z(4, 1), **args, split=2)
    assert str(got.value) == str(want.value)


def test_alpha_backward_arithmetic_in_float64():
    """The statement of include/sgr_object_alpha.h, pinned without a GPU: the gradient of sum(w * alpha) of the SUBSET's
    render -- float64 autograd through tests/torch_ref.py over the subset's own oracle lists -- equals the reference
    algorithm's backward (the C oracle, float32) over the subset with the upstream gradient on alpha only.

    Bound: 3e-4 of the tensor's largest entry + 1e-9, the bound tests/test_oracle.py holds the same pair of implementations
    to on its non-saturating cases (the float32 oracle's own rounding against float64); nothing of the library under test
    enters."""
    import torch_ref as tr
    from oracle import oracle
    cam, sc = small_case(P=60)
    split = 24
    W, H = cam.image_width, cam.image_height
    kw = oracle_kwargs(cam, sc, semantics=False)
    per = ("means3D", "opacities", "shs", "scales", "rotations")
    sub = {k: (v[split:] if k in per else v) for k, v in kw.items()}
    fw = oracle.forward(**sub)
    assert fw.num_rendered > 0 and (fw.radii > 0).sum() > 5

    d = lambda t: t[split:].double().clone().requires_grad_(True)
    m3, s, q, o, sh = map(d, (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs))
    pre = tr.preprocess(m3, cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx, cam.tanfovy, W, H, 3, o, shs=sh,
                        scales=s, rotations=q)
    pl = torch.from_numpy(fw.point_list.astype(np.int64))
    _, _, alp, _, _ = tr.render(pre, pl, fw.ranges, W, H, torch.zeros(3), None)
    assert np.abs(alp.detach().numpy() - fw.alpha).max() < 2e-5
    assert fw.alpha.max() > 0.2
    w = torch.rand(1, H, W, generator=torch.Generator().manual_seed(11)) * 2.0 - 1.0
    (alp * w.double()).sum().backward()
    g = oracle.backward(fw, torch.zeros(3, H, W), torch.zeros(1, H, W), w, None)
    fw.free()
    for name, a, b in [("means3D", m3.grad, g["means3D"]), ("opacity", o.grad, g["opacity"]), ("scales", s.grad, g["scales"]),
                       ("rotations", q.grad, g["rotations"])]:
        a = a.numpy().reshape(b.shape)
        assert np.abs(a).max() > 0, name
        assert np.abs(a - b).max() <= 3e-4 * np.abs(a).max() + 1e-9, f"{name}: {np.abs(a - b).max()} vs {np.abs(a).max()}"
    # an alpha-only upstream gradient leaves the colour path alone
    assert not np.asarray(g["sh"]).any() and (sh.grad is None or not sh.grad.abs().max())
