"""`-m gpu` tests of the rasterizer path under GENERAL cameras (tests/cameras.py): pitch, roll, an off-centre K with
fx != fy, a z-up world basis, skew, and a camera tens of metres from the origin -- what the reference's ``Camera`` hands over
for a real frame.  Every other rasterizer test builds its camera with synthetic.make_camera (yaw about y, a symmetric
frustum), under which view[1], view[4], view[6], view[9] and proj[1], proj[4], proj[7], proj[9] are exactly zero and the
x / y rows of proj are multiples of view's: a good part of the kernels' arithmetic is then multiplied by zero.  The maths
header is held to the oracle under these cameras on the host (tests/test_host_math.py); what only exists on the device --
the packed camera block, the filter kernel's copy of it, the rect / tile / key generation, the per-view camera arrays of
multiview, the Python wrappers -- is held here.

One scene per camera (cameras.gpu_scene: 150 x 100 px, 3000 Gaussians, SH degree 3, two semantic channels; its premises --
Gaussians past the tan-fov clamp in x and in y, behind the camera, culled -- are asserted on the CPU in
tests/test_cameras_cpu.py), one C-oracle forward per camera, shared and left unchanged.

`far` (t = (30, -4, 55)): float32 cancels in view . p + t there, for the reference as for the library.  Integer and
bitwise statements do not care; the float gates are applied as for the other cameras, and in the default mode the library's
images are additionally held to the reference's OWN float32 error against a float64 restatement
(test_far_camera_is_as_close_to_float64_as_the_reference)."""
import functools
import math

import numpy as np
import pytest
import torch

import cameras
import torch_ref as tr
from gpu_utils import (GRAD_NAMES, SAME_STATE_GATE, _log, dev, exact_mode_against_reference_kernels, exact_mode_bit_faithful,
                       grad_close, image_close, npy, oracle_backward_same_state, raw_backward, raw_forward, restrict_oracle,
                       settings, strict_mode_against_reference, switches)
from helpers import oracle_kwargs
from jacobian_utils import asking_for_jacobian
from oracle import oracle
from street_gaussians_amd import _C
from street_gaussians_amd import synthetic as syn

pytestmark = pytest.mark.gpu

MODES = {"default": 0, "exact": _C.EXACT, "strict": _C.EXACT | _C.REF_RECT}
BG = torch.tensor([0.3, 0.1, 0.7])
IMAGES = ("color", "depth", "alpha", "semantic")


@functools.lru_cache(maxsize=None)
def _case(name, S=cameras.GPU_S):
    """-> (cam, scene, oracle-style kwargs, loss weights) of a camera; built once."""
    cam, sc = cameras.gpu_scene(name, S=S)
    sc.shs[::4, 0, :] -= 2.0  # some clamped colour channels
    return cam, sc, oracle_kwargs(cam, sc, deg=3, bg=BG), syn.loss_weights(cam, S=S)


@functools.lru_cache(maxsize=None)
def _oracle_forward(name):
    """The C oracle's forward of a camera's scene: computed once, shared, never modified (nor freed)."""
    return oracle.forward(**_case(name)[2])


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libref_rasterizer.so did not travel (built only where /root/reference exists)")
    return ref


# ---- 1. every camera, every mode, against the C oracle -------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", cameras.NAMES)
def test_camera_against_oracle(name, mode):
    """tests/test_gpu_preprocess_hoist._check under a general camera: radii, num_rendered, tiles_touched, point_list, keys and
    ranges identical to the C oracle's (restricted to the emitted tile rects; with the reference's rects, entry for entry),
    images inside image_close's defaults, every gradient against the oracle's backward on the same forward state inside
    SAME_STATE_GATE, exact zeros for culled Gaussians."""
    cam, sc, kw, wts = _case(name)
    S, P = sc.semantics.shape[1], sc.P
    fw = _oracle_forward(name)
    label = f"camera {name}/{mode}"
    with switches(_C.test_switches(-1) | MODES[mode]):
        res, internal = raw_forward(kw)
        b = restrict_oracle(internal, fw, kw)
        lists = {k: npy(internal(k)).view(dt).reshape(-1) for k, dt in [("tiles_touched", np.uint32), ("point_list", np.uint32),
                                                                        ("keys", np.uint64), ("ranges", np.uint32)]}
        g = raw_backward(kw, res, wts)
        torch.cuda.synchronize()
    culled = fw.radii == 0
    assert culled.any() and not culled.all(), label
    if mode == "strict":  # the reference's own rects: nothing is left out of its lists
        assert b.removed == 0 and b.num_rendered == fw.num_rendered, label
    assert res["R"] == b.num_rendered > 0, label
    assert (npy(res["radii"]) == fw.radii).all(), label
    assert (lists["tiles_touched"] == b.tiles_touched).all(), label
    assert (lists["point_list"] == b.point_list).all(), label
    assert (lists["keys"] == b.keys).all(), label
    assert (lists["ranges"] == b.ranges.reshape(-1)).all(), label
    measured = {}
    for k in IMAGES:
        got, want = npy(res[k]), getattr(fw, k)
        measured[k] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))
        image_close(got, want, name=f"{label}: {k}")
    same = oracle_backward_same_state(oracle, fw, res, wts, S)
    cm = torch.from_numpy(culled)
    for k in GRAD_NAMES:
        a = npy(g[k]).reshape(same[k].shape)
        measured["g_" + k] = float(np.abs(a - same[k]).max() / max(np.abs(same[k]).max(), 1e-30))
        grad_close(a, same[k], name=f"same-state {label}:{k}", **SAME_STATE_GATE)
        assert (g[k].reshape(P, -1).cpu()[cm] == 0).all(), f"{label}: {k}: a culled Gaussian got a gradient"
    if name == "far":  # the measured maxima (over the tensor's scale) at the ill-conditioned translation, for the record
        _log(dict(kind="camera_far", name=label, worst_abs_over_scale=measured))


# ---- 1b. `far`, default mode: the yardstick is the reference's own float32 error -------------------------------------------

@functools.lru_cache(maxsize=None)
def _float64_images(name):
    """tests/torch_ref.py (float64) over the C oracle's lists -> {image: array}; computed once on the CPU."""
    cam, sc, kw, _ = _case(name)
    fw = _oracle_forward(name)
    W, H = cam.image_width, cam.image_height
    d = lambda t: t.double()
    with torch.no_grad():
        pre = tr.preprocess(d(sc.means3D), cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx, cam.tanfovy, W, H, 3,
                            d(sc.opacities), shs=d(sc.shs), scales=d(sc.scales), rotations=d(sc.rotations))
        col, dep, alp, sem, _ = tr.render(pre, torch.from_numpy(fw.point_list.astype(np.int64)), fw.ranges, W, H, BG,
                                          d(sc.semantics))
    return dict(color=col.numpy(), depth=dep.numpy(), alpha=alp.numpy(), semantic=sem.numpy())


def far_errors(name, images):
    """-> {image: (e_ref, e_hip, floor)}: max |C oracle - float64|, max |images - float64| and the absolute floor of
    gpu_utils.image_close (rel 1e-4 of 1e-2 of the image's scale)."""
    fw, f64 = _oracle_forward(name), _float64_images(name)
    out = {}
    for k in IMAGES:
        want = f64[k]
        e_ref = float(np.abs(getattr(fw, k).reshape(want.shape) - want).max())
        e_hip = float(np.abs(np.asarray(images[k], np.float64).reshape(want.shape) - want).max())
        out[k] = (e_ref, e_hip, 1e-4 * 1e-2 * float(np.abs(want).max()))
    return out


def test_far_camera_is_as_close_to_float64_as_the_reference():
    """At t = (30, -4, 55) the float32 reference itself is off the float64 restatement (cancellation in view . p + t).  Per
    output image, e_ref = max |C oracle - float64| and e_hip = max |library - float64|: the library may be no further off
    than 2 e_ref + image_close's absolute floor -- two float32 pipelines round independently, so their errors against
    float64 can add.  Both figures go to the parity log (gpu_utils._log, kind "camera_far_f64"); measured on MI355X
    (profiles/general_cameras/far_measured.jsonl): colour 2.1274e-3 / 2.1273e-3, depth 8.6868e-3 / 8.6861e-3, alpha
    1.76893e-3 / 1.76887e-3, semantic 6.62925e-3 / 6.62929e-3 -- single alpha-threshold flips between float32 and float64
    dominate both sides; the library is within 4e-7 of the C oracle's images."""
    _, _, kw, _ = _case("far")
    res, _ = raw_forward(kw)
    torch.cuda.synchronize()
    errs = far_errors("far", {k: npy(res[k]) for k in IMAGES})
    _log(dict(kind="camera_far_f64", name="camera far/default", **{k: dict(e_ref=v[0], e_hip=v[1], floor=v[2]) for k, v in errs.items()}))
    print("far: e_ref / e_hip / floor per image:", errs)
    for k, (e_ref, e_hip, floor) in errs.items():
        assert e_hip <= 2.0 * e_ref + floor, f"far: {k}: e_hip {e_hip:.3g} > 2 * e_ref {e_ref:.3g} + {floor:.3g}"


# ---- 2. against the reference's own kernels --------------------------------------------------------------------------------

REF_CAMERAS = ["general", "zup", "skewed", "far"]


@pytest.mark.parametrize("name", REF_CAMERAS)
def test_exact_mode_against_reference_kernels(name):
    _ref()
    _, sc, kw, wts = _case(name)
    exact_mode_against_reference_kernels(kw, wts, sc.semantics.shape[1], f"camera {name}")


@pytest.mark.parametrize("name", REF_CAMERAS)
def test_strict_mode_against_reference_kernels(name):
    _ref()
    _, sc, kw, wts = _case(name)
    strict_mode_against_reference(kw, wts, sc.semantics.shape[1], f"camera {name}")


@pytest.mark.parametrize("S", [0, 3])
@pytest.mark.parametrize("name", ["general", "far"])
def test_exact_parity_mode_is_bit_faithful_to_the_reference_kernels(name, S):
    """The three-way check of tests/test_gpu_parity.py (alpha / depth / semantic bit-identical to the reference's kernels, the
    C oracle's alpha within its exp() ulps) -- bit equality does not care about conditioning, so this is the strongest
    statement there is at Waymo-scale translations."""
    ref = _ref()
    _, _, kw, wts = _case(name, S)
    exact_mode_bit_faithful(ref, oracle, kw, wts, S, label=f" (camera {name}, S={S})")


# ---- 3. visible_filter and markVisible -------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 257, 3000])
@pytest.mark.parametrize("name", ["general", "far"])
def test_visible_filter_and_mark_visible(name, P):
    """The filter kernel has its own copy of the camera: its radii and means2D are bitwise the forward's, and markVisible is
    the oracle's tz > 0.2, for one Gaussian, just past a workgroup, and the whole scene."""
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, full, _, _ = _case(name)
    lo = 0 if P == full.P else int(np.nonzero(_oracle_forward(name).radii > 0)[0][0])  # P = 1: one that is on screen
    sc = syn.Scene(*[t[lo:lo + P].contiguous() for t in (full.means3D, full.scales, full.rotations, full.opacities, full.shs,
                                                         full.semantics)])
    assert sc.P == P
    kw = oracle_kwargs(cam, sc, deg=3, bg=BG)
    fw = oracle.forward(**kw)
    res, internal = raw_forward(kw)
    rast = GaussianRasterizer(settings(cam, bg=BG))
    radii, m2d = rast.visible_filter(dev(sc.means3D), scales=dev(sc.scales), rotations=dev(sc.rotations))
    present = rast.markVisible(dev(sc.means3D))
    torch.cuda.synchronize()
    vis = fw.radii > 0
    assert vis.any() and (P == 1 or not vis.all())
    assert torch.equal(radii, res["radii"]) and (npy(radii) == fw.radii).all()
    fwd_m2d = npy(internal("means2D")).reshape(P, -1)[:, :2]
    assert np.array_equal(npy(m2d).reshape(P, -1)[:, :2][vis].view(np.uint32), fwd_m2d[vis].view(np.uint32))
    assert np.array_equal(fwd_m2d[vis], fw.means2D[vis])
    want = oracle.mark_visible(sc.means3D, cam.viewmatrix, cam.projmatrix)
    assert (npy(present).astype(bool) == want.astype(bool)).all()
    assert want[vis].all() and (fw.depths[vis] > 0.2).all()  # the oracle's depths: everything with a radius is in front
    t = (torch.cat([sc.means3D.double(), torch.ones(P, 1, dtype=torch.float64)], 1) @ cam.viewmatrix.double())[:, 2].numpy()
    clear = np.abs(t - 0.2) > 1e-4 * (1.0 + np.abs(cam.viewmatrix[3, :3].numpy()).max())  # away from the cut: no rounding doubt
    assert (want.astype(bool)[clear] == (t > 0.2)[clear]).all()
    fw.free()


# ---- 4. layers and object alpha --------------------------------------------------------------------------------------------

SPLIT = 1200


@pytest.mark.parametrize("mode", ["default", "exact"])
def test_layers_equal_subset_forwards(mode):
    from test_gpu_layers import _check
    cam, sc, _, _ = _case("general")
    with switches(MODES[mode]):
        got, subs = _check(cam, sc, SPLIT, f"camera general layers/{mode}")
    assert subs[0]["alpha"].max() > 0.5 and subs[1]["alpha"].max() > 0.5


@pytest.mark.parametrize("mode", ["default", "exact"])
def test_object_alpha_equals_the_subset_render_and_its_backward(mode):
    import test_gpu_object_alpha as oa
    cam, sc, _, _ = _case("general")
    w = oa._weight(cam)
    with switches(MODES[mode]):
        want_alpha, want = oa._yardstick(cam, sc, SPLIT, w)
        got, grads = oa._head(cam, sc, SPLIT, w)
    assert want_alpha.max() > 0.5
    assert np.array_equal(got["acc"], want_alpha), "acc_object differs from the subset forward's alpha"
    oa._compare(grads, want, SPLIT, f"camera general/{mode}")


# ---- 5. the drop-in API with the matrices the reference's Camera hands over ------------------------------------------------

def test_drop_in_api_with_the_reference_cameras_tensors():
    """diff_gaussian_rasterization called as the reference's renderer calls it for a K camera (lib/utils/camera_utils.py:50-61,
    lib/utils/graphics_utils.py:72-100): float32 world_view_transform = W2C^T as a TRANSPOSED VIEW (not contiguous),
    full_proj_transform = their float32 product, camera_center from the float32 inverse, tanfov = tan(FoV / 2) with
    FoV = 2 atan(size / 2 f).  Images and gradients are the raw path's on the same values, bit for bit -- the raw path being
    the one the API runs: a forward that stores the colour Jacobian for its backward (tests/test_gpu_color_jacobian.py: the
    row-reading backward rounds dL/dmeans3D differently, by design)."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    _, sc, _, wts = _case("general")
    W, H = cameras.GPU_W, cameras.GPU_H
    K, R, t = cameras.pose("general", W, H)
    W2C = torch.eye(4, dtype=torch.float64)
    W2C[:3, :3], W2C[:3, 3] = R, t
    wvt = W2C.float().transpose(0, 1).cuda()
    proj = syn.projection_matrix_K(K, W, H, 0.001, 1000.0).float().transpose(0, 1).cuda()
    full = wvt.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0)
    center = torch.linalg.inv(W2C.float().transpose(0, 1))[3, :3].cuda()
    fovx, fovy = 2 * math.atan(W / (2 * float(K[0, 0]))), 2 * math.atan(H / (2 * float(K[1, 1])))
    tanfovx, tanfovy = math.tan(fovx * 0.5), math.tan(fovy * 0.5)
    assert not wvt.is_contiguous()
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tanfovx, tanfovy=tanfovy, bg=dev(BG),
                                       scale_modifier=1.0, viewmatrix=wvt, projmatrix=full, sh_degree=3, campos=center,
                                       prefiltered=False, debug=False)
    leaves = {k: dev(getattr(sc, k)).requires_grad_(True) for k in ["means3D", "scales", "rotations", "opacities", "shs", "semantics"]}
    m2d = torch.zeros(sc.P, 3, device="cuda", requires_grad=True)
    color, radii, depth, alpha, sem = GaussianRasterizer(st)(leaves["means3D"], m2d, leaves["opacities"], shs=leaves["shs"],
                                                             scales=leaves["scales"], rotations=leaves["rotations"],
                                                             semantics=leaves["semantics"])
    torch.autograd.backward([color, depth, alpha, sem], [dev(wts[k]) for k in IMAGES])
    cam = syn.Camera(H, W, tanfovx, tanfovy, wvt.cpu().contiguous(), full.cpu().contiguous(), center.cpu().contiguous())
    kw = oracle_kwargs(cam, sc, deg=3, bg=BG)
    with asking_for_jacobian():  # as a forward of the API does when a backward will follow (rasterizer.py: want_jac)
        res, _ = raw_forward(kw)
    g = raw_backward(kw, res, wts)
    torch.cuda.synchronize()
    assert int((radii > 0).sum()) > 500
    assert torch.equal(radii, res["radii"])
    for k, got in zip(IMAGES, (color, depth, alpha, sem)):
        assert torch.equal(got, res[k]), k
    pairs = [("means3D", leaves["means3D"]), ("means2D", m2d), ("opacity", leaves["opacities"]), ("sh", leaves["shs"]),
             ("scales", leaves["scales"]), ("rotations", leaves["rotations"]), ("semantics", leaves["semantics"])]
    for k, leaf in pairs:
        assert float(leaf.grad.abs().max()) > 0, k
        assert torch.equal(leaf.grad.reshape(-1), g[k].reshape(-1)), k
    # ... and the camera is the one synthetic.make_camera_general builds, up to the float32 rounding of the reference's products
    ours = cameras.camera("general", W, H)
    assert torch.equal(wvt.cpu(), ours.viewmatrix)
    assert torch.allclose(full.cpu(), ours.projmatrix, rtol=1e-6, atol=1e-6)


# ---- 6. multiview: per-view camera arrays ----------------------------------------------------------------------------------

def test_factored_sh_gradient_equals_sum_over_general_views():
    """tests/test_gpu_multiview.py::test_factored_sh_gradient_equals_sum_over_views (degree 3) with the views general, zup and
    offcentre in place of yaw steps: three camera centres and three unrelated rotations in the per-view arrays."""
    from test_gpu_multiview import factored_equals_sum_over_views
    cams, sc = cameras.multiview_scene()
    sc.shs[::3, 0, :] -= 2.0  # plenty of clamped channels
    factored_equals_sum_over_views(cams, sc, 3)
