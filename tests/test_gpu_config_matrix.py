"""`-m gpu` tests of the rasterizer over the configuration matrix of the reference's render_kernel
(lib/models/street_gaussian_renderer.py:153-240): colour from SH rows or precomputed, covariance from scales + rotations or
precomputed, and a scale modifier other than 1 -- forward AND backward.

One scene for the whole file: 1061 Gaussians (no multiple of 64 or 256), 160 x 104 (ragged tiles), S = 2, M = 16, every third
Gaussian with a negative DC so that colour channels clamp.  Every test first asserts, on the C oracle, what makes it
meaningful: at least 900 Gaussians of the scene visible, clamped channels, radii that differ from the modifier-1 run on more
than half of the visible Gaussians at its modifier, a non-zero scales gradient.  Every leg runs in the three modes of the
suite: default, EXACT, EXACT | REF_RECT.

The reference forms dL/dscale from s = mod * scale WITHOUT the chain factor mod (backward.cu:295,323-325); dL/drot is right.
The library must reproduce that, and must take the modifier from the forward's geometry buffer.

Which legs are bitwise and which are bounded:
  (a) test_matrix_against_the_oracle, BOUNDED by the project's own gates: 4 input kinds x modifiers 1.0 / 0.6 / 1.5 against
      the C oracle (image_close, grad_close with SAME_STATE_GATE on identical state and the end-to-end gate of
      test_random_scenes_against_oracle; strict mode: strict_mode_against_reference, and against the reference's OWN kernels
      where oracle/_ref is built).  test_both_bindings_* and test_wrapper_*: colors_precomp + scales at 0.6, BITWISE between
      the two bindings and between the autograd wrapper and the raw entry points.
  (b) test_scales_gradient_against_float64, BOUNDED: the HIP gradients against float64 autograd (tests/torch_ref.py) rebuilt
      from the HIP run's own lists; scales.grad / mod is what must match.  Bound: max(4 x yardstick, 16 x 2^-24 x the largest
      reference element), yardstick = the C oracle's own deviation from the same float64 result.  The undivided comparison
      must FAIL that bound.  Ratios are printed and logged (gpu_utils._log, kind "config_matrix_f64").
  (c) test_fold_identity, BITWISE: scale_modifier = m with scales == scale_modifier = 1 with (scales * m).float(), for
      m = 0.5, 2.0, 0.6, 1.5: R, radii, the four images, point_list, ranges, all nine raw gradients (dL/dscale included: a
      backward with the chain factor cannot pass), visible_filter, forward_layers, forward_with_object_alpha and its backward.
  (d) test_cov3D_precomp_ignores_the_modifier, BITWISE: both kinds with cov3D_precomp at 0.6 == at 1.0.
  (e) test_mixed_kinds_equal_the_pure_ones, BITWISE: shs + cov3D_precomp = the scales run's cov3D, and colors_precomp = the
      SH run's rgb + scales, against the pure runs.
  (f) test_backward_ignores_its_modifier_argument, BITWISE: a backward handed 1.5 after a forward at 0.6 (include/sgr.h,
      include/sgr_object_alpha.h)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import torch_ref as tr
from gpu_utils import (GRAD_NAMES, SAME_STATE_GATE, _log, dev, grad_close, image_close, npy, oracle_backward_same_state,
                       raw_backward, raw_forward, restrict_oracle, settings, strict_mode_against_reference, switches)
from helpers import oracle_kwargs
from oracle import oracle
from street_gaussians_amd import _C
from street_gaussians_amd import synthetic as syn

pytestmark = pytest.mark.gpu

P, W, H, S = 1061, 160, 104, 2
BG = torch.tensor([0.3, 0.1, 0.7])
MODES = {"default": 0, "exact": _C.EXACT, "strict": _C.EXACT | _C.REF_RECT}
KINDS = [("sh", "scales"), ("precomp", "scales"), ("sh", "cov"), ("precomp", "cov")]
mode_param = pytest.mark.parametrize("mode", list(MODES))


# ---- the scene and its references: built once, shared, never written to ------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scene():
    cam = syn.make_camera(W, H, fx=170.0, yaw_deg=3.0)
    sc = syn.make_scene(P, cam, S=S, seed=7, scale_px=0.02, zmin=1.0, zmax=12.0, margin=1.3)
    sc.shs[::3, 0, :] -= 1.5
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(5))
    return cam, sc, syn.loss_weights(cam, S=S), colors


def _cov6(mod):
    """cov3D_precomp as the reference's get_covariance(scaling_modifier) builds it: the modifier inside the matrix."""
    _, sc, _, _ = _scene()
    Sig = tr.cov3d_from_scale_rot(sc.scales.double(), sc.rotations.double(), mod)
    return torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], -1).float()


def _kw(kind, mod, **over):
    """Oracle-style keyword dict of one configuration; `over` replaces entries (scales=..., cov3D_precomp=..., ...)."""
    cam, sc, _, colors = _scene()
    kw = oracle_kwargs(cam, sc, bg=BG, use_sh=kind[0] == "sh", colors=colors, use_cov_precomp=kind[1] == "cov",
                       cov3D=_cov6(mod) if kind[1] == "cov" else None, scale_modifier=mod)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def _oracle(kind, mod):
    """-> (the C oracle's forward state, its gradients) for one configuration."""
    _, _, wts, _ = _scene()
    fw = oracle.forward(**_kw(kind, mod))
    return fw, oracle.backward(fw, wts["color"], wts["depth"], wts["alpha"], wts["semantic"])


def _meaningful(kind, mod):
    """What makes a case worth running, asserted on the oracle."""
    fw1, _ = _oracle(kind, 1.0)
    fw, g = _oracle(kind, mod)
    assert (fw1.radii > 0).sum() >= 900 and (fw.radii > 0).sum() >= 800
    if kind[0] == "sh":
        assert fw.clamped.sum() > 0
    if mod != 1.0:
        vis = (fw1.radii > 0) | (fw.radii > 0)
        assert (fw.radii != fw1.radii)[vis].mean() > 0.5, "the modifier hardly changes the radii"
    if kind[1] == "scales":
        assert np.abs(g["scales"]).max() > 0 and np.abs(g["rotations"]).max() > 0
    else:
        assert np.abs(g["cov3D"]).max() > 0


def _run(kw, mode, wts=None):
    """Raw forward + backward in one mode -> (res, internal, gradients)."""
    wts = _scene()[2] if wts is None else wts
    with switches(MODES[mode]):
        res, internal = raw_forward(kw)
        g = raw_backward(kw, res, wts)
        torch.cuda.synchronize()
    return res, internal, g


def _lists(internal, mode):
    with switches(MODES[mode]):
        return npy(internal("point_list")).copy(), npy(internal("ranges")).copy()


def _same_forward(a, b, label, mode):
    """Two raw runs: R, radii, the four images and the exported lists bit for bit."""
    (ra, ia), (rb, ib) = a, b
    assert ra["R"] == rb["R"] > 0, label
    for k in ("radii", "color", "depth", "alpha", "semantic"):
        assert torch.equal(ra[k], rb[k]), f"{label}: {k}"
    for x, y in zip(_lists(ia, mode), _lists(ib, mode)):
        assert np.array_equal(x, y), f"{label}: lists"


def _keys(kind):
    return (["means2D", "colors", "opacity", "means3D", "cov3D", "semantics"] + (["sh"] if kind[0] == "sh" else []) +
            (["scales", "rotations"] if kind[1] == "scales" else []))


# ---- (a) against the oracle ----------------------------------------------------------------------------------------------

@mode_param
@pytest.mark.parametrize("mod", [1.0, 0.6, 1.5])
@pytest.mark.parametrize("kind", KINDS, ids=["-".join(k) for k in KINDS])
def test_matrix_against_the_oracle(kind, mod, mode):
    _meaningful(kind, mod)
    cam, sc, wts, _ = _scene()
    kw = _kw(kind, mod)
    fw, ref = _oracle(kind, mod)
    label = f"matrix {'-'.join(kind)} x{mod}"
    if mode == "strict":
        _, g, _ = strict_mode_against_reference(kw, wts, S, label, rf=fw)
        from oracle import ref as ref_kernels
        if ref_kernels.available():  # the reference's own kernels: the authority on the quirk
            strict_mode_against_reference(kw, wts, S, label)
    else:
        res, internal, g = _run(kw, mode)
        with switches(MODES[mode]):
            b = restrict_oracle(internal, fw, kw)
            assert res["R"] == b.num_rendered > 0
            assert (npy(res["radii"]) == fw.radii).all()
            assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
            assert (npy(internal("keys")).view(np.uint64) == b.keys).all()
            assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
        for k in ("color", "depth", "alpha", "semantic"):
            image_close(npy(res[k]), getattr(fw, k), name=f"{label}/{mode}: {k}")
        # identical state: the backward alone; end to end: the gate test_random_scenes_against_oracle holds scenes of this
        # regime to (its scale modifiers 0.7 / 1.3, splats up to scale_px 0.02)
        same = oracle_backward_same_state(oracle, fw, res, wts, S)
        for k in _keys(kind):
            grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"same-state {label}/{mode}:{k}", **SAME_STATE_GATE)
            grad_close(npy(g[k]).reshape(ref[k].shape), ref[k], rel=2e-4, abs_frac=3e-4, name=f"{label}/{mode}:{k}")
    if kind[1] == "cov":
        assert float(g["scales"].abs().max()) == 0.0 and float(g["rotations"].abs().max()) == 0.0


@contextlib.contextmanager
def _binding(name):
    prev = _C.binding()
    _C.set_binding(name)
    try:
        yield
    finally:
        _C.set_binding(prev)


@pytest.fixture(params=["ctypes", "pybind"])
def binding(request):
    with _binding(request.param):
        yield request.param


@mode_param
def test_both_bindings_give_the_same_bits(binding, mode):
    """colors_precomp + scales at 0.6 (what override_color / convert_SHs_python alone produce) through the binding of the
    fixture and through ctypes: every output and every gradient bit for bit."""
    kind, mod = ("precomp", "scales"), 0.6
    _meaningful(kind, mod)
    kw = _kw(kind, mod)
    res, internal, g = _run(kw, mode)
    with _binding("ctypes"):
        res_c, internal_c, g_c = _run(kw, mode)
    _same_forward((res, internal), (res_c, internal_c), binding, mode)
    for k in GRAD_NAMES:
        assert torch.equal(g[k], g_c[k]), (binding, k)
    assert float(g["scales"].abs().max()) > 0


@mode_param
def test_wrapper_with_colors_precomp_and_scales(binding, mode):
    """The same configuration through the GaussianRasterizer autograd wrapper: the gradients of the inputs that are there
    arrive and equal the raw entry point's; nothing is returned for shs and cov3D_precomp, which are absent."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from street_gaussians_amd import rasterizer as rz
    kind, mod = ("precomp", "scales"), 0.6
    _meaningful(kind, mod)
    cam, sc, wts, colors = _scene()
    t = {k: dev(getattr(sc, k)).requires_grad_(True) for k in ["means3D", "scales", "rotations", "opacities", "semantics"]}
    t["colors_precomp"] = dev(colors).requires_grad_(True)
    m2d = torch.zeros(P, 3, device="cuda", requires_grad=True)
    seen = {}
    orig = rz._RasterizeGaussians.backward

    def spy(ctx, *grads):
        seen["returned"] = orig(ctx, *grads)
        return seen["returned"]
    rz._RasterizeGaussians.backward = staticmethod(spy)
    try:
        with switches(MODES[mode]):
            color, radii, depth, alpha, sem = GaussianRasterizer(settings(cam, bg=BG, scale_modifier=mod))(
                t["means3D"], m2d, t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                rotations=t["rotations"], semantics=t["semantics"])
            ((color * dev(wts["color"])).sum() + (depth * dev(wts["depth"])).sum() + (alpha * dev(wts["alpha"])).sum() +
             (sem * dev(wts["semantic"])).sum()).backward()
            torch.cuda.synchronize()
    finally:
        rz._RasterizeGaussians.backward = staticmethod(orig)
    res, _, g = _run(_kw(kind, mod), mode)
    for k, o in (("color", color), ("radii", radii), ("depth", depth), ("alpha", alpha), ("semantic", sem)):
        assert torch.equal(o.detach(), res[k]), k
    pairs = [("means3D", t["means3D"]), ("colors", t["colors_precomp"]), ("scales", t["scales"]), ("rotations", t["rotations"]),
             ("opacity", t["opacities"]), ("semantics", t["semantics"]), ("means2D", m2d)]
    for k, leaf in pairs:
        assert leaf.grad is not None and float(leaf.grad.abs().max()) > 0, k
        assert torch.equal(leaf.grad, g[k].reshape(leaf.shape)), k
    # (means3D, means2D, sh, colors_precomp, semantics, opacities, scales, rotations, cov3D_precomp, settings, ...)
    returned = seen["returned"]
    assert returned[2] is None and returned[8] is None and all(r is None for r in returned[9:])
    assert all(returned[i] is not None for i in (0, 1, 3, 4, 5, 6, 7))


# ---- (b) the quirk against float64 directly -------------------------------------------------------------------------------

_F64 = {}


def _float64_gradients(mod, point_list, ranges):
    """The SH + scales render rebuilt in float64 from the given lists and differentiated by autograd (cached per list)."""
    key = (mod, point_list.tobytes(), ranges.tobytes())
    if key not in _F64:
        cam, sc, wts, _ = _scene()
        d = lambda t: t.double().clone().requires_grad_(True)
        m3, s, q, o, sh, sem = map(d, (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs, sc.semantics))
        pre = tr.preprocess(m3, cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx, cam.tanfovy, W, H, 3, o, shs=sh,
                            scales=s, rotations=q, scale_modifier=mod)
        pre["pix"].retain_grad()
        pl = torch.from_numpy(point_list.view(np.uint32).astype(np.int64))
        col, dep, alp, se, _ = tr.render_batched(pre, pl, ranges.view(np.uint32).reshape(-1, 2), W, H, BG, sem)
        ((col * wts["color"]).sum() + (dep * wts["depth"]).sum() + (alp * wts["alpha"]).sum() +
         (se * wts["semantic"]).sum()).backward()
        pg = pre["pix"].grad
        _F64[key] = dict(means3D=m3.grad.numpy(), opacity=o.grad.numpy(), sh=sh.grad.numpy(), rotations=q.grad.numpy(),
                         semantics=sem.grad.numpy(), scales_autograd=s.grad.numpy(), scales=(s.grad / mod).numpy(),
                         means2D=torch.stack([pg[:, 0] * 0.5 * W, pg[:, 1] * 0.5 * H], -1).numpy())
    return _F64[key]


@mode_param
@pytest.mark.parametrize("mod", [0.6, 1.5])
def test_scales_gradient_against_float64(mod, mode):
    kind = ("sh", "scales")
    _meaningful(kind, mod)
    _, go = _oracle(kind, mod)
    res, internal, g = _run(_kw(kind, mod), mode)
    f64 = _float64_gradients(mod, *_lists(internal, mode))
    floor = 16 * 2.0 ** -24
    bound = {}
    for k in ("means3D", "opacity", "sh", "scales", "rotations", "semantics", "means2D"):
        want = f64[k]
        take = (lambda a: np.asarray(a, np.float64).reshape(P, -1)[:, :2]) if k == "means2D" else \
            (lambda a: np.asarray(a, np.float64).reshape(want.shape))
        yard = np.abs(take(go[k]) - want).max()
        bound[k] = max(4 * yard, floor * np.abs(want).max())
        err = np.abs(take(npy(g[k])) - want).max()
        ratio = err / bound[k]
        print(f"config matrix f64 x{mod}/{mode}: {k}: err {err:.3e} yardstick {yard:.3e} bound {bound[k]:.3e} ratio {ratio:.3f}")
        _log(dict(kind="config_matrix_f64", name=f"x{mod}/{mode}:{k}", err=float(err), yardstick=float(yard),
                  bound=float(bound[k]), ratio=float(ratio)))
        assert ratio <= 1.0, f"{k}: {err} vs bound {bound[k]} (x{mod}, {mode})"
    # the quirk itself: against the TRUE gradient (autograd, undivided) the same bound must fail
    undivided = np.abs(npy(g["scales"]).astype(np.float64) - f64["scales_autograd"]).max()
    print(f"config matrix f64 x{mod}/{mode}: scales undivided: err {undivided:.3e} ratio {undivided / bound['scales']:.3e}")
    assert undivided > bound["scales"]


# ---- (c) fold identity ------------------------------------------------------------------------------------------------------

def _wrapper_args(kw, grad=False):
    """Keyword arguments of GaussianRasterizer.forward* from an oracle-style dict."""
    names = dict(means3D="means3D", opacities="opacities", shs="shs", colors_precomp="colors_precomp", scales="scales",
                 rotations="rotations", cov3D_precomp="cov3D_precomp", semantics="semantics")
    a = {n: (dev(kw[k]).requires_grad_(True) if grad else dev(kw[k])) for n, k in names.items() if kw.get(k) is not None}
    a["means2D"] = torch.zeros(P, 3, device="cuda", requires_grad=grad)
    return a


def _entry_points(kw, mode):
    """visible_filter, forward_layers and forward_with_object_alpha (+ its backward) of one configuration -> dict of tensors."""
    from diff_gaussian_rasterization import GaussianRasterizer
    cam = _scene()[0]
    split = 400
    out = {}
    with switches(MODES[mode]):
        rast = GaussianRasterizer(settings(cam, bg=BG, scale_modifier=kw["scale_modifier"]))
        a = _wrapper_args(kw)
        geo = {k: a[k] for k in ("scales", "rotations", "cov3D_precomp") if k in a}
        out["filter_radii"], out["filter_means2D"] = rast.visible_filter(a["means3D"], **geo)
        with torch.no_grad():
            lay = rast.forward_layers(**a, split=split, layer_background=dev(torch.tensor([0.2, 0.5, 0.9])))[5]
        for n, t in zip(lay._fields, lay):
            out["layers_" + n] = t
        a = _wrapper_args(kw, grad=True)
        acc = rast.forward_with_object_alpha(**a, split=split)[5]
        w = dev(torch.rand(1, H, W, generator=torch.Generator().manual_seed(11)) * 2.0 - 1.0)
        (acc * w).sum().backward()
        torch.cuda.synchronize()
        out["acc_object"] = acc.detach()
        for k in ("means3D", "opacities", "scales", "rotations", "cov3D_precomp"):
            if k in a:
                out["object_grad_" + k] = a[k].grad
    return out


@mode_param
@pytest.mark.parametrize("mod", [0.5, 2.0, 0.6, 1.5])
def test_fold_identity(mod, mode):
    """mod * scale is the first thing sgr_cov3d and sgr_cov3d_backward form (FP contraction cannot touch a product of
    products), so the modifier folds into the scales exactly -- and, because dL/dscale lacks the chain factor, so does the
    scales gradient.  No tolerance anywhere."""
    kind = ("sh", "scales")
    _meaningful(kind, mod)
    sc = _scene()[1]
    kw_m = _kw(kind, mod)
    kw_f = _kw(kind, 1.0, scales=(sc.scales * mod).float())
    res_m, int_m, g_m = _run(kw_m, mode)
    res_f, int_f, g_f = _run(kw_f, mode)
    _same_forward((res_m, int_m), (res_f, int_f), f"fold x{mod}", mode)
    assert float(g_m["scales"].abs().max()) > 0
    for k in GRAD_NAMES:
        assert torch.equal(g_m[k], g_f[k]), f"fold x{mod}/{mode}: dL/d{k}"
    em, ef = _entry_points(kw_m, mode), _entry_points(kw_f, mode)
    assert float(em["acc_object"].max()) > 0.5 and float(em["object_grad_scales"].abs().max()) > 0
    assert set(em) == set(ef) and len(em) == 11
    for k in em:
        assert torch.equal(em[k], ef[k]), f"fold x{mod}/{mode}: {k}"


# ---- (d) cov3D_precomp ignores the modifier -------------------------------------------------------------------------------

@mode_param
@pytest.mark.parametrize("kind", [("sh", "cov"), ("precomp", "cov")], ids=["sh-cov", "precomp-cov"])
def test_cov3D_precomp_ignores_the_modifier(kind, mode):
    from diff_gaussian_rasterization import GaussianRasterizer
    _meaningful(kind, 1.0)
    cam = _scene()[0]
    cov = _cov6(1.0)
    kw_1, kw_m = _kw(kind, 1.0, cov3D_precomp=cov), _kw(kind, 0.6, cov3D_precomp=cov)
    res_1, int_1, g_1 = _run(kw_1, mode)
    res_m, int_m, g_m = _run(kw_m, mode)
    _same_forward((res_1, int_1), (res_m, int_m), "cov3D_precomp x0.6", mode)
    assert float(g_1["cov3D"].abs().max()) > 0
    for k in GRAD_NAMES:
        assert torch.equal(g_1[k], g_m[k]), k
    with switches(MODES[mode]):
        f1 = GaussianRasterizer(settings(cam, bg=BG, scale_modifier=1.0)).visible_filter(dev(kw_1["means3D"]), cov3D_precomp=dev(cov))
        fm = GaussianRasterizer(settings(cam, bg=BG, scale_modifier=0.6)).visible_filter(dev(kw_1["means3D"]), cov3D_precomp=dev(cov))
        torch.cuda.synchronize()
    assert torch.equal(f1[0], res_1["radii"]) and torch.equal(f1[0], fm[0]) and torch.equal(f1[1], fm[1])


# ---- (e) mixed kinds against the pure ones ---------------------------------------------------------------------------------

@mode_param
def test_mixed_kinds_equal_the_pure_ones(mode):
    mod = 0.6
    _meaningful(("sh", "scales"), mod)
    kw = _kw(("sh", "scales"), mod)
    res, internal, g = _run(kw, mode)
    with switches(MODES[mode]):
        cov, rgb = internal("cov3D").clone(), internal("rgb").clone()
        rgb[res["radii"] == 0] = 0.0  # (the preprocess writes no colour for a Gaussian it culls)
        torch.cuda.synchronize()
    assert float(g["cov3D"].abs().max()) > 0 and bool((rgb[res["radii"] > 0] == 0).any())  # clamped channels went into the colours
    # shs + cov3D_precomp = the cov3D the scales run computed
    kw_c = _kw(("sh", "cov"), mod, cov3D_precomp=cov.cpu())
    res_c, int_c, g_c = _run(kw_c, mode)
    _same_forward((res, internal), (res_c, int_c), "sh + cov3D_precomp", mode)
    for k in ("means2D", "opacity", "sh", "semantics", "means3D", "cov3D", "colors"):
        assert torch.equal(g[k], g_c[k]), f"sh + cov3D_precomp: dL/d{k}"
    assert float(g_c["scales"].abs().max()) == 0.0 and float(g_c["rotations"].abs().max()) == 0.0
    # colors_precomp = the rgb the SH run computed, + scales
    kw_p = _kw(("precomp", "scales"), mod, colors_precomp=rgb.cpu())
    res_p, int_p, g_p = _run(kw_p, mode)
    _same_forward((res, internal), (res_p, int_p), "colors_precomp + scales", mode)
    for k in ("means2D", "opacity", "scales", "rotations", "semantics", "cov3D"):
        assert torch.equal(g[k], g_p[k]), f"colors_precomp + scales: dL/d{k}"
    # the raw `colors` output of the SH run is the UNMASKED dL/dcolour (the clamp mask is applied on the way to dL/dSH)
    assert torch.equal(g["colors"], g_p["colors"])
    # no view-direction path without SH rows: dL/dmeans3D differs (held to the oracle by test_matrix_against_the_oracle)
    assert not torch.equal(g["means3D"], g_p["means3D"])


# ---- (f) the backward's modifier argument -----------------------------------------------------------------------------------

@mode_param
def test_backward_ignores_its_modifier_argument(mode):
    """sgr_backward and sgr_layer_alpha_backward differentiate the forward they follow: the modifier comes from the geometry
    buffer, whatever the argument says."""
    kind, mod, split = ("sh", "scales"), 0.6, 400
    _meaningful(kind, mod)
    wts = _scene()[2]
    kw = _kw(kind, mod)
    other = dict(kw, scale_modifier=1.5)
    with switches(MODES[mode]):
        res, _ = raw_forward(kw)
        g = raw_backward(kw, res, wts)
        g_other = raw_backward(other, res, wts)
        a, last = _C.layer_alpha_forward(P, res["R"], H, W, split, res["geom"], res["binning"], res["img"])
        w = dev(torch.rand(1, H, W, generator=torch.Generator().manual_seed(11)) * 2.0 - 1.0)
        lay = [_C.layer_alpha_backward(res["R"], H, W, split, dev(kw["means3D"]), dev(kw["scales"]), dev(kw["rotations"]), m, None,
                                       res["radii"], res["geom"], res["binning"], res["img"], a, last, w, False) for m in (mod, 1.5)]
        torch.cuda.synchronize()
    assert float(g["scales"].abs().max()) > 0
    for k in GRAD_NAMES:
        assert torch.equal(g[k], g_other[k]), k
    assert float(lay[0][2].abs().max()) > 0
    for x, y in zip(lay[0][:4], lay[1][:4]):
        assert torch.equal(x, y)
    # ... and the modifier matters: the same backward after a forward at 1.5 gives other numbers
    with switches(MODES[mode]):
        res15, _ = raw_forward(other)
        g15 = raw_backward(other, res15, wts)
        torch.cuda.synchronize()
    assert not torch.equal(g15["scales"], g["scales"])
