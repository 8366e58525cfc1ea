"""`-m gpu` parity tests: the HIP path (through the C ABI / drop-in Python API) against
  (1) the C oracle (oracle/sgr_oracle.c) on the same seeded inputs,
  (2) the reference's own kernels compiled for gfx950 (oracle/_ref, when the .so travelled),
  (3) committed golden fixtures (tests/golden/*.npz, generated from (2) on the MI355X box),
plus size-independent properties at BASELINE.json's full sizes.

Gates: integer outputs (radii, tiles_touched, point_offsets, num_rendered, sorted keys,
point_list, ranges) bit-exact; float images and gradients within 1e-4 relative (with a small floor), apart
from a bounded handful of alpha-threshold flips (see gpu_utils.image_close).

Strict legs.  The configuration bench.py reports, EXACT | REF_RECT (SGR_EXACT=1 SGR_REF_RECT=1: parity arithmetic on the
reference's own tile rects, out-of-rect instances marked dead, the compact hit list and the backward that walks it), goes
through gpu_utils.strict_mode_against_reference, which compares the library's lists with the reference's ENTRY FOR ENTRY --
nothing is filtered through rects or masks the library exports: test_strict_mode_matches_oracle (every case, C oracle),
test_strict_mode_cases_against_reference_kernels (every case, oracle/_ref), mode "strict" of test_edge_sizes /
test_random_scenes_against_oracle / test_golden_fixture / test_tight_rects_are_invisible_random_sweep,
test_every_channel_width_strict, test_widest_instantiations_agree_with_the_narrower_ones_strict,
test_precomputed_colors_and_cov3D_strict, test_far_depths_fall_back_to_the_32_bit_depth_sort_strict,
test_degenerate_inputs_strict, and test_strict_environment_names_in_a_fresh_process (the two environment names in a child
process against the switch mask in this one, bit for bit)."""
import glob
import os

import numpy as np
import pytest
import torch

from gpu_utils import (SAME_STATE_GATE, conditioned_allowance, dev, exact_mode_against_reference_kernels,
                       exact_mode_bit_faithful, grad_close,
                       image_close, npy, oracle_backward_same_state, raw_backward, raw_forward, restrict_binning, restrict_oracle,
                       settings, strict_gate, strict_mode_against_reference, switches)
from street_gaussians_amd import _C
from helpers import oracle_kwargs, small_case
from oracle import oracle
from street_gaussians_amd import synthetic as syn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _cases():
    out = {}
    cam, sc = small_case(P=80, S=2)
    out["tiny_sh3_sem2"] = (cam, sc, dict(bg=torch.tensor([0.3, 0.1, 0.7])))
    cam, sc = small_case(P=300, S=0, scale_px=0.03, zmax=6.0)
    sc.opacities.fill_(0.95)
    out["dense_saturating"] = (cam, sc, dict())
    cam = syn.make_camera(480, 320, fx=512.5, yaw_deg=2.0)
    out["mid_20k_sem3"] = (cam, syn.make_scene(20000, cam, S=3, seed=3), dict(bg=torch.tensor([1.0, 1.0, 1.0])))
    cam = syn.make_camera(333, 211, fx=300.0)
    sc = syn.make_scene(30000, cam, S=0, seed=4, margin=1.6, scale_px=0.004)
    sc.shs[::2, 0, :] -= 2.0
    out["ragged_clamped_offscreen"] = (cam, sc, dict(deg=2))
    cam = syn.make_camera(256, 256, fx=280.0)
    out["sem19_deg1"] = (cam, syn.make_scene(5000, cam, S=19, seed=5, scale_px=0.005), dict(deg=1))
    cam = syn.make_camera(640, 400, fx=700.0)
    sc = syn.make_scene(4000, cam, S=0, seed=6, scale_px=0.05, zmin=0.3, zmax=10.0)  # huge splats, fat tiles
    out["huge_splats"] = (cam, sc, dict())
    # giant, nearly degenerate splats (sigma of ~1e3 px along one axis, sub-pixel along the others): the conic's
    # determinant cancels in fp32, which is where a cull box derived from the covariance could disagree with the
    # conic the blend kernels evaluate
    cam = syn.make_camera(400, 240, fx=420.0)
    sc = syn.make_scene(600, cam, S=0, seed=8, scale_px=0.004, zmin=0.5, zmax=6.0)
    sc.scales[::2] = sc.scales[::2] * torch.tensor([900.0, 0.02, 0.02])
    sc.scales[1::4] = sc.scales[1::4] * torch.tensor([0.05, 400.0, 0.05])
    out["giant_degenerate"] = (cam, sc, dict())
    # SH rows narrower than 16 coefficients (max_sh_degree 0 / 1 / 2 models: M = 1, 4, 9): 3-, 12- and 27-float rows take the
    # scalar / float4 / scalar row paths of the preprocess and of the per-Gaussian backward instead of the LDS-staged one
    cam = syn.make_camera(320, 200, fx=330.0, yaw_deg=-3.0)
    out["sh_rows_M1"] = (cam, syn.make_scene(3000, cam, sh_degree_max=0, S=0, seed=11, scale_px=0.006), dict(deg=0))
    out["sh_rows_M4"] = (cam, syn.make_scene(3000, cam, sh_degree_max=1, S=2, seed=12, scale_px=0.006), dict(deg=1))
    out["sh_rows_M9"] = (cam, syn.make_scene(3000, cam, sh_degree_max=2, S=0, seed=13, scale_px=0.006), dict(deg=2))
    out["sh_rows_M9_deg1"] = (cam, syn.make_scene(3000, cam, sh_degree_max=2, S=0, seed=14, scale_px=0.006), dict(deg=1))
    return out


# Not compared with the oracle: at sigma ~1e3 px the quadratic form -0.5*(A dx^2 + C dy^2) - B dx dy cancels by 4-6
# digits, so two correct evaluation orders (the reference's, the pre-scaled FMA form of the kernels) differ by more
# than the parity gate.  What must hold, and is tested, is that the CULL never changes a bit on such splats.
ILL_CONDITIONED = {"giant_degenerate"}


CASES = _cases()

# (rel, abs_frac) for the two deliberately saturating cases.  The reference algorithm takes T_final = 1 - sum(w)
# (backward.cu:468) and recovers every T_i by repeated division by (1-alpha) (backward.cu:547): for pixels whose
# final transmittance is ~1e-4 the fp32 cancellation in 1 - sum(w) alone is a ~6e-4 RELATIVE error that multiplies
# every gradient term of that pixel.  Measured on MI355X, the reference's own kernels and their line-by-line C
# restatement differ by up to 2.2e-4 of the tensor scale on `huge_splats` (255 blended layers per pixel).
SATURATING_TOL = {"dense_saturating": (2e-3, 2e-4), "huge_splats": (1e-4, 1e-3)}

GRAD_KEYS = ["means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "semantics"]
# SAME_STATE_GATE (gpu_utils): the backward on identical inputs, gpu_utils.oracle_backward_same_state


def _kw(name):
    cam, sc, opt = CASES[name]
    return cam, sc, oracle_kwargs(cam, sc, deg=opt.get("deg", 3), bg=opt.get("bg"))


@pytest.mark.parametrize("name", [n for n in CASES if n not in ILL_CONDITIONED])
def test_forward_matches_oracle(name):
    cam, sc, kw = _kw(name)
    fw = oracle.forward(**kw)
    res, internal = raw_forward(kw)
    P, H, W = sc.P, cam.image_height, cam.image_width
    # ---- integer / index outputs: bit exact (the binning arrays = the oracle's restricted to the emitted tile rects)
    b = restrict_oracle(internal, fw, kw)
    assert res["R"] == b.num_rendered
    assert (npy(res["radii"]) == fw.radii).all()
    assert (npy(internal("tiles_touched")).view(np.uint32) == b.tiles_touched).all()
    assert (npy(internal("point_offsets")).view(np.uint32) == b.point_offsets).all()
    assert (npy(internal("keys")).view(np.uint64) == b.keys).all()
    assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
    assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
    with switches(_C.test_switches(-1) | _C.REF_RECT):  # with the reference's rects: the oracle's arrays entry for entry
        res_r, int_r = raw_forward(kw)
        assert res_r["R"] == fw.num_rendered and int(int_r("num_rendered_reference")[0]) == fw.num_rendered
        assert (npy(int_r("tiles_touched")).view(np.uint32) == fw.tiles_touched).all()
        assert (npy(int_r("point_offsets")).view(np.uint32) == fw.point_offsets).all()
        assert (npy(int_r("keys")).view(np.uint64) == fw.keys).all()
        assert (npy(int_r("point_list")).view(np.uint32) == fw.point_list).all()
        assert (npy(int_r("ranges")).view(np.uint32) == fw.ranges).all()
        for k in ["color", "depth", "alpha", "semantic"]:  # the instances the tight rects leave out change no pixel
            assert torch.equal(res[k], res_r[k]), f"tile rects changed {k}"
    assert int(internal("num_rendered_reference")[0]) == fw.num_rendered
    vis = fw.radii > 0
    # ---- preprocess floats (contraction off on both sides -> exact)
    assert (npy(internal("depths"))[vis] == fw.depths[vis]).all()
    assert (npy(internal("means2D"))[vis] == fw.means2D[vis]).all()
    assert (npy(internal("conic_opacity"))[vis] == fw.conic_opacity[vis]).all()
    assert (npy(internal("clamped"))[vis] == fw.clamped[vis]).all()
    assert np.abs(npy(internal("rgb"))[vis] - fw.rgb[vis]).max() <= 2e-6
    # ---- images
    flips = image_close(npy(res["color"]), fw.color, name="color")
    image_close(npy(res["depth"]), fw.depth, name="depth")
    image_close(npy(res["alpha"]), fw.alpha, name="alpha")
    image_close(npy(res["semantic"]), fw.semantic, name="semantic")
    nc = npy(internal("n_contrib")).view(np.uint32).reshape(H, W)
    assert (nc != b.n_contrib).mean() <= 1e-3, "n_contrib differs beyond exp-ulp flips"
    fw.free()


@pytest.mark.parametrize("name", [n for n in CASES if n not in ILL_CONDITIONED])
def test_backward_matches_oracle(name):
    cam, sc, kw = _kw(name)
    S = sc.semantics.shape[1]
    wts = syn.loss_weights(cam, S=S)
    fw = oracle.forward(**kw)
    ref = oracle.backward(fw, wts["color"], wts["depth"], wts["alpha"], wts["semantic"])
    res, _ = raw_forward(kw)
    g = raw_backward(kw, res, wts)
    # (1) identical inputs: the oracle's backward on the forward state the HIP backward got -> the north-star gate
    same = oracle_backward_same_state(oracle, fw, res, wts, S)
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"same-state {name}:{k}", **SAME_STATE_GATE)
    # (2) end to end, each side on its own forward.  dense_saturating / huge_splats: T_final = 1 - sum(w) cancels and T
    # is recovered by repeated division by (1-alpha) in fp32 (backward.cu:468,547), which amplifies last-ulp
    # differences of the two forwards (see SATURATING_TOL)
    tol, af = SATURATING_TOL.get(name, (1e-4, 2e-6))
    mags = _color_mag(fw, wts) if name == "huge_splats" else {}
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(ref[k].shape), ref[k], rel=tol, abs_frac=af, name=f"{name}:{k}", mag=mags.get(k))
    fw.free()


@pytest.mark.parametrize("name", [n for n in CASES if n not in ILL_CONDITIONED])
def test_strict_mode_matches_oracle(name):
    """The strict leg of test_forward_matches_oracle / test_backward_matches_oracle: every case under EXACT | REF_RECT
    against the C oracle -- the lists entry for entry, images / n_contrib / gradients within the bounds of those two tests
    (gpu_utils.strict_mode_against_reference).  Needs nothing but the C oracle: it runs wherever the suite runs."""
    cam, sc, kw = _kw(name)
    S = sc.semantics.shape[1]
    fw = oracle.forward(**kw)
    strict_mode_against_reference(kw, syn.loss_weights(cam, S=S), S, name, rf=fw)
    fw.free()


@pytest.mark.parametrize("name", [n for n in CASES if n not in ILL_CONDITIONED and CASES[n][1].semantics.shape[1] == 0])
def test_scalar_walk_backward_matches_oracle(name):
    if not _C.has_variants():
        pytest.skip("the scalar-walk backward is an A/B design outside the shipped library (tools/build_variant.py -DSGR_WITH_VARIANTS=1)")
    """The second blend-backward design (csrc/sgr_blend_bwd_sw.hip, switch USE_SW / SGR_SW=1: a wave owns its quadrant, records
    through the scalar cache, four rows per instance) is held to the same gates as the shipped kernel, in both modes."""
    cam, sc, kw = _kw(name)
    wts = syn.loss_weights(cam, S=0)
    fw = oracle.forward(**kw)
    res, _ = raw_forward(kw)
    with switches(_C.USE_SW):
        g = raw_backward(kw, res, wts)
    same = oracle_backward_same_state(oracle, fw, res, wts, 0)
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"scalar walk same-state {name}:{k}", **SAME_STATE_GATE)
    fw.free()
    from oracle import ref
    if ref.available():
        with switches(_C.USE_SW):
            exact_mode_against_reference_kernels(kw, wts, 0, f"scalar walk {name}", allow=EXACT_ALLOW.get(name))


def _color_mag(fw, wts):
    """sum_pix w*|dL/dC| per Gaussian = the sum of |terms| behind dL/drgb (and, through Y_k(dir), dL/dSH): the
    oracle's backward run with absolute-valued colour weights and nothing else."""
    z = {k: torch.zeros_like(v) for k, v in wts.items()}
    gabs = oracle.backward(fw, wts["color"].abs(), z["depth"], z["alpha"], z["semantic"])
    return {"colors": gabs["colors"], "sh": np.abs(gabs["sh"]) + gabs["colors"][:, None, :] * 0.3}


# documented exceptions of the strict gate in parity mode (elements outside rel 1e-4 + 2e-6 of the scale), per case
EXACT_ALLOW = {}


@pytest.mark.parametrize("name", [n for n in CASES if n not in ILL_CONDITIONED])
def test_exact_mode_cases_against_reference_kernels(name):
    """Every case of this file in the parity mode (sgr_test_switches bit 7) against the reference's own kernels, end to
    end, each side on its own forward: integer outputs identical, alpha / depth / semantic / n_contrib bit-identical, colour
    within rel 1e-4 without an outlier, all gradients inside rel 1e-4 + 2e-6 of the scale without an element outside."""
    _ref()
    cam, sc, kw = _kw(name)
    S = sc.semantics.shape[1]
    wts = syn.loss_weights(cam, S=S)
    res, g = exact_mode_against_reference_kernels(kw, wts, S, name, allow=EXACT_ALLOW.get(name))
    # parity mode is as deterministic as the default one
    with switches(_C.EXACT):
        g2 = raw_backward(kw, res, wts)
    for k in g:
        assert torch.equal(g[k], g2[k]), f"exact mode: {k} not deterministic"


# ... and of the strict gate in the strictly conforming configuration (EXACT | REF_RECT), per case
STRICT_ALLOW = {}


@pytest.mark.parametrize("name", [n for n in CASES if n not in ILL_CONDITIONED])
def test_strict_mode_cases_against_reference_kernels(name):
    """The same cases in the strictly conforming configuration (EXACT | REF_RECT: the marked list, the compact hit list and
    the backward that walks it) against the reference's own kernels, end to end, with the lists compared entry for entry."""
    _ref()
    cam, sc, kw = _kw(name)
    S = sc.semantics.shape[1]
    strict_mode_against_reference(kw, syn.loss_weights(cam, S=S), S, name, allow=STRICT_ALLOW.get(name))


# ... and of SAME_STATE_GATE in the strict legs that run against the C oracle, per case: {tensor: elements outside}.
# edge65 (65 large overlapping splats, 195 elements in dL/dscales, so the gate's 4e-3 admits none): element 17 is 1.4e-4
# from the C oracle's same-state value (3.15175 vs 3.15131; 2.0e-5 of the tensor's scale, cap 1e-3) in parity and strict mode
# alike, compact walk or positional.  Measured on MI355X against the reference's OWN kernels the same element is 5e-5 away
# (3.15159) and no element of any tensor is outside rel 1e-4 + 2e-6 (worst 4.3e-6 of the scale), while those kernels
# themselves sit 9e-5 from the C oracle there, up to 5.0e-5 of the scale in dL/dcov3D, with one element of dL/drotations
# outside; their rerun spread is 8e-7.  All six dL/dcov3D entries of that Gaussian differ from the oracle's by the same 5.5e-5:
# the oracle's libm expf against the device's in the T recovery of a deep pixel (SATURATING_TOL), amplified by the cancelling
# dL/dconic -> dL/dcov3D sums (gpu_utils.CONDITIONED).  The library is between the two references.
STRICT_ORACLE_ALLOW = {"edge65": {"scales": 1}}


def _strict_legs(kw, wts, S, label, oracle_sum=False):
    """The strict leg of a case that has a `mode` parameter: against the C oracle always, and against the reference's own
    kernels as well where oracle/_ref travelled -- nothing is skipped.  (`oracle_sum`: strict_mode_against_reference.)"""
    from oracle import ref
    fw = oracle.forward(**kw)
    strict_mode_against_reference(kw, wts, S, label, rf=fw, allow=STRICT_ORACLE_ALLOW.get(label), oracle_sum=oracle_sum)
    fw.free()
    if ref.available():
        strict_mode_against_reference(kw, wts, S, label, allow=STRICT_ALLOW.get(label))


@pytest.mark.parametrize("name", ["mid_20k_sem3", "huge_splats", "sem19_deg1", "giant_degenerate"])
def test_culling_is_invisible_and_backward_is_deterministic(name):
    """The ballot cull may only skip pairs that fail the alpha test: images must be BIT-identical with the cull
    on and off; gradients bit-identical run to run (no atomics), with the backward walking the forward's hit record
    or redoing the geometric cull or walking everything; equal up to rounding with the DPP / shuffle reductions."""
    cam, sc, kw = _kw(name)
    wts = syn.loss_weights(cam, S=sc.semantics.shape[1])
    res_a, int_a = raw_forward(kw)
    g_a = raw_backward(kw, res_a, wts)
    g_a2 = raw_backward(kw, res_a, wts)
    for k in g_a:
        assert torch.equal(g_a[k], g_a2[k]), f"{k} not deterministic"
    # the scalar-walk kernel (switch USE_SW; S = 0 only, other widths fall through to the LDS kernel): the same terms summed
    # in another order (per quadrant, moments -> gradients once per Gaussian) -- deterministic, equal up to rounding, and
    # the row flags of the two kernels do not leak into each other when they follow one another over one forward
    if _C.has_variants():  # an A/B design outside the shipped library (tools/build_variant.py -DSGR_WITH_VARIANTS=1)
        with switches(_C.USE_SW):
            g_s = raw_backward(kw, res_a, wts)
            g_s2 = raw_backward(kw, res_a, wts)
        g_a3 = raw_backward(kw, res_a, wts)
        for k in g_a:
            assert torch.equal(g_s[k], g_s2[k]), f"{k} not deterministic (scalar walk)"
            assert torch.equal(g_a[k], g_a3[k]), f"{k} changed after a scalar-walk backward over the same forward"
            if name not in ILL_CONDITIONED:
                grad_close(npy(g_s[k]), npy(g_a[k]), rel=1e-4, abs_frac=2e-5, name=f"scalar walk vs LDS kernel:{k}", max_outlier_frac=0.0)
    if _C.has_variants():  # an A/B design outside the shipped library (tools/build_variant.py -DSGR_WITH_VARIANTS=1)
        with switches(_C.USE_RS_WAVE):  # the wave-cooperative row sum (A/B form): another fixed summation order
            g_w = raw_backward(kw, res_a, wts)
            g_w2 = raw_backward(kw, res_a, wts)
        for k in g_a:
            assert torch.equal(g_w[k], g_w2[k]), f"{k} not deterministic (wave-cooperative row sum)"
            if name not in ILL_CONDITIONED:
                grad_close(npy(g_w[k]), npy(g_a[k]), rel=1e-4, abs_frac=2e-5, name=f"wave row sum vs quads:{k}", max_outlier_frac=0.0)
    with switches(_C.NO_HITS):  # geometric cull instead of the hit record: a superset of the same visits
        g_h = raw_backward(kw, res_a, wts)
    for k in g_a:
        assert torch.equal(g_a[k], g_h[k]), f"hit record changed dL/d{k}"
    with switches(_C.NO_CULL):
        res_b, int_b = raw_forward(kw)
        for k in ["color", "depth", "alpha", "semantic"]:
            assert torch.equal(res_a[k], res_b[k]), f"cull changed {k}"
        assert torch.equal(int_a("n_contrib"), int_b("n_contrib"))
        g_b = raw_backward(kw, res_b, wts)
    for k in g_a:  # same pairs, same order: the cull must not change the gradients at all
        assert torch.equal(g_a[k], g_b[k]), f"cull changed dL/d{k}"
    g_b2 = raw_backward(kw, res_b, wts)  # hit record written by the un-culled forward
    for k in g_a:
        assert torch.equal(g_a[k], g_b2[k]), f"hit record of the un-culled forward changed dL/d{k}"
    if _C.has_variants():  # an A/B design outside the shipped library (tools/build_variant.py -DSGR_WITH_VARIANTS=1)
        with switches(_C.USE_SW):  # ... and walked by the scalar-walk kernel
            g_b3 = raw_backward(kw, res_b, wts)
        for k in g_s:
            assert torch.equal(g_s[k], g_b3[k]), f"scalar walk: hit record of the un-culled forward changed dL/d{k}"
    if _C.has_variants():  # an A/B design outside the shipped library (tools/build_variant.py -DSGR_WITH_VARIANTS=1)
        with switches(_C.USE_ONESWEEP):  # the radix sorts in their one-sweep A/B form: the same order, bit for bit
            res_s, int_s = raw_forward(kw)
            for k in ["keys", "point_list", "ranges", "point_offsets"]:
                assert torch.equal(int_a(k), int_s(k)), f"sort form changed {k}"
            for k in ["color", "depth", "alpha", "semantic"]:
                assert torch.equal(res_a[k], res_s[k]), f"sort form changed {k}"
    with switches(_C.PRE_STAGE_SH):  # SH rows through LDS in the preprocess (A/B form): the same operations, the same bits
        res_p, int_p = raw_forward(kw)
        vis = res_a["radii"] > 0
        for k in ["rgb", "clamped"]:
            assert torch.equal(int_a(k)[vis], int_p(k)[vis]), f"staged SH rows changed {k}"
        for k in ["color", "depth", "alpha", "semantic"]:
            assert torch.equal(res_a[k], res_p[k]), f"staged SH rows changed {k}"
    if name in ILL_CONDITIONED:
        return  # the comparisons below are rounding-level statements; they do not apply to cancelling quadratic forms
    with switches(_C.NO_DPP):
        g_c = raw_backward(kw, res_a, wts)
    for k in g_a:  # different summation order inside a wave: equal up to fp32 rounding
        grad_close(npy(g_a[k]), npy(g_c[k]), rel=1e-4, abs_frac=2e-5, name=f"dpp:{k}", max_outlier_frac=0.0)
    if _C.has_variants():  # an A/B design outside the shipped library (tools/build_variant.py -DSGR_WITH_VARIANTS=1)
        with switches(_C.USE_V2):  # S = 0: the transposed-accumulation A/B kernel (moments): equal up to rounding
            g_d = raw_backward(kw, res_a, wts)
            g_d2 = raw_backward(kw, res_a, wts)
        for k in g_a:
            assert torch.equal(g_d[k], g_d2[k]), f"{k} not deterministic (transposed accumulation)"
            grad_close(npy(g_a[k]), npy(g_d[k]), rel=1e-4, abs_frac=2e-5, name=f"v2:{k}", max_outlier_frac=0.0)


@pytest.mark.parametrize("mode", ["default", "exact"])
@pytest.mark.parametrize("name", list(CASES))
def test_tight_rects_are_invisible(name, mode):
    """The forward emits a Gaussian only for the tiles of the reference's rect (auxiliary.h:46-57) in which it can reach
    alpha >= 1/255 (sgr_preprocess.hip; sgr_test_switches bit 10 = the reference's whole rect).  The instances left out are
    ones the blend skips (forward.cu:428-430): every image must be bit-identical between the two forms -- including the
    ill-conditioned splats, whose conic cancels in fp32 --, the gradients equal up to the grouping of the row sum's additions,
    and the emitted list must be the full list with exactly those instances removed."""
    cam, sc, kw = _kw(name)
    S = sc.semantics.shape[1]
    wts = syn.loss_weights(cam, S=S)
    base = _C.test_switches(-1) | (_C.EXACT if mode == "exact" else 0)
    with switches(base | _C.REF_RECT):
        res_r, int_r = raw_forward(kw)
        g_r = raw_backward(kw, res_r, wts)
        full = dict(point_list=npy(int_r("point_list")).view(np.uint32), ranges=npy(int_r("ranges")).view(np.uint32),
                    keys=npy(int_r("keys")).view(np.uint64), n_contrib=npy(int_r("n_contrib")).view(np.uint32))
        rect_r = npy(int_r("tile_rect"))
    with switches(base):
        res, internal = raw_forward(kw)
        g = raw_backward(kw, res, wts)
        torch.cuda.synchronize()
        assert int(internal("num_rendered_reference")[0]) == res_r["R"]
        b = restrict_binning(internal, full["point_list"], full["ranges"], cam.image_width, cam.image_height, keys=full["keys"],
                             n_contrib=full["n_contrib"])
        assert res["R"] == b.num_rendered <= res_r["R"]
        assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
        assert (npy(internal("keys")).view(np.uint64) == b.keys).all()
        assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
        assert (npy(internal("n_contrib")).view(np.uint32).reshape(-1) == b.n_contrib.reshape(-1)).all()
        rect = npy(internal("tile_rect"))
        vis = npy(res["radii"]) > 0
        assert (rect[vis, 0] >= rect_r[vis, 0]).all() and (rect[vis, 2] <= rect_r[vis, 2]).all()
        assert (rect[vis, 1] >= rect_r[vis, 1]).all() and (rect[vis, 3] <= rect_r[vis, 3]).all()
        assert ((rect[vis, 2] > rect[vis, 0]) & (rect[vis, 3] > rect[vis, 1])).all(), "a visible Gaussian without a tile"
        assert (rect[~vis] == 0).all()
    assert torch.equal(res["radii"], res_r["radii"])
    for k in ["color", "depth", "alpha", "semantic"]:
        assert torch.equal(res[k], res_r[k]), f"tile rects changed {k}"
    # gradients: the same (pixel, Gaussian) terms; a Gaussian's partial rows are numbered inside its rect and the row sum adds
    # rows q, q + 4, ... per lane, so removing rows regroups the fp32 additions -- equal up to that rounding
    if name not in ILL_CONDITIONED:
        for k in g:
            grad_close(npy(g[k]), npy(g_r[k]), rel=1e-4, abs_frac=2e-5, name=f"tile rects:{k}", max_outlier_frac=0.0)
    if name == "mid_20k_sem3":
        assert res["R"] < 0.9 * res_r["R"]  # the point of it: far fewer instances to duplicate, sort, stage and reduce


def _sweep_scenes():
    """The 32 random scenes of test_tight_rects_are_invisible_random_sweep -> (seed, kw, W, H)."""
    for seed in range(32):
        rng = np.random.default_rng(7000 + seed)
        W, H = int(rng.integers(17, 500)), int(rng.integers(17, 320))
        cam = syn.make_camera(W, H, fx=float(rng.uniform(0.4, 1.6)) * W, yaw_deg=float(rng.uniform(-8, 8)))
        S = int(rng.choice([0, 0, 2, 5]))
        P = int(rng.integers(1, 6000))
        sc = syn.make_scene(P, cam, S=S, seed=seed, margin=float(rng.uniform(0.8, 1.8)), scale_px=float(rng.uniform(0.002, 0.05)),
                            zmin=float(rng.uniform(0.15, 2.0)), zmax=float(rng.uniform(5, 60)))
        kind = seed % 4
        if kind == 1:  # opacities straddling 1/255 = 0.00392 (the box is empty below 0.0039 and tiny just above)
            sc.opacities.copy_(torch.from_numpy(rng.uniform(0.0030, 0.0060, (P, 1)).astype(np.float32)))
        elif kind == 2:  # saturated opacities: the alpha >= 1/255 ellipse reaches 3.33 sigma, beyond the reference's square
            sc.opacities.copy_(torch.from_numpy(rng.uniform(0.9, 1.0, (P, 1)).astype(np.float32)))
        elif kind == 3:  # needles
            sc.scales[:, 0] *= float(rng.uniform(20, 300))
            sc.scales[:, 1:] *= 0.05
        kw = oracle_kwargs(cam, sc, deg=int(rng.integers(0, 4)), bg=torch.tensor(rng.uniform(0, 1, 3), dtype=torch.float32))
        kw["scale_modifier"] = float(rng.choice([1.0, 0.6, 1.5]))
        yield seed, kw, W, H


@pytest.mark.parametrize("mode", ["default", "exact", "strict"])
def test_tight_rects_are_invisible_random_sweep(mode):
    """The same statement over 32 random scenes that stress the box the rects are cut to: opacities around the 1/255 threshold
    (where the box collapses) and near 1 (where it is wider than the reference's 3-sigma square), needle-shaped and huge
    splats, scale modifiers, odd image sizes, off-screen centres.  Images bit-identical, the list = the full list minus the
    outside instances, n_contrib re-counted.
    mode "strict": the strict run (EXACT | REF_RECT) of each scene against the C oracle instead of against the other rect
    mode -- num_rendered, radii, point_list, ranges and keys identical, entry for entry."""
    if mode == "strict":
        seen = 0
        for seed, kw, W, H in _sweep_scenes():
            fw = oracle.forward(**kw)
            with switches(_C.test_switches(-1) | _C.EXACT | _C.REF_RECT):
                res, internal = raw_forward(kw)
                assert res["R"] == fw.num_rendered == int(internal("num_rendered_reference")[0]), seed
                assert np.array_equal(npy(res["radii"]), fw.radii), seed
                assert np.array_equal(npy(internal("point_list")).view(np.uint32), fw.point_list), seed
                assert np.array_equal(npy(internal("ranges")).view(np.uint32), fw.ranges), seed
                assert np.array_equal(npy(internal("keys")).view(np.uint64), fw.keys), seed
            seen += fw.num_rendered
            fw.free()
        assert seen > 0
        return
    base = _C.test_switches(-1) | (_C.EXACT if mode == "exact" else 0)
    removed = total = 0
    for seed, kw, W, H in _sweep_scenes():
        with switches(base | _C.REF_RECT):
            res_r, int_r = raw_forward(kw)
            full = [npy(int_r(k)) for k in ("point_list", "ranges", "keys", "n_contrib")]
        with switches(base):
            res, internal = raw_forward(kw)
            assert torch.equal(res["radii"], res_r["radii"]), seed
            for k in ["color", "depth", "alpha", "semantic"]:
                assert torch.equal(res[k], res_r[k]), (seed, k)
            if res_r["R"] == 0:
                assert res["R"] == 0
                continue
            b = restrict_binning(internal, full[0].view(np.uint32), full[1].view(np.uint32), W, H, keys=full[2].view(np.uint64),
                                 n_contrib=full[3].view(np.uint32))
            assert res["R"] == b.num_rendered, seed
            if b.num_rendered:
                assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all(), seed
            assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all(), seed
            assert (npy(internal("n_contrib")).view(np.uint32).reshape(-1) == b.n_contrib.reshape(-1)).all(), seed
            removed += b.removed
            total += res_r["R"]
    assert removed > 0.1 * total


@pytest.mark.parametrize("mode", ["default", "exact", "strict"])
@pytest.mark.parametrize("P,S,scale_px", [(1, 0, 0.8), (2, 20, 0.3), (65, 1, 0.05), (129, 7, 0.02)])
def test_edge_sizes(P, S, scale_px, mode):
    """Ragged sizes: fewer Gaussians than a wave, one Gaussian covering the whole tile grid (a single owner of every
    slot in the cooperative duplicate kernel), the reference's maximum number of semantic channels (NUM_CLASSES = 20, config.h:16), P just past a wave boundary.
    mode "exact": the parity mode against the reference's own kernels, north_star's gate itself, end to end.
    mode "strict": EXACT | REF_RECT with the lists entry for entry, against the C oracle and the reference's kernels."""
    cam = syn.make_camera(200, 120, fx=150.0)
    sc = syn.make_scene(P, cam, S=S, seed=20 + P, scale_px=scale_px, zmin=2.0, zmax=4.0, margin=0.5)
    kw = oracle_kwargs(cam, sc, deg=3)
    wts = syn.loss_weights(cam, S=S)
    if mode == "exact":
        _ref()
        exact_mode_against_reference_kernels(kw, wts, S, f"edge{P}")
        return
    if mode == "strict":
        _strict_legs(kw, wts, S, f"edge{P}")
        return
    fw = oracle.forward(**kw)
    ref = oracle.backward(fw, wts["color"], wts["depth"], wts["alpha"], wts["semantic"] if S else None)
    res, internal = raw_forward(kw)
    b = restrict_oracle(internal, fw, kw)
    assert res["R"] == b.num_rendered and b.num_rendered > 0
    assert (npy(res["radii"]) == fw.radii).all()
    assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
    assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
    image_close(npy(res["color"]), fw.color, name="color")
    image_close(npy(res["alpha"]), fw.alpha, name="alpha")
    image_close(npy(res["semantic"]), fw.semantic, name="semantic")
    g = raw_backward(kw, res, wts)
    same = oracle_backward_same_state(oracle, fw, res, wts, S)
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"same-state edge{P}:{k}", **SAME_STATE_GATE)
        grad_close(npy(g[k]).reshape(ref[k].shape), ref[k], rel=2e-4, abs_frac=3e-4, name=f"edge{P}:{k}")  # end to end, large overlapping splats: see SATURATING_TOL
    fw.free()


def test_side_stream_varying_sizes_and_repeated_backward():
    """The binning buffer is sized from the previous call's num_rendered (grow, shrink, grow), work may run on a
    non-default stream, and backward may run twice on one forward (retain_graph): results never change."""
    from diff_gaussian_rasterization import GaussianRasterizer
    order = ["tiny_sh3_sem2", "mid_20k_sem3", "tiny_sh3_sem2", "huge_splats", "mid_20k_sem3"]

    def run(name):
        cam, sc, _ = _kw(name)
        S = sc.semantics.shape[1]
        t = {k: dev(getattr(sc, k)).requires_grad_(True) for k in ["means3D", "scales", "rotations", "opacities", "shs"]}
        sem = dev(sc.semantics) if S else None
        outs = GaussianRasterizer(settings(cam))(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"],
                                                 rotations=t["rotations"], semantics=sem)
        w = syn.loss_weights(cam, S=S)
        sel = [outs[0], outs[2], outs[3]]
        ups = [dev(w["color"]), dev(w["depth"]), dev(w["alpha"])]
        torch.autograd.backward(sel, ups, retain_graph=True)
        g1 = {k: v.grad.clone() for k, v in t.items()}
        for v in t.values():
            v.grad = None
        torch.autograd.backward(sel, ups)  # second backward over the same buffers
        g2 = {k: v.grad.clone() for k, v in t.items()}
        return [o.detach().clone() for o in outs], g1, g2

    base = {}
    for name in dict.fromkeys(order):
        base[name] = run(name)
        for k in base[name][1]:  # every instantiation of the backward is bit-reproducible
            assert torch.equal(base[name][1][k], base[name][2][k]), (name, k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for name in order:
            outs, g1, _ = run(name)
            for a, b in zip(outs, base[name][0]):
                assert torch.equal(a, b), name
            for k in g1:
                assert torch.equal(g1[k], base[name][1][k]), (name, k)
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("mode", ["default", "exact", "strict"])
@pytest.mark.parametrize("seed", range(8))
def test_random_scenes_against_oracle(seed, mode):
    """Randomised sweep: odd image sizes, yawed cameras, off-screen margins, scale modifiers, backgrounds, SH degrees
    and semantic widths drawn from the seed; integer outputs bit-exact, images and gradients within tolerance.
    mode "exact": the parity mode against the reference's own kernels, north_star's gate itself, end to end.
    mode "strict": EXACT | REF_RECT with the lists entry for entry, against the C oracle and the reference's kernels."""
    rng = np.random.default_rng(1000 + seed)
    W, H = int(rng.integers(17, 400)), int(rng.integers(17, 300))
    cam = syn.make_camera(W, H, fx=float(rng.uniform(0.4, 1.6)) * W, yaw_deg=float(rng.uniform(-8, 8)))
    S = int(rng.choice([0, 1, 3, 9]))
    P = int(rng.integers(1, 4000))
    sc = syn.make_scene(P, cam, S=S, seed=seed, margin=float(rng.uniform(0.8, 1.8)), scale_px=float(rng.uniform(0.002, 0.02)),
                        zmin=float(rng.uniform(0.15, 2.0)), zmax=float(rng.uniform(5, 60)))
    deg = int(rng.integers(0, 4))
    kw = oracle_kwargs(cam, sc, deg=deg, bg=torch.tensor(rng.uniform(0, 1, 3), dtype=torch.float32))
    kw["scale_modifier"] = float(rng.choice([1.0, 0.7, 1.3]))
    wts = syn.loss_weights(cam, S=S, seed=seed)
    if mode == "exact":
        _ref()
        exact_mode_against_reference_kernels(kw, wts, S, f"rand{seed}")
        return
    if mode == "strict":
        _strict_legs(kw, wts, S, f"rand{seed}")
        return
    fw = oracle.forward(**kw)
    ref = oracle.backward(fw, wts["color"], wts["depth"], wts["alpha"], wts["semantic"] if S else None)
    res, internal = raw_forward(kw)
    b = restrict_oracle(internal, fw, kw)
    assert res["R"] == b.num_rendered
    assert (npy(res["radii"]) == fw.radii).all()
    if b.num_rendered:
        assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
        assert (npy(internal("keys")).view(np.uint64) == b.keys).all()
    assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
    image_close(npy(res["color"]), fw.color, name="color")
    image_close(npy(res["depth"]), fw.depth, name="depth")
    image_close(npy(res["alpha"]), fw.alpha, name="alpha")
    image_close(npy(res["semantic"]), fw.semantic, name="semantic")
    g = raw_backward(kw, res, wts)
    same = oracle_backward_same_state(oracle, fw, res, wts, S)
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"same-state rand{seed}:{k}", **SAME_STATE_GATE)
        grad_close(npy(g[k]).reshape(ref[k].shape), ref[k], rel=2e-4, abs_frac=3e-4, name=f"rand{seed}:{k}")  # end to end
    fw.free()


def _width_case(S):
    cam = syn.make_camera(224, 160, fx=250.0)
    sc = syn.make_scene(3000, cam, S=S, seed=40 + S, scale_px=0.01)
    return oracle_kwargs(cam, sc, deg=2), syn.loss_weights(cam, S=S, seed=S)


@pytest.mark.parametrize("S", [5, 11, 14, 16, 18])
def test_every_channel_width_strict(S):
    """The same widths in the strictly conforming configuration: the SMAX = 8 / 12 / 16 / 20 instantiations of the backward
    that walks the compact hit list, whose rounds end inside a list at the odd widths."""
    kw, wts = _width_case(S)
    _strict_legs(kw, wts, S, f"S{S}")


@pytest.mark.parametrize("S", [5, 11, 14, 16, 18])
def test_every_channel_width_against_oracle(S):
    """One case per kernel instantiation the reference's channel limit allows (SMAX = 8, 12, 16, 20; 4 and 20 are in
    CASES): they are compiled with different register caps, round sizes and reduction chunking."""
    kw, wts = _width_case(S)
    fw = oracle.forward(**kw)
    res, internal = raw_forward(kw)
    assert res["R"] == restrict_oracle(internal, fw, kw).num_rendered
    image_close(npy(res["semantic"]), fw.semantic, name="semantic")
    image_close(npy(res["color"]), fw.color, name="color")
    g = raw_backward(kw, res, wts)
    same = oracle_backward_same_state(oracle, fw, res, wts, S)
    for k in GRAD_KEYS:
        grad_close(npy(g[k]).reshape(same[k].shape), same[k], name=f"same-state S{S}:{k}", **SAME_STATE_GATE)
    g2 = raw_backward(kw, res, wts)
    for k in g:
        assert torch.equal(g[k], g2[k]), f"S={S}: {k} not deterministic"
    fw.free()


@pytest.mark.parametrize("S", [24, 32])
def test_widest_instantiations_agree_with_the_narrower_ones_strict(S):
    """The same agreement under EXACT | REF_RECT.  The reference stops at 20 channels, so nothing outside the library can
    be the reference here: the narrower strict runs (held to the reference by the other strict legs) are."""
    with switches(_C.test_switches(-1) | _C.EXACT | _C.REF_RECT):
        _widest_agree(S)


@pytest.mark.parametrize("S", [24, 32])
def test_widest_instantiations_agree_with_the_narrower_ones(S):
    """More than 20 channels is beyond the reference (NUM_CLASSES = 20, config.h:16) and so beyond the oracle; the API
    allows up to 32.  Channels are independent of each other in the forward, and in the backward they meet only in a
    sum: a run with S channels must reproduce, bit for bit, the run with its first S/2 channels -- semantic image,
    and every gradient when the upstream gradient of the other half is zero."""
    _widest_agree(S)


def _widest_agree(S):
    cam = syn.make_camera(200, 144, fx=230.0)
    sc = syn.make_scene(2500, cam, S=S, seed=70 + S, scale_px=0.012)
    h = S // 2
    kw = oracle_kwargs(cam, sc, deg=1)
    kw_h = dict(kw, semantics=kw["semantics"][:, :h].contiguous())
    wts = syn.loss_weights(cam, S=S, seed=S)
    wts["semantic"] = wts["semantic"].clone()
    wts["semantic"][h:] = 0
    wts_h = dict(wts, semantic=wts["semantic"][:h].contiguous())
    res, _ = raw_forward(kw)
    res_h, _ = raw_forward(kw_h)
    assert torch.equal(res["semantic"][:h], res_h["semantic"])
    for k in ["color", "depth", "alpha"]:
        assert torch.equal(res[k], res_h[k]), k
    g, g_h = raw_backward(kw, res, wts), raw_backward(kw_h, res_h, wts_h)
    for k in GRAD_KEYS:
        if k == "semantics":
            assert torch.equal(g[k][:, :h], g_h[k]), "semantics (first half)"
        else:
            assert torch.equal(g[k], g_h[k]), k
    # the second half of the channel gradients: the same statement with the halves swapped
    wts2 = dict(wts, semantic=syn.loss_weights(cam, S=S, seed=S)["semantic"].clone())
    wts2["semantic"][:h] = 0
    kw_t = dict(kw, semantics=kw["semantics"][:, h:].contiguous())
    res_t, _ = raw_forward(kw_t)
    assert torch.equal(res["semantic"][h:], res_t["semantic"])
    g2 = raw_backward(kw, res, wts2)
    g_t = raw_backward(kw_t, res_t, dict(wts2, semantic=wts2["semantic"][h:].contiguous()))
    assert torch.equal(g2["semantics"][:, h:], g_t["semantics"])
    assert torch.equal(g2["means3D"], g_t["means3D"])


def test_precomputed_colors_and_cov3D():
    cam, sc, _ = CASES["mid_20k_sem3"]
    g = torch.Generator().manual_seed(5)
    colors = torch.rand(sc.P, 3, generator=g)
    fw0 = oracle.forward(**oracle_kwargs(cam, sc))
    cov6 = torch.from_numpy(fw0.cov3D.copy())
    kw = oracle_kwargs(cam, sc, use_sh=False, colors=colors, use_cov_precomp=True, cov3D=cov6)
    fw = oracle.forward(**kw)
    wts = syn.loss_weights(cam, S=3)
    ref = oracle.backward(fw, wts["color"], wts["depth"], wts["alpha"], wts["semantic"])
    res, internal = raw_forward(kw)
    b = restrict_oracle(internal, fw, kw)
    assert res["R"] == b.num_rendered and (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
    image_close(npy(res["color"]), fw.color, name="color")
    gr = raw_backward(kw, res, wts)
    for k in ["means2D", "colors", "opacity", "means3D", "cov3D", "semantics"]:
        grad_close(npy(gr[k]).reshape(ref[k].shape), ref[k], name=k)
    assert float(gr["scales"].abs().max()) == 0.0 and float(gr["rotations"].abs().max()) == 0.0


def test_precomputed_colors_and_cov3D_strict():
    """colors_precomp + cov3D_precomp in the strictly conforming configuration: the lists entry for entry."""
    cam, sc, _ = CASES["mid_20k_sem3"]
    g = torch.Generator().manual_seed(5)
    colors = torch.rand(sc.P, 3, generator=g)
    fw0 = oracle.forward(**oracle_kwargs(cam, sc))
    cov6 = torch.from_numpy(fw0.cov3D.copy())
    fw0.free()
    kw = oracle_kwargs(cam, sc, use_sh=False, colors=colors, use_cov_precomp=True, cov3D=cov6)
    wts = syn.loss_weights(cam, S=3)
    fw = oracle.forward(**kw)
    res, g_, _ = strict_mode_against_reference(kw, wts, 3, "precomputed", rf=fw)
    fw.free()
    assert float(g_["scales"].abs().max()) == 0.0 and float(g_["rotations"].abs().max()) == 0.0
    from oracle import ref
    if ref.available():
        strict_mode_against_reference(kw, wts, 3, "precomputed")


def test_smoke_recipe_config0():
    """BASELINE config 1 / the reference's only test (script/test_gaussian_rasterization.py:44-91):
    10k random Gaussians, SH degree 0 with M=4, un-normalised quaternions, then 15 semantic channels."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    import math
    c = syn.smoke_test_camera()
    for (H, W) in [(375, 1242), (256, 256)]:
        g = torch.Generator().manual_seed(0)
        n = 10000
        means3D, means2D = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
        shs, opacity = torch.rand(n, 4, 3, generator=g), torch.rand(n, 1, generator=g)
        scales, rotations = torch.rand(n, 3, generator=g), torch.rand(n, 4, generator=g)
        rotations[:, 0] = 1
        semantics = torch.rand(n, 15, generator=g)
        tanx, tany = math.tan(c["FoVx"] * 0.5), math.tan(c["FoVy"] * 0.5)
        st = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, bg=torch.zeros(3).cuda(), scale_modifier=1.0,
            viewmatrix=c["world_view_transform"].cuda(), projmatrix=c["full_proj_transform"].cuda(), sh_degree=0,
            campos=c["camera_center"].cuda(), prefiltered=False, debug=True)
        rast = GaussianRasterizer(raster_settings=st)
        for sem in (None, semantics):
            img, radii, depth, alpha, semo = rast(means3D=means3D.cuda(), means2D=means2D.cuda(), shs=shs.cuda(),
                                                  colors_precomp=None, opacities=opacity.cuda(), scales=scales.cuda(),
                                                  rotations=rotations.cuda(), cov3D_precomp=None,
                                                  semantics=None if sem is None else sem.cuda())
            fw = oracle.forward(means3D=means3D, opacities=opacity, viewmatrix=c["world_view_transform"],
                                projmatrix=c["full_proj_transform"], campos=c["camera_center"], bg=torch.zeros(3),
                                tanfovx=tanx, tanfovy=tany, image_height=H, image_width=W, sh_degree=0, shs=shs,
                                scales=scales, rotations=rotations, semantics=sem)
            assert (npy(radii) == fw.radii).all()
            image_close(npy(img), fw.color, name="smoke color")
            image_close(npy(depth), fw.depth, name="smoke depth")
            image_close(npy(alpha), fw.alpha, name="smoke alpha")
            image_close(npy(semo), fw.semantic, name="smoke semantic")
            fw.free()


def test_autograd_api_and_error_behaviour():
    from diff_gaussian_rasterization import GaussianRasterizer
    from street_gaussians_amd._native import SgrError
    cam, sc, kw = _kw("tiny_sh3_sem2")
    st = settings(cam, bg=torch.tensor([0.3, 0.1, 0.7]))
    rast = GaussianRasterizer(raster_settings=st)
    t = {k: dev(getattr(sc, k)).requires_grad_(True) for k in ["means3D", "scales", "rotations", "opacities", "shs", "semantics"]}
    m2d = torch.zeros(sc.P, 3, device="cuda", requires_grad=True)
    color, radii, depth, alpha, sem = rast(t["means3D"], m2d, t["opacities"], shs=t["shs"], scales=t["scales"],
                                           rotations=t["rotations"], semantics=t["semantics"])
    wts = syn.loss_weights(cam, S=2)
    loss = (color * dev(wts["color"])).sum() + (depth * dev(wts["depth"])).sum() + (alpha * dev(wts["alpha"])).sum() + \
        (sem * dev(wts["semantic"])).sum()
    loss.backward()
    fw = oracle.forward(**kw)
    ref = oracle.backward(fw, wts["color"], wts["depth"], wts["alpha"], wts["semantic"])
    grad_close(npy(t["means3D"].grad), ref["means3D"], name="means3D")
    grad_close(npy(m2d.grad), ref["means2D"], name="means2D")
    grad_close(npy(t["shs"].grad), ref["sh"], name="sh")
    grad_close(npy(t["opacities"].grad), ref["opacity"], name="opacity")
    grad_close(npy(t["scales"].grad), ref["scales"], name="scales")
    grad_close(npy(t["rotations"].grad), ref["rotations"], name="rotations")
    grad_close(npy(t["semantics"].grad), ref["semantics"], name="semantics")
    # a loss on the colour image alone (train.py's usual case): the outputs without a gradient count as zero, exactly
    # as if zeros had been passed for them
    def only_color(explicit_zeros):
        for p_ in list(t.values()) + [m2d]:
            p_.grad = None
        c_, _, d_, a_, s_ = rast(t["means3D"], m2d, t["opacities"], shs=t["shs"], scales=t["scales"],
                                 rotations=t["rotations"], semantics=t["semantics"])
        if explicit_zeros:
            torch.autograd.backward([c_, d_, a_, s_], [dev(wts["color"]), torch.zeros_like(d_), torch.zeros_like(a_),
                                                       torch.zeros_like(s_)])
        else:
            (c_ * dev(wts["color"])).sum().backward()
        return {k: v.grad.clone() for k, v in t.items()}
    ga, gb = only_color(False), only_color(True)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # eval mode: means2D=None, no semantics (street_gaussian_renderer.py:170-173)
    with torch.no_grad():
        out = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    assert out[4].shape == (0, cam.image_height, cam.image_width)
    # argument validation (reference __init__.py:201-205)
    with pytest.raises(Exception, match="excatly one"):
        rast(t["means3D"], None, t["opacities"], scales=t["scales"], rotations=t["rotations"])
    with pytest.raises(Exception, match="exactly one"):
        rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"])
    with pytest.raises(RuntimeError, match="num_points, 3"):
        rast(t["means3D"].reshape(-1), None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    with pytest.raises(SgrError, match="no CPU path"):
        rast(t["means3D"].cpu(), None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    with pytest.raises(SgrError, match=r"\[0, 32\]"):
        rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
             semantics=torch.zeros(sc.P, 40, device="cuda"))
    # P == 0 is legal (rasterize_points.cu:86)
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = rast(z(0, 3), None, z(0, 1), shs=z(0, 16, 3), scales=z(0, 3), rotations=z(0, 4))
    assert float(out[0].abs().max()) == 0.0 and out[1].numel() == 0
    # markVisible / visible_filter
    mv = rast.markVisible(t["means3D"].detach())
    assert (npy(mv) == oracle.mark_visible(sc.means3D, cam.viewmatrix, cam.projmatrix)).all()
    r2, m2 = rast.visible_filter(t["means3D"].detach(), scales=t["scales"].detach(), rotations=t["rotations"].detach())
    assert (npy(r2) == fw.radii).all()
    assert (npy(m2)[fw.radii > 0] == fw.means2D[fw.radii > 0]).all()
    fw.free()


def test_far_depths_fall_back_to_the_32_bit_depth_sort():
    """The depth sort orders 27 key bits (depth bits minus the bits of 0.2: below 2^27 for depths under 13 107) in three
    passes.  A scene with a Gaussian farther away than that raises a device flag that comes back with num_rendered, and the
    forward repeats its front end with a sort on all 32 bits: the order must be the oracle's either way."""
    cam = syn.make_camera(160, 96, fx=170.0)
    sc = syn.make_scene(400, cam, S=0, seed=31, scale_px=0.02, zmin=1.0, zmax=8.0)
    far = sc.means3D.clone()
    far[::7, :] = far[::7, :] * torch.tensor([1.0, 1.0, 0.0]) * 3000.0 + torch.tensor([0.0, 0.0, 1.0]) * torch.linspace(13000.0, 90000.0, far[::7].shape[0])[:, None]
    sc.means3D.copy_(far)
    sc.scales[::7] *= 4000.0  # so that the far ones still cover pixels
    kw = oracle_kwargs(cam, sc)
    fw = oracle.forward(**kw)
    assert (fw.depths[fw.radii > 0] > 13107.2).sum() >= 3 and (fw.depths[fw.radii > 0] < 13107.2).sum() > 100
    for _ in range(2):  # the first call takes the repeat, the second starts with the wide sort (kept for the next 64 forwards)
        res, internal = raw_forward(kw)
        b = restrict_oracle(internal, fw, kw)
        assert res["R"] == b.num_rendered
        assert (npy(internal("keys")).view(np.uint64) == b.keys).all()
        assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
        assert (npy(internal("point_offsets")).view(np.uint32) == b.point_offsets).all()
        image_close(npy(res["color"]), fw.color, name="far color")
    fw.free()


def test_far_depths_fall_back_to_the_32_bit_depth_sort_strict():
    """The same fallback in the strictly conforming configuration: the repeat of the front end and the wide sort must leave
    the reference's list, entry for entry, marks and compact list included."""
    cam = syn.make_camera(160, 96, fx=170.0)
    sc = syn.make_scene(400, cam, S=0, seed=31, scale_px=0.02, zmin=1.0, zmax=8.0)
    far = sc.means3D.clone()
    far[::7, :] = far[::7, :] * torch.tensor([1.0, 1.0, 0.0]) * 3000.0 + torch.tensor([0.0, 0.0, 1.0]) * torch.linspace(13000.0, 90000.0, far[::7].shape[0])[:, None]
    sc.means3D.copy_(far)
    sc.scales[::7] *= 4000.0
    kw = oracle_kwargs(cam, sc)
    fw = oracle.forward(**kw)
    assert (fw.depths[fw.radii > 0] > 13107.2).sum() >= 3 and (fw.depths[fw.radii > 0] < 13107.2).sum() > 100
    with switches(_C.test_switches(-1) | _C.EXACT | _C.REF_RECT):
        for _ in range(2):  # the first call takes the repeat, the second starts with the wide sort
            res, internal = raw_forward(kw)
            assert res["R"] == fw.num_rendered
            assert np.array_equal(npy(internal("keys")).view(np.uint64), fw.keys)
            assert np.array_equal(npy(internal("point_list")).view(np.uint32), fw.point_list)
            assert np.array_equal(npy(internal("point_offsets")).view(np.uint32), fw.point_offsets)
            assert np.array_equal(npy(internal("ranges")).view(np.uint32), fw.ranges)
            image_close(npy(res["color"]), fw.color, name="far color, strict")
    strict_mode_against_reference(kw, syn.loss_weights(cam, S=0), 0, "far depths", rf=fw)
    fw.free()


def test_prefiltered_raises_instead_of_trapping():
    from diff_gaussian_rasterization import GaussianRasterizer
    from street_gaussians_amd._native import SgrError
    cam, sc, _ = CASES["tiny_sh3_sem2"]
    rast = GaussianRasterizer(raster_settings=settings(cam, prefiltered=True))
    m = dev(sc.means3D * torch.tensor([1.0, 1.0, -1.0]))
    with pytest.raises(SgrError, match="prefiltered"):
        rast(m, None, dev(sc.opacities), shs=dev(sc.shs), scales=dev(sc.scales), rotations=dev(sc.rotations))


def _knn_clouds(sizes, seed):
    """(name, points): per size a cloud that straddles the origin on every axis, one with every coordinate positive (in
    [3, 13]^3: the {0,0,0} initial value of the bounding-box reduction, cub's `init` in the reference, then widens the box)
    and one with a constant non-zero axis (an all-zero axis divides 0 by 0 in the Morton code, which nothing defines).
    Every cloud of more than one point has a duplicated point."""
    g = torch.Generator().manual_seed(seed)
    for n in sizes:
        straddling = torch.rand(n, 3, generator=g) * torch.tensor([10.0, 4.0, 7.0]) - 2.0
        positive = torch.rand(n, 3, generator=g) * 10.0 + 3.0
        flat = torch.rand(n, 3, generator=g) * torch.tensor([10.0, 4.0, 7.0]) - 2.0
        flat[:, 1] = -2.5 if n % 2 else 1.75
        for name, pts in (("straddling", straddling), ("positive", positive), ("flat-y", flat)):
            pts[n // 2] = pts[0]
            yield f"{name} n={n}", pts


def _same_bits(a, b):
    """Array equality on the bits: inf (fewer than four points: a missing neighbour's distance stays FLT_MAX and the sum
    overflows) is a value like any other."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


KNN_SMALL = [1, 2, 3, 4]  # fewer points than neighbours + 1, and the first size with three of them


def test_knn_matches_oracle_bit_exact():
    """Sizes: KNN_SMALL, one box exactly (1024) and one point more, the edge of the bounding-box reduction's blocks (4096 /
    4097), and several boxes."""
    from simple_knn._C import distCUDA2
    for name, pts in _knn_clouds(KNN_SMALL + [5, 1000, 1024, 1025, 4096, 4097, 50000], seed=3):
        want = oracle.dist2(pts)
        n = pts.shape[0]
        if n < 3:    # the cases are what they are there for: no third neighbour, and below three points not even a sum
            assert np.isinf(want).all(), name
        else:
            assert np.isfinite(want).all() and bool((want > 1e37).all()) == (n == 3), name
        assert _same_bits(npy(distCUDA2(pts.cuda())), want), name


# ---------------------------------------------------------------------------------------------------
# secondary oracle: the reference's own kernels on this GPU
def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libref_rasterizer.so did not travel (built only where /root/reference exists)")
    return ref


@pytest.mark.parametrize("name", ["mid_20k_sem3", "ragged_clamped_offscreen", "huge_splats"])
def test_against_reference_kernels(name):
    ref = _ref()
    cam, sc, kw = _kw(name)
    S = sc.semantics.shape[1]
    wts = syn.loss_weights(cam, S=S)
    rf = ref.forward(**kw)
    fw = oracle.forward(**kw)
    res, internal = raw_forward(kw)
    # the reference build, the C oracle and the HIP path agree on every integer output
    # (the HIP path: the same arrays restricted to the tile rects it emits -- gpu_utils.restrict_binning)
    b = restrict_oracle(internal, rf, kw)
    assert rf.num_rendered == fw.num_rendered and res["R"] == b.num_rendered
    assert (npy(rf.radii) == fw.radii).all() and (npy(res["radii"]) == fw.radii).all()
    assert (npy(rf.internal("point_list")).view(np.uint32) == fw.point_list).all()
    assert (npy(rf.internal("keys")).view(np.uint64) == fw.keys).all()
    assert (npy(rf.internal("ranges")).view(np.uint32) == fw.ranges).all()
    assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
    assert (npy(internal("keys")).view(np.uint64) == b.keys).all()
    assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
    for k in ["color", "depth", "alpha", "semantic"]:
        image_close(npy(res[k]), npy(getattr(rf, k)), name=f"hip vs ref {k}")
        image_close(getattr(fw, k), npy(getattr(rf, k)), name=f"oracle vs ref {k}")
    gref = ref.backward(rf, wts["color"], wts["depth"], wts["alpha"], wts["semantic"])
    gor = oracle.backward(fw, wts["color"], wts["depth"], wts["alpha"], wts["semantic"])
    g = raw_backward(kw, res, wts)
    mags = _color_mag(fw, wts) if name == "huge_splats" else {}
    tol, af = SATURATING_TOL.get(name, (1e-4, 2e-6))
    for k in ["means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "semantics"]:
        grad_close(npy(g[k]).reshape(gor[k].shape), npy(gref[k]).reshape(gor[k].shape), name=f"hip vs ref {k}",
                   rel=tol, abs_frac=af, mag=mags.get(k))
        grad_close(gor[k], npy(gref[k]).reshape(gor[k].shape), name=f"oracle vs ref {k}", rel=tol, abs_frac=af,
                   mag=mags.get(k))
    rf.free()
    fw.free()


def test_knn_against_reference_kernels():
    ref = _ref()
    from simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(7)
    pts = torch.randn(200000, 3, generator=g) * torch.tensor([30.0, 3.0, 40.0])
    assert torch.equal(distCUDA2(pts.cuda()), ref.dist2(pts))
    for name, pts in _knn_clouds(KNN_SMALL + [1024, 4097], seed=8):
        assert _same_bits(npy(distCUDA2(pts.cuda())), npy(ref.dist2(pts))), name


# ---------------------------------------------------------------------------------------------------
# golden fixtures generated from the reference kernels on the MI355X box (tests/golden/make_golden.py)
@pytest.mark.parametrize("mode", ["default", "exact", "strict"])
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(HERE, "golden", "*.npz"))) or [None])
def test_golden_fixture(path, mode):
    if path is None:
        pytest.skip("no golden fixtures committed yet")
    from golden.make_golden import load_case
    kw, wts, gold = load_case(path)
    if mode == "exact":  # the committed outputs of the reference's kernels: bit-identical images, the north-star gate itself
        S = int(gold["semantics"].shape[1])
        exact_mode_against_reference_kernels(kw, wts, S, "golden " + os.path.basename(path), rf=gold, gref=gold)
        return
    if mode == "strict":  # ... with the file's lists, n_contrib and num_rendered entry for entry
        S = int(gold["semantics"].shape[1])
        strict_mode_against_reference(kw, wts, S, "golden " + os.path.basename(path), rf=gold, gref=gold)
        return
    res, internal = raw_forward(kw)
    b = restrict_binning(internal, gold["point_list"], gold["ranges"], int(kw["image_width"]), int(kw["image_height"]))
    assert res["R"] == b.num_rendered and int(internal("num_rendered_reference")[0]) == int(gold["num_rendered"])
    assert (npy(res["radii"]) == gold["radii"]).all()
    assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
    assert (npy(internal("ranges")).view(np.uint32) == b.ranges).all()
    for k in ["color", "depth", "alpha", "semantic"]:
        image_close(npy(res[k]), gold[k], name=f"golden {k}")
    g = raw_backward(kw, res, wts)
    rel, af = (2e-3, 2e-4) if "dense" in os.path.basename(path) else (1e-4, 2e-6)  # see tests/test_golden_cpu.py
    for k in ["means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "semantics"]:
        grad_close(npy(g[k]).reshape(gold["g_" + k].shape), gold["g_" + k], rel=rel, abs_frac=af, name=f"golden {k}")


# ---------------------------------------------------------------------------------------------------
# BASELINE.json full sizes: size-independent properties (the oracle would take minutes here)
@pytest.mark.parametrize("P,S", [(500_000, 0), (1_000_000, 0), (300_000, 19)])
def test_full_size_properties(P, S):
    cam = syn.make_camera(1920, 1280, fx=2050.0)
    sc = syn.make_scene(P, cam, S=S, seed=0)
    bg0, bg1 = torch.zeros(3), torch.tensor([0.2, 0.5, 0.9])
    kw = oracle_kwargs(cam, sc, bg=bg0)
    res, internal = raw_forward(kw)
    R = res["R"]
    keys = npy(internal("keys")).view(np.uint64)
    tiles_touched = npy(internal("tiles_touched")).view(np.uint32)
    assert R == int(tiles_touched.astype(np.int64).sum()) and R > P
    assert (np.diff(keys.astype(np.int64)) >= 0).all(), "keys not sorted"
    pl = npy(internal("point_list")).view(np.uint32)
    same = np.diff(keys.astype(np.int64)) == 0
    assert (np.diff(pl.astype(np.int64))[same] > 0).all(), "sort not stable"
    # the sorted list is a permutation of the duplicated instances
    assert (np.bincount(pl, minlength=P) == tiles_touched).all()
    rg = npy(internal("ranges")).view(np.uint32)
    tile_of = (keys >> np.uint64(32)).astype(np.int64)
    counts = np.bincount(tile_of, minlength=rg.shape[0])
    assert ((rg[:, 1] - rg[:, 0]) == counts).all()
    nz = counts > 0
    assert (rg[nz, 0] == (np.cumsum(counts) - counts)[nz]).all()
    a = npy(res["alpha"])
    assert a.min() >= 0.0 and a.max() <= 1.0 + 1e-5
    # background enters linearly with the final transmittance: out(bg1) - out(bg0) = T_final * (bg1 - bg0)
    res1, _ = raw_forward(oracle_kwargs(cam, sc, bg=bg1))
    T_final = 1.0 - a
    d = npy(res1["color"]) - npy(res["color"])
    assert np.abs(d - T_final * bg1.numpy()[:, None, None]).max() <= 2e-5
    for k in ["depth", "alpha", "semantic"]:
        assert torch.equal(res[k], res1[k])
    # culling invisible at full size as well
    with switches(_C.NO_CULL):
        res2, int2 = raw_forward(kw)
    for k in ["color", "depth", "alpha", "semantic"]:
        assert torch.equal(res[k], res2[k])
    assert torch.equal(internal("n_contrib"), int2("n_contrib"))
    # gradient sanity: finite, zero for culled Gaussians, colour-gradient checksum
    wts = syn.loss_weights(cam, S=S)
    g = raw_backward(kw, res, wts)
    radii = npy(res["radii"])
    for k, v in g.items():
        assert torch.isfinite(v).all(), k
        assert float(v[torch.from_numpy(radii == 0).cuda()].abs().sum()) == 0.0, k
    # sum_g dL/drgb_g = sum_pix dL/dC_pix * (sum_i w_i) = sum over pixels of dL_dC * alpha  (checksum of checksums)
    lhs = npy(g["colors"]).astype(np.float64).sum(0)
    rhs = (wts["color"].numpy().astype(np.float64) * a.astype(np.float64)).sum((1, 2))
    assert np.abs(lhs - rhs).max() <= 1e-3 * np.abs(rhs).max() + 1e-2
    # ... and so are the tile rects (the reference's 3-sigma squares against the ones cut down to where alpha >= 1/255 is
    # possible): the same images bit for bit, the same gradients, from three quarters of the instances
    with switches(_C.REF_RECT):
        res3, _ = raw_forward(kw)
        g3 = raw_backward(kw, res3, wts)
    assert int(internal("num_rendered_reference")[0]) == res3["R"] and R < 0.8 * res3["R"]
    for k in ["color", "depth", "alpha", "semantic"]:
        assert torch.equal(res[k], res3[k]), k
    from gpu_utils import conditioned_allowance
    for k in g:  # (the row sum groups its additions by row number: equal up to fp32 rounding; dL/dcov3D / dL/dscale / dL/drot
        # amplify a last-bit difference of dL/dconic for a handful of elongated splats per million -- gpu_utils.CONDITIONED)
        n = g[k].numel()
        grad_close(npy(g[k]), npy(g3[k]), rel=1e-4, abs_frac=2e-5, name=f"tile rects, full size:{k}",
                   max_outlier_frac=(conditioned_allowance(k, n) / n) if n else 0.0)


def test_pybind_and_ctypes_bindings_agree():
    """The pybind `_C` module (csrc/ext.cpp, torch.utils.cpp_extension) and the ctypes binding drive the same C ABI:
    bit-identical outputs, the reference's error behaviour on both."""
    from street_gaussians_amd._native import SgrError
    cam, sc, kw = _kw("mid_20k_sem3")
    wts = syn.loss_weights(cam, S=3)
    prev = _C.binding()
    out = {}
    try:
        for b in ("ctypes", "pybind"):
            _C.set_binding(b)
            assert _C.binding() == b
            res, _ = raw_forward(kw)
            g = raw_backward(kw, res, wts)
            out[b] = (res, g)
            with pytest.raises(SgrError, match=r"\[0, 32\]"):
                bad = dict(kw, semantics=torch.zeros(sc.P, 40))
                raw_forward(bad)
            with pytest.raises(SgrError, match="no CPU path"):
                _C.distCUDA2(torch.rand(10, 3))
            assert torch.equal(_C.mark_visible(dev(sc.means3D), dev(cam.viewmatrix), dev(cam.projmatrix)),
                               torch.from_numpy(oracle.mark_visible(sc.means3D, cam.viewmatrix, cam.projmatrix)).cuda())
    finally:
        _C.set_binding(prev)
    for k in ["color", "depth", "alpha", "semantic", "radii"]:
        assert torch.equal(out["ctypes"][0][k], out["pybind"][0][k]), k
    assert out["ctypes"][0]["R"] == out["pybind"][0]["R"]
    for k in out["ctypes"][1]:
        assert torch.equal(out["ctypes"][1][k], out["pybind"][1][k]), k


def test_degenerate_inputs():
    """Edge cases of the boundary: nothing visible (every Gaussian behind the camera: R = 0, zero images, zero
    gradients, backward still legal), a 1x1 image, the maximum number of semantic channels (32), and an image wider
    than the packed tile rect allows (an error, not a crash)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from street_gaussians_amd._native import SgrError
    cam, sc, kw = _kw("tiny_sh3_sem2")
    # (1) everything behind the camera
    behind = dict(kw, means3D=sc.means3D * torch.tensor([1.0, 1.0, -1.0]))
    res, internal = raw_forward(behind)
    assert res["R"] == 0 and int(res["radii"].abs().sum()) == 0
    bg = npy(dev(kw["bg"]))
    assert np.array_equal(npy(res["color"]), np.broadcast_to(bg[:, None, None], res["color"].shape))
    assert float(res["alpha"].abs().max()) == 0.0 and float(res["depth"].abs().max()) == 0.0
    wts = syn.loss_weights(cam, S=2)
    g = raw_backward(behind, res, wts)
    for k, v in g.items():
        assert float(v.abs().max()) == 0.0, k
    # (2) a 1x1 image against the oracle
    cam1 = syn.make_camera(1, 1, fx=1.0)
    sc1 = syn.make_scene(50, cam1, S=0, seed=2, scale_px=0.3, zmin=1.0, zmax=3.0, margin=0.3)
    kw1 = oracle_kwargs(cam1, sc1)
    fw1 = oracle.forward(**kw1)
    res1, int1 = raw_forward(kw1)
    assert res1["R"] == fw1.num_rendered and (npy(res1["radii"]) == fw1.radii).all()
    image_close(npy(res1["color"]), fw1.color, name="1x1 color", max_outliers=0)
    # (3) 32 semantic channels (the oracle follows the reference's limit of 20, so: linearity in the channels)
    cam2 = syn.make_camera(96, 64, fx=100.0)
    sc2 = syn.make_scene(400, cam2, S=32, seed=4, scale_px=0.02)
    t = {k: dev(getattr(sc2, k)) for k in ["means3D", "scales", "rotations", "opacities", "shs", "semantics"]}
    rast = GaussianRasterizer(settings(cam2))
    full = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                semantics=t["semantics"])
    part = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                semantics=t["semantics"][:, 7:20].contiguous())
    assert full[4].shape == (32, 64, 96)
    assert torch.allclose(full[4][7:20], part[4], rtol=1e-6, atol=1e-7) and torch.equal(full[0], part[0])
    sem = t["semantics"].clone().requires_grad_(True)
    out = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"], semantics=sem)
    out[4].sum().backward()
    assert torch.isfinite(sem.grad).all() and float(sem.grad.abs().max()) > 0
    assert torch.allclose(sem.grad, sem.grad[:, :1].expand_as(sem.grad), rtol=1e-5, atol=1e-7)  # dL/dsem = sum_pix alpha*T
    # (4) an image the 10-bit packed tile rect cannot address
    big = settings(cam)._replace(image_width=16400, image_height=8)
    with pytest.raises(SgrError, match="not supported"):
        GaussianRasterizer(big)(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])


SWITCH_ENV_NAMES = ("SGR_NO_CULL", "SGR_NO_DPP", "SGR_NO_DET", "SGR_NO_HITS", "SGR_V2", "SGR_ONESWEEP", "SGR_PRE_STAGE", "SGR_EXACT",
                    "SGR_SW", "SGR_SW8", "SGR_RS_WAVE", "SGR_SW9", "SGR_REF_RECT", "SGR_NO_TILE_MASK", "SGR_TILE_SORT",
                    "SGR_REF_RECT_PLAIN", "SGR_LPT", "SGR_NO_LPT", "SGR_NO_HLIST", "SGR_HLIST_ALWAYS", "SGR_KEY32")

_ENV_CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from gpu_utils import npy, raw_forward
from helpers import oracle_kwargs, small_case
from street_gaussians_amd import _C
cam, sc = small_case(P=80, S=2)
kw = oracle_kwargs(cam, sc, deg=3, bg=torch.tensor([0.3, 0.1, 0.7]))
res, internal = raw_forward(kw)
torch.cuda.synchronize()
np.savez(sys.argv[2], mask=_C.test_switches(-1), R=res["R"], point_list=npy(internal("point_list")),
         ranges=npy(internal("ranges")), **{k: npy(res[k]) for k in ("color", "depth", "alpha", "semantic", "radii")})
"""


def test_strict_environment_names_in_a_fresh_process(tmp_path):
    """SGR_EXACT=1 SGR_REF_RECT=1 is what users are told to export.  The library reads the names once per
    process, as the initial switch mask, so only a fresh process exercises that path: a child started with the two names
    renders tiny_sh3_sem2 and must give, bit for bit, what this process gives under switches(EXACT | REF_RECT)."""
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in SWITCH_ENV_NAMES}
    env.update(SGR_EXACT="1", SGR_REF_RECT="1")
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", _ENV_CHILD, HERE, out], cwd=root, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert int(got["mask"]) == _C.EXACT | _C.REF_RECT
    cam, sc, kw = _kw("tiny_sh3_sem2")
    with switches(_C.EXACT | _C.REF_RECT):
        res, internal = raw_forward(kw)
        torch.cuda.synchronize()
        assert int(got["R"]) == res["R"] == int(internal("num_rendered_reference")[0]) > 0
        assert np.array_equal(got["point_list"], npy(internal("point_list")))
        assert np.array_equal(got["ranges"], npy(internal("ranges")))
    for k in ("color", "depth", "alpha", "semantic", "radii"):
        assert np.array_equal(got[k], npy(res[k])), f"{k}: the environment's strict mode differs from the switch's"


def test_degenerate_inputs_strict():
    """Parts (1) to (3) of test_degenerate_inputs in the strictly conforming configuration: R = 0 with a legal all-zero
    backward (an empty marked list, an empty compact list), the 1x1 image against the C oracle, 32-channel linearity."""
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc, kw = _kw("tiny_sh3_sem2")
    strict = _C.test_switches(-1) | _C.EXACT | _C.REF_RECT
    # (1) everything behind the camera
    behind = dict(kw, means3D=sc.means3D * torch.tensor([1.0, 1.0, -1.0]))
    wts = syn.loss_weights(cam, S=2)
    fw = oracle.forward(**behind)
    assert fw.num_rendered == 0
    res, g, _ = strict_mode_against_reference(behind, wts, 2, "behind the camera", rf=fw)
    fw.free()
    assert res["R"] == 0 and int(res["radii"].abs().sum()) == 0
    bg = npy(dev(kw["bg"]))
    assert np.array_equal(npy(res["color"]), np.broadcast_to(bg[:, None, None], res["color"].shape))
    assert float(res["alpha"].abs().max()) == 0.0 and float(res["depth"].abs().max()) == 0.0
    for k, v in g.items():
        assert float(v.abs().max()) == 0.0, k
    # (2) a 1x1 image against the oracle
    cam1 = syn.make_camera(1, 1, fx=1.0)
    sc1 = syn.make_scene(50, cam1, S=0, seed=2, scale_px=0.3, zmin=1.0, zmax=3.0, margin=0.3)
    kw1 = oracle_kwargs(cam1, sc1)
    fw1 = oracle.forward(**kw1)
    res1, _, _ = strict_mode_against_reference(kw1, syn.loss_weights(cam1, S=0), 0, "1x1", rf=fw1)
    assert res1["R"] == fw1.num_rendered and (npy(res1["radii"]) == fw1.radii).all()
    image_close(npy(res1["color"]), fw1.color, name="1x1 color, strict", max_outliers=0)
    fw1.free()
    # (3) 32 semantic channels: linearity in the channels
    cam2 = syn.make_camera(96, 64, fx=100.0)
    sc2 = syn.make_scene(400, cam2, S=32, seed=4, scale_px=0.02)
    t = {k: dev(getattr(sc2, k)) for k in ["means3D", "scales", "rotations", "opacities", "shs", "semantics"]}
    rast = GaussianRasterizer(settings(cam2))
    with switches(strict):
        full = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                    semantics=t["semantics"])
        part = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                    semantics=t["semantics"][:, 7:20].contiguous())
        assert full[4].shape == (32, 64, 96)
        assert torch.allclose(full[4][7:20], part[4], rtol=1e-6, atol=1e-7) and torch.equal(full[0], part[0])
        sem = t["semantics"].clone().requires_grad_(True)
        out = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"], semantics=sem)
        out[4].sum().backward()
        torch.cuda.synchronize()
    assert torch.isfinite(sem.grad).all() and float(sem.grad.abs().max()) > 0
    assert torch.allclose(sem.grad, sem.grad[:, :1].expand_as(sem.grad), rtol=1e-5, atol=1e-7)  # dL/dsem = sum_pix alpha*T


@pytest.mark.parametrize("S", [0, 3, 19])
def test_exact_parity_mode_is_bit_faithful_to_the_reference_kernels(S):
    """sgr_test_switches bit 7 / SGR_EXACT=1: the blend kernels evaluate the reference's own power expression without
    contraction, the library's accurate expf and a true division for the T recovery.  Against oracle/_ref's strict build
    (the reference's untouched kernels, -ffp-contract=off, the same device expf) alpha_out, depth and the semantic image
    are then BIT-IDENTICAL, n_contrib is identical, and -- T_final = 1 - alpha_out carrying no forward rounding into the
    backward -- the gradients meet the north-star gate (rel 1e-4) END TO END, each side on its own forward.  (The C oracle
    uses the host's libm expf, which differs from the device's in rare last bits: it is compared with a few-ulp gate.)"""
    ref = _ref()
    cam = syn.make_camera(320, 208, fx=340.0, yaw_deg=2.0)
    sc = syn.make_scene(15000, cam, S=S, seed=21, scale_px=0.004)
    kw = oracle_kwargs(cam, sc, bg=torch.tensor([0.3, 0.1, 0.2]))
    exact_mode_bit_faithful(ref, oracle, kw, syn.loss_weights(cam, S=S), S)
