"""`-m gpu`: the HIP forward's rgb (export 5), clamp flags (export 1) and cov3D (export 3, sgr_export_cov3d) against the
reference's own Python -- ``eval_sh`` + ``clamp_min(x + 0.5, 0)`` and ``strip_symmetric(L @ L^T)`` with
``L = build_scaling_rotation(mod * s, r)``, committed as data in tests/golden/hotpath/pins.npz
(tests/golden/make_hotpath_fixture.py; tests/test_hotpath_pins_cpu.py pins the file and holds the C oracle to it).

The kernel and the reference's float32 Python are two float32 evaluations of one polynomial in different orders; the truth
is the file's float64 evaluation.  Gate: |x - ref_f64| <= 4 * e_ref * scale with scale = the largest |ref_f64| entry of the
Gaussian's OWN row and e_ref = the reference's own float32-vs-float64 error in those units (stored in the file).  The factor
the HIP path actually needs is printed and appended to the suite's parity log.  Default, parity and strict mode."""
import numpy as np
import pytest
import torch

from golden import make_hotpath_fixture as hp
from gpu_utils import _log, image_close, npy, raw_forward, switches
from oracle import oracle
from street_gaussians_amd import _C

pytestmark = pytest.mark.gpu

MODES = {"default": 0, "exact": _C.EXACT, "strict": _C.EXACT | _C.REF_RECT}


@pytest.fixture(scope="module")
def pins():
    return hp.load()


@pytest.mark.parametrize("mode", list(MODES))
def test_rgb_clamped_cov3D_against_the_reference_python(pins, mode):
    for group in range(4):
        rows, kw = hp.group_kwargs(pins, group)
        with switches(_C.test_switches(-1) | MODES[mode]):
            res, internal = raw_forward(kw)
            rgb, clamped, cov = npy(internal("rgb")), npy(internal("clamped")), npy(internal("cov3D"))
        assert (npy(res["radii"]) > 0).all(), "a pinned Gaussian is culled: its rgb would not be computed"
        ok_c, need_c = hp.gate(rgb, pins["rgb64"][rows], float(pins["e_ref_sh"]))
        ok_v, need_v = hp.gate(cov, pins["cov64"][rows], float(pins["e_ref_cov"]))
        bad_flags = hp.clamp_flags_agree(clamped, pins, rows)
        print(f"{mode}, group {group} (degree {hp.GROUP_DEGREE[group]}, modifier {hp.GROUP_MODIFIER[group]}): rgb needs "
              f"{need_c:.2f} x e_ref, cov3D needs {need_v:.2f} x e_ref (gate {hp.FACTOR}); clamp flags off: {bad_flags}")
        _log(dict(kind="hotpath_pin", mode=mode, group=group, rgb_factor_needed=need_c, cov3D_factor_needed=need_v,
                  gate=hp.FACTOR, e_ref_sh=float(pins["e_ref_sh"]), e_ref_cov=float(pins["e_ref_cov"]), clamp_flags_off=bad_flags))
        assert ok_c, (mode, group, need_c)
        assert ok_v, (mode, group, need_v)
        assert bad_flags == 0, (mode, group)


@pytest.mark.parametrize("mode", list(MODES))
def test_the_reference_python_cov3D_as_cov3D_precomp(pins, mode):
    """The file's float32 cov3D fed as ``cov3D_precomp`` (what the reference does with ``compute_cov3D_python``) against
    the ``scales`` + ``rotations`` run of the same Gaussians.

    Where the library's own cov3D equals the file's bit for bit (about four rows in five) the two runs are the same
    function of the same numbers: conic_opacity and radii must be bit-identical, row by row.

    For the other rows the two inputs differ within the cov3D gate (by a last bit, typically), and what that does to
    conic_opacity is a property of the reference's algorithm, not of a kernel: the conic is the inverse of the 2x2
    covariance, whose condition number reaches 1e6 for the needles this file holds (scales over five decades), so a
    relative 1e-7 of the row's scale going in comes out as up to 8e-2 of the row's scale -- measured on the CPU with the C
    oracle alone, its `scales` run against its `cov3D_precomp` run.  No tolerance on conic_opacity derived from the input
    gate can therefore hold.  What is required instead is tighter than any: on EACH of the two inputs the HIP forward's
    conic_opacity and radii equal the C oracle's (the reference's preprocess restated line by line) bit for bit, so that the
    difference between the two HIP runs is the reference's own, to the bit; and each run's images are held to the oracle's
    on the same input by the bound of test_forward_matches_oracle."""
    equal_rows = total = 0
    for group in range(4):
        rows, kw = hp.group_kwargs(pins, group)
        kb = {k: v for k, v in kw.items() if k not in ("scales", "rotations")}
        kb["cov3D_precomp"] = torch.from_numpy(pins["cov32"][rows].copy())
        fa, fb = oracle.forward(**kw), oracle.forward(**kb)
        with switches(_C.test_switches(-1) | MODES[mode]):
            ra, ia = raw_forward(kw)
            rb, ib = raw_forward(kb)
            cov = npy(ia("cov3D"))
            ca, cb = npy(ia("conic_opacity")), npy(ib("conic_opacity"))
        same = (cov == pins["cov32"][rows]).all(axis=1)
        equal_rows += int(same.sum())
        total += rows.size
        assert np.array_equal(ca[same], cb[same]), (mode, group, "conic_opacity differs on bit-identical cov3D")
        assert np.array_equal(npy(ra["radii"])[same], npy(rb["radii"])[same]), (mode, group)
        for tag, r, c, f in (("scales", ra, ca, fa), ("precomp", rb, cb, fb)):
            assert np.array_equal(npy(r["radii"]), f.radii), (mode, group, tag)
            assert np.array_equal(c, f.conic_opacity), (mode, group, tag)
            assert int(ia("num_rendered_reference")[0]) == fa.num_rendered and int(ib("num_rendered_reference")[0]) == fb.num_rendered
            for k in ("color", "depth", "alpha"):
                image_close(npy(r[k]), getattr(f, k), name=f"hotpath {tag} {mode} g{group}: {k}")
        fa.free()
        fb.free()
    print(f"{mode}: cov3D bit-identical to the reference's float32 Python on {equal_rows} of {total} rows")
    _log(dict(kind="hotpath_cov_equal_rows", mode=mode, equal=equal_rows, total=total))
    assert equal_rows > total // 2
