"""CPU pin of two hot-path NUMBERS to the reference's own Python (tests/golden/make_hotpath_fixture.py): SH -> RGB as
``eval_sh`` + ``clamp_min(x + 0.5, 0)`` gives it, cov3D as ``strip_symmetric(L @ L^T)`` with ``L = build_scaling_rotation(mod * s,
r)`` gives it, each evaluated in float32 and in float64 and committed as data (tests/golden/hotpath/pins.npz).  Here: (a) where
/root/reference exists the fixture is regenerated from its source and must reproduce the committed file bit for bit, (b) the
fixture's own figures (e_ref, the clamp-exempt share) are recomputed from its arrays, (c) the C oracle's rgb / clamped / cov3D
are held to the float64 outputs within 4 * e_ref of each Gaussian's own scale.  tests/test_gpu_hotpath_pins.py holds the HIP
forward to the same gate."""
import os

import numpy as np
import pytest

from golden import make_hotpath_fixture as hp
from oracle import oracle


@pytest.fixture(scope="module")
def pins():
    assert os.path.exists(hp.OUT), "tests/golden/hotpath/pins.npz is not committed"
    return hp.load()


@pytest.mark.skipif(not os.path.exists("/root/reference/lib/utils/sh_utils.py"),
                    reason="reference checkout not present on this machine")
def test_regenerating_from_the_reference_source_reproduces_the_fixture(pins):
    d = hp.build()
    assert sorted(d) == sorted(pins)
    for k in d:
        a, b = np.asarray(d[k]), pins[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k


def test_fixture_holds_what_it_says(pins):
    d = pins
    P = d["shs"].shape[0]
    assert P == hp.P <= 4096 and os.path.getsize(hp.OUT) < 1 << 20
    assert d["rgb32"].dtype == d["cov32"].dtype == np.float32 and d["rgb64"].dtype == d["cov64"].dtype == np.float64
    assert sorted(set(d["degree"].tolist())) == [0, 1, 2, 3]
    # e_ref is what the arrays give
    for t, name in (("rgb", "e_ref_sh"), ("cov", "e_ref_cov")):
        sc = hp.row_scale(d[t + "64"])
        err = np.abs(d[t + "32"].astype(np.float64) - d[t + "64"])
        assert float((err / np.where(sc > 0, sc, 1.0)).max()) == float(d[name])
        assert 0 < float(d[name]) < 2e-6  # a few float32 ulps: anything larger means an input cancels and hides the rest
        assert hp.gate(d[t + "32"], d[t + "64"], float(d[name]))[0]
    # the edges the inputs are there for
    assert ((d["pre64"] < 0).any(axis=1)).mean() > 0.1 and (d["pre64"] < 0).all(axis=1).any() and (d["rgb64"] >= 0).all()
    n = d["dirs"] / np.linalg.norm(d["dirs"], axis=1, keepdims=True)
    for deg in range(4):  # +-x, +-y, +-z in every degree group
        m = d["degree"] == deg
        assert len({tuple(r) for r in np.round(n[m][(np.abs(n[m]) == 1).any(axis=1)]).astype(int).tolist()}) == 6
    assert d["scales"].min() <= 1e-3 and d["scales"].max() >= 1e2
    assert (d["scales"].max(axis=1) / d["scales"].min(axis=1)).max() >= 1e4
    assert np.abs(np.linalg.norm(d["rotations"].astype(np.float64), axis=1) - 1).max() < 1e-7
    assert (np.abs(d["rotations"][:, 0]) < 1e-5).sum() >= 16  # rotations by (almost) 180 degrees
    # clamp flags: the share of rows the gate cannot pin is capped, and the reference's own float32 flags sit inside it
    ex = hp.clamp_exempt(d)
    assert 0 < ex.any(axis=1).mean() <= hp.CLAMP_EXEMPT_CAP
    assert not (((d["rgb32"] == 0) != (d["pre64"] < 0)) & ~ex).any()


@pytest.mark.parametrize("group", range(4))
def test_oracle_rgb_clamped_cov3D_against_the_reference_python(pins, group):
    rows, kw = hp.group_kwargs(pins, group)
    fw = oracle.forward(**kw, internals=True)
    assert (fw.radii > 0).all(), "a pinned Gaussian is culled: its rgb / cov3D would not be computed"
    ok, need = hp.gate(fw.rgb, pins["rgb64"][rows], float(pins["e_ref_sh"]))
    print(f"oracle rgb, group {group}: needs factor {need:.2f} of e_ref (gate {hp.FACTOR})")
    assert ok, need
    ok, need = hp.gate(fw.cov3D, pins["cov64"][rows], float(pins["e_ref_cov"]))
    print(f"oracle cov3D, group {group}: needs factor {need:.2f} of e_ref (gate {hp.FACTOR})")
    assert ok, need
    assert hp.clamp_flags_agree(fw.clamped, pins, rows) == 0
    fw.free()
