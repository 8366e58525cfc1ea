"""Pins two hot-path NUMBERS to the reference's own Python and writes them to tests/golden/hotpath/pins.npz:

  * SH -> RGB: ``eval_sh`` (/root/reference/lib/utils/sh_utils.py) followed by ``clamp_min(x + 0.5, 0)`` on directions
    normalised as ``dir_pp / dir_pp.norm(dim=1, keepdim=True)`` -- what StreetGaussianRenderer.render_kernel does with
    ``convert_SHs_python`` (lib/models/street_gaussian_renderer.py:192-197);
  * cov3D: ``strip_symmetric(L @ L^T)`` with ``L = build_scaling_rotation(mod * s, r)`` (lib/utils/general_utils.py, with
    ``quaternion_to_matrix`` and ``strip_lowerdiag`` behind them) -- what ``get_covariance`` hands on with
    ``compute_cov3D_python``.

The functions are cut out of the reference's files when this runs and executed here (no GPU); nothing of their text is kept.
The only textual changes are ``.cuda()`` / ``device="cuda"`` (there is no GPU here) and ``dtype=torch.float`` ->
``dtype=torch.get_default_dtype()``, so that the same text also runs in float64.  Each output is evaluated twice, in float32
(what the reference computes) and in float64 on the same float32 inputs (the truth both float32 evaluations -- the reference's
and the kernels' -- are held against).  Run where /root/reference exists:

    python tests/golden/make_hotpath_fixture.py

The file holds data only.  Inputs (P rows, row i belongs to group i % 4, which fixes its SH degree and scale modifier because a
forward takes one of each): ``shs`` [P,16,3], ``dirs`` [P,3] (NOT normalised; every component a multiple of 2^-20 so that
``centre + dirs`` and ``means3D - campos`` are exact in float32), ``degree`` [P], ``scales`` [P,3], ``rotations`` [P,4]
(normalised, the form get_rotation hands on: the kernels do not normalise), ``scale_modifier`` [P].  Outputs: ``rgb32`` /
``rgb64`` [P,3], ``pre64`` [P,3] (the float64 value before the clamp), ``cov32`` / ``cov64`` [P,6], and ``e_ref_sh`` /
``e_ref_cov``: max |ref_f32 - ref_f64| / scale per tensor, scale = the largest |ref_f64| entry of the Gaussian's own row.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden import make_callsite_fixture as mk  # noqa: E402

OUT = os.path.join(HERE, "hotpath", "pins.npz")
REF = mk.REF
P = 2048
GROUP_DEGREE = (0, 1, 2, 3)
GROUP_MODIFIER = (1.0, 0.6, 1.5, 1.0)
CENTRE = (0.0, 0.0, 8.0)  # means3D = CENTRE + dirs, campos = CENTRE: every Gaussian in front of an identity-view camera
FACTOR = 4.0  # the gate is FACTOR * e_ref * scale: a different association of up to 16 products per channel / 9 per entry
CLAMP_EXEMPT_CAP = 0.01


def reference_functions():
    """-> (eval_sh, build_scaling_rotation, strip_symmetric), executed from the reference's source."""
    shu = {}
    exec(mk._nocuda(open(os.path.join(REF, "lib/utils/sh_utils.py")).read()), shu)
    ns = {"torch": torch, "np": np}
    gu = os.path.join(REF, "lib/utils/general_utils.py")
    for name in ("quaternion_to_matrix", "strip_lowerdiag", "strip_symmetric", "build_scaling_rotation"):
        exec(mk._func(gu, name).replace("dtype=torch.float,", "dtype=torch.get_default_dtype(),"), ns)
    return shu["eval_sh"], ns["build_scaling_rotation"], ns["strip_symmetric"]


def make_inputs():
    """Seeded inputs made of draws and exactly rounded operations only (no libm), so they are the same everywhere."""
    rng = np.random.default_rng(20240611)
    q20 = lambda a: np.round(a * 2.0 ** 20) / 2.0 ** 20
    # ---- directions: random, along the axes, a hair off the axes; lengths 0.25 .. 1
    d = rng.standard_normal((P, 3))
    d = d / np.sqrt((d * d).sum(1, keepdims=True)) * rng.uniform(0.25, 1.0, (P, 1))
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    for k in range(48):  # (row 64 + k is in group k % 4) every axis in every degree group, at two lengths
        d[64 + k] = axes[(k // 4) % 6] * (0.5, 1.0)[k // 24]
    for k in range(48):
        d[128 + k] = axes[(k // 4) % 6] * 0.5 + rng.uniform(-1, 1, 3) * 2.0 ** -(10 + k % 9)
    dirs = q20(d).astype(np.float32)
    assert (np.abs(dirs).max(1) > 0).all()
    # ---- SH coefficients: DC offset so colours sit in range, higher bands damped; every 8th row pushed far below the clamp
    # in one, two or three channels (a row with all three clamped has scale 0: its zeros must be exact)
    shs = 0.3 * rng.standard_normal((P, 16, 3))
    shs[:, 1:] *= 0.5
    shs[:, 0] += 0.5
    low = np.arange(P) % 8 == 5
    shs[low, 0, 0] -= 6.0
    shs[low & (np.arange(P) % 16 == 5), 0, 1] -= 6.0
    shs[low & (np.arange(P) % 32 == 5), 0, 2] -= 6.0
    shs = shs.astype(np.float32)
    # ... and 16 degree-0 rows whose first channel sits ON the threshold (C0 * sh + 0.5 = 0 up to the rounding of sh): the
    # rows whose clamp flag the gate cannot pin, 0.8 % of all
    shs[np.arange(P) % 128 == 0, 0, 0] = np.float32(-0.5 / 0.28209479177387814)
    # ---- scales: mantissa * 2^e per axis, e in [-10, 6]: 1e-3 .. 1.3e2, independent per axis (anisotropy up to 1e5)
    scales = np.ldexp(rng.uniform(1.0, 2.0, (P, 3)), rng.integers(-10, 7, (P, 3))).astype(np.float32)
    scales[0] = (2.0 ** -10, 1.0, 127.0)
    scales[1] = (127.0, 2.0 ** -10, 2.0 ** -10)
    # ---- rotations (w, x, y, z): random; identity; half turns about the axes; w -> 0 (rotations by almost 180 degrees)
    q = rng.standard_normal((P, 4))
    q[256] = (1, 0, 0, 0)
    q[257:260] = np.eye(4)[1:]
    near = np.arange(P) % 8 == 3
    q[near, 0] = rng.choice([-1.0, 1.0], near.sum()) * np.ldexp(1.0, -rng.integers(3, 24, near.sum()))
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    rotations = q.astype(np.float32)
    group = np.arange(P) % 4
    return dict(shs=shs, dirs=dirs, degree=np.asarray(GROUP_DEGREE, np.int32)[group], scales=scales, rotations=rotations,
                scale_modifier=np.asarray(GROUP_MODIFIER, np.float32)[group])


def row_scale(ref64):
    return np.abs(ref64).max(axis=1, keepdims=True)


def evaluate(inp):
    """The reference's functions on the inputs, in float32 and in float64 -> dict of outputs."""
    eval_sh, build_scaling_rotation, strip_symmetric = reference_functions()
    out = {}
    prev = torch.get_default_dtype()
    try:
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            torch.set_default_dtype(dt)
            shs, dirs = torch.from_numpy(inp["shs"]).to(dt), torch.from_numpy(inp["dirs"]).to(dt)
            s, r = torch.from_numpy(inp["scales"]).to(dt), torch.from_numpy(inp["rotations"]).to(dt)
            mod = torch.from_numpy(inp["scale_modifier"]).to(dt)[:, None]
            pre = torch.zeros(P, 3, dtype=dt)
            for deg in sorted(set(GROUP_DEGREE)):
                m = torch.from_numpy(inp["degree"] == deg)
                dn = dirs[m] / dirs[m].norm(dim=1, keepdim=True)  # street_gaussian_renderer.py:195
                pre[m] = eval_sh(deg, shs[m].transpose(1, 2), dn) + 0.5
            out["rgb" + tag] = torch.clamp_min(pre, 0.0).numpy()
            if tag == "64":
                out["pre64"] = pre.numpy()
            L = build_scaling_rotation(mod * s, r)
            cov = strip_symmetric(L @ L.transpose(1, 2))
            assert cov.dtype == dt
            out["cov" + tag] = cov.numpy()
    finally:
        torch.set_default_dtype(prev)
    assert out["rgb32"].dtype == np.float32 and out["cov32"].dtype == np.float32 and out["rgb64"].dtype == np.float64
    for t, name in (("rgb", "e_ref_sh"), ("cov", "e_ref_cov")):
        sc = row_scale(out[t + "64"])
        err = np.abs(out[t + "32"].astype(np.float64) - out[t + "64"])
        assert (err[(sc == 0).reshape(-1)] == 0).all()
        out[name] = np.float64((err / np.where(sc > 0, sc, 1.0)).max())
    return out


def clamp_exempt(inp_out):
    """Rows x channels whose clamp flag is not pinned: |pre64| within the gate of the clamp threshold."""
    bound = FACTOR * float(inp_out["e_ref_sh"]) * row_scale(inp_out["rgb64"])
    return np.abs(inp_out["pre64"]) <= bound


def build():
    inp = make_inputs()
    out = evaluate(inp)
    d = dict(inp, **out)
    # the inputs must exercise what they are there for, and the reference's own float32 flags must sit inside the cap
    assert (d["pre64"] < 0).any(axis=1).mean() > 0.1 and (d["pre64"] < 0).all(axis=1).any()
    ex = clamp_exempt(d)
    own = ((d["rgb32"] == 0) != (d["pre64"] < 0)) & ~ex
    assert ex.any(axis=1).mean() <= CLAMP_EXEMPT_CAP and not own.any(), (ex.mean(), own.sum())
    assert d["scales"].min() <= 1e-3 and d["scales"].max() >= 1e2
    return d


def load(path=OUT):
    return dict(np.load(path))


def group_kwargs(d, group):
    """The rows of one group as a forward call (oracle-style keyword dict, tests/helpers.oracle_kwargs) -> (rows, kw): an
    identity-view camera at the origin looking down +z at a 64 x 64 image, means3D = CENTRE + dirs (all in front of it and
    on screen), campos = CENTRE so that means3D - campos is `dirs` exactly."""
    from street_gaussians_amd import synthetic as syn
    rows = np.nonzero(np.arange(d["shs"].shape[0]) % 4 == group)[0]
    cam = syn.make_camera(64, 64, fx=64.0)
    assert torch.equal(cam.viewmatrix, torch.eye(4))
    c = torch.tensor(CENTRE, dtype=torch.float32)
    t = lambda k: torch.from_numpy(d[k][rows].copy())
    means = c + t("dirs")
    assert torch.equal(means - c, t("dirs"))
    kw = dict(means3D=means, opacities=torch.full((rows.size, 1), 0.5), viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix,
              campos=c, bg=torch.zeros(3), tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, image_height=64, image_width=64,
              sh_degree=int(GROUP_DEGREE[group]), scale_modifier=float(np.float32(GROUP_MODIFIER[group])), shs=t("shs"),
              scales=t("scales"), rotations=t("rotations"))
    return rows, kw


def gate(x, ref64, e_ref):
    """|x - ref_f64| <= FACTOR * e_ref * scale, scale = the largest |ref_f64| entry of the Gaussian's own row.
    -> (every element inside, the worst |x - ref_f64| / (e_ref * scale): the factor this x would need)."""
    sc = row_scale(ref64)
    err = np.abs(np.asarray(x, np.float64) - ref64)
    ok = err <= FACTOR * e_ref * sc
    need = (err / np.where(sc > 0, e_ref * sc, 1.0))[(sc > 0).reshape(-1)].max()
    return bool(ok.all()), float(need)


def clamp_flags_agree(clamped, d, rows):
    """The forward's clamp flags against the float64 sign wherever the gate can pin them -> number of disagreements."""
    sub = {k: d[k][rows] for k in ("pre64", "rgb64")}
    sub["e_ref_sh"] = d["e_ref_sh"]
    ex = clamp_exempt(sub)
    return int(((np.asarray(clamped).astype(bool) != (sub["pre64"] < 0)) & ~ex).sum())


if __name__ == "__main__":
    d = build()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes; e_ref_sh", d["e_ref_sh"], "e_ref_cov", d["e_ref_cov"],
          "clamp-exempt rows", int(clamp_exempt(d).any(axis=1).sum()))
