"""`-m gpu` tests of the row-sum stage of the per-Gaussian backward (csrc/sgr_gauss_bwd.hip, sgr_row_sum_kernel at S = 0):
a lane asks for the flag bytes of its next rows in one go, then for every touched row among them, and Gaussians with more
rows than one such trip loop.  What can go wrong there is a flag or a row paired with the wrong Gaussian or the wrong trip, so
the scene is built around the ROW COUNTS at which the walk changes shape, and around where a Gaussian sits in its quad, pair
and wave:

  * 256 x 256 pixels = 256 tiles; isotropic Gaussians from sub-pixel to image-filling, thin diagonal ones (their rects are
    masked: rows numbered by the rank of the tile in the mask), a few behind the camera (no rows), and an opaque splat in
    front of a part of the image, so that the tiles behind it stop early and many rows stay untouched;
  * the per-Gaussian row counts include 0, 1, 3, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33 and more than 64 -- asserted from the
    exported tile counts (the scene's members were picked from `_pool()` by those counts: the reference rects' with the C
    oracle, the cut-down rects' from an export);
  * P = 1, 2, 7, 8, 9, 31, 33, 65, 129 (prefixes of the scene): every gradient against the C oracle in the three modes;
  * k Gaussians behind the camera in front of the scene, k = 1, 2, 3, 15, 16, 17: every original Gaussian's gradient rows are
    the unshifted run's, byte for byte -- the additions of a Gaussian do not depend on its slot;
  * the statistics sink and masked_color_out against the same quantities computed from the returned gradients."""
import numpy as np
import pytest
import torch

from gpu_utils import (CONDITIONED, GRAD_NAMES, SAME_STATE_GATE, conditioned_allowance, count_outside, image_close, npy, oracle_backward_same_state,
                       raw_backward, raw_forward, restrict_oracle, settings, strict_gate, switches)
from helpers import oracle_kwargs
from jacobian_utils import backward_with
from oracle import oracle
from street_gaussians_amd import _C, scene
from street_gaussians_amd import synthetic as syn

pytestmark = pytest.mark.gpu

W = H = 256
FX = 256.0
COUNTS = (0, 1, 3, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33)
MODES = {"default": lambda: 0, "exact": lambda: _C.EXACT, "strict": lambda: _C.EXACT | _C.REF_RECT}
N_ISO, N_DIAG, N_EDGE = 512, 256, 256


def _camera():
    return syn.make_camera(W, H, fx=FX)


def _place(u, v, z):
    """World position (camera = world here) that projects to pixel (u, v) at depth z."""
    return torch.stack([((u + 0.5) / (0.5 * W) - 1.0) * 0.5 * W / FX * z, ((v + 0.5) / (0.5 * H) - 1.0) * 0.5 * H / FX * z, z], 1)


def _pool():
    """The candidates the scene is picked from, generated from a seed: N_ISO isotropic Gaussians whose sizes sweep 0.3 .. 300
    pixels (sigma), then N_DIAG thin ones (sigma 0.4 .. 1.5 pixels across, 6 .. 150 along) lying at an angle in the image ..."""
    g = torch.Generator().manual_seed(7)
    r = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    n = N_ISO + N_DIAG
    u, v, z = r(n, -10.0, W + 10.0), r(n, -10.0, H + 10.0), r(n, 3.0, 12.0)
    means = _place(u, v, z)
    sig = 0.3 * 1000.0 ** (torch.arange(N_ISO, dtype=torch.float64) / (N_ISO - 1))
    iso = (sig * z[:N_ISO] / FX)[:, None].expand(-1, 3)
    along = 6.0 * 25.0 ** (torch.arange(N_DIAG, dtype=torch.float64) / (N_DIAG - 1))
    across = r(N_DIAG, 0.4, 1.5)
    zd = z[N_ISO:]
    diag = torch.stack([along * zd / FX, across * zd / FX, across * zd / FX], 1)
    ang = torch.deg2rad(r(N_DIAG, 20.0, 160.0))
    q = torch.zeros(n, 4, dtype=torch.float64)
    q[:, 0] = 1.0
    q[N_ISO:, 0], q[N_ISO:, 3] = torch.cos(0.5 * ang), torch.sin(0.5 * ang)
    opac = r(n, 0.02, 0.98)[:, None]
    opac[N_ISO:] = 0.3 + 0.68 * (opac[N_ISO:] - 0.02) / 0.96
    shs = 0.3 * torch.randn(n, 16, 3, generator=g, dtype=torch.float64)
    shs[:, 1:] *= 0.3
    shs[:, 0] += 0.5
    shs[::5, 0] -= 3.0  # (colours the forward clamps at zero)
    # ... and N_EDGE isotropic ones centred outside the image, above it or left of it, by a little less than their 3-sigma
    # radius: their rects are one tile row (or a few columns) thin -- where the counts 5, 13 and 33 of a rect come from
    g2 = torch.Generator().manual_seed(8)
    r2 = lambda m, lo, hi: lo + (hi - lo) * torch.rand(m, generator=g2, dtype=torch.float64)
    above = torch.arange(N_EDGE) % 2 == 0
    rad, other = r2(N_EDGE, 10.0, 120.0), r2(N_EDGE, 0.0, float(W))
    inside = torch.where(above, r2(N_EDGE, 1.0, 15.0), r2(N_EDGE, 1.0, 47.0))  # pixels of the radius that reach into the image
    ue, ve = torch.where(above, other, inside - rad), torch.where(above, inside - rad, other)
    # (the last two by hand, around (120, -86) and (-86, 120): the radius comes out as 96 pixels -- rects of 13 x 1 and 1 x 13 tiles)
    rad[-2:] = 80.0
    ue[-2], ve[-2], ue[-1], ve[-1] = 120.0, -86.0, -86.0, 120.0
    ze = r2(N_EDGE, 3.0, 12.0)
    means = torch.cat([means, _place(ue, ve, ze)])
    edge = (rad / 3.0 * ze / FX)[:, None].expand(-1, 3)
    qe = torch.zeros(N_EDGE, 4, dtype=torch.float64)
    qe[:, 0] = 1.0
    opac = torch.cat([opac, r2(N_EDGE, 0.3, 0.98)[:, None]])
    shs = torch.cat([shs, shs[:N_EDGE].flip(0)])
    n += N_EDGE
    return syn.Scene(means.float().contiguous(), torch.cat([iso, diag, edge]).float().contiguous(),
                     torch.cat([q, qe]).float().contiguous(), opac.float().contiguous(), shs.float().contiguous(), torch.zeros(n, 0))


def _take(sc, idx):
    idx = torch.as_tensor(idx, dtype=torch.long)
    return syn.Scene(*[getattr(sc, k)[idx].contiguous() for k in ("means3D", "scales", "rotations", "opacities", "shs", "semantics")])


def _cat(*parts):
    return syn.Scene(*[torch.cat([getattr(p, k) for p in parts]).contiguous()
                       for k in ("means3D", "scales", "rotations", "opacities", "shs", "semantics")])


def _behind(n, seed=3):
    """n Gaussians behind the camera: culled by the near plane, no rows."""
    g = torch.Generator().manual_seed(seed)
    sc = _take(_pool(), torch.randint(0, N_ISO, (n,), generator=g))
    sc.means3D[:, 2] = -sc.means3D[:, 2]
    return sc


N_OCC, N_BEHIND = 4, 5


def _occluder():
    """An opaque splat nearer than everything else, over the upper left part of the image: N_OCC layers of sigma 150 pixels
    (one layer leaves T = 0.01 at its centre; a pixel is finished below 1e-4), so that inside ~65 pixels of (90, 80) every
    tile ends at the last layer and the rows behind it stay untouched."""
    sc = _take(_pool(), list(range(N_OCC)))
    z = 1.0 + 0.1 * torch.arange(N_OCC, dtype=torch.float64)
    sc.means3D[:] = _place(torch.full((N_OCC,), 90.0, dtype=torch.float64), torch.full((N_OCC,), 80.0, dtype=torch.float64), z).float()
    sc.scales[:] = (150.0 * z / FX).float()[:, None]
    sc.opacities[:] = 0.999
    return sc


# members of _pool(), picked by their tile counts (see the module docstring); the scene is
# [the first member, the occluder's layers, then the others in groups of 15, a Gaussian behind the camera after each of the
# first five groups] = 129
SELECT = [651, 379, 243, 15, 158, 214, 314, 598, 190, 5, 838, 524, 458, 194, 68, 634, 515, 29, 770, 159, 1022, 602, 350, 224,
          807, 328, 347, 702, 955, 16, 120, 558, 844, 406, 202, 881, 569, 992, 713, 172, 276, 566, 380, 510, 231, 250,
          736, 832, 315, 198, 531, 289, 341, 228, 146, 133, 445, 239, 639, 55, 583, 216, 107, 549, 393, 237, 304, 799,
          794, 497, 1023, 623, 432, 309, 471, 594, 302, 240, 42, 640, 552, 617, 820, 630, 7, 365, 321, 43, 532, 263,
          247, 211, 294, 668, 94, 292, 615, 618, 151, 753, 367, 685, 81, 200, 185, 419, 918, 484, 719, 227, 600, 3,
          354, 9, 38, 67, 96, 125, 154, 183]


def _scene():
    pool, back = _pool(), _behind(N_BEHIND)
    # a long thin one first: dL/drotation of an isotropic Gaussian is zero up to rounding, and a tensor of nothing but such
    # zeros has no scale to gate against -- with this one every prefix's tensor has
    parts, b = [_take(pool, SELECT[:1]), _occluder()], 0
    for i in range(1, len(SELECT), 15):
        parts.append(_take(pool, SELECT[i:i + 15]))
        if b < back.P:
            parts.append(_take(back, [b]))
            b += 1
    sc = _cat(*parts)
    assert sc.P == 129, sc.P
    return sc


@pytest.fixture(scope="module")
def full():
    """The scene, its oracle keywords, loss weights and the C oracle's forward (computed once; not modified)."""
    cam = _camera()
    sc = _scene()
    kw = oracle_kwargs(cam, sc, deg=3, semantics=False)
    return cam, sc, kw, syn.loss_weights(cam, S=0)


def _run(kw, wts, mode):
    with switches(_C.test_switches(-1) | MODES[mode]()):
        res, internal = raw_forward(kw)
        g = raw_backward(kw, res, wts)
        torch.cuda.synchronize()
        tt = npy(internal("tiles_touched")).view(np.uint32).copy()
    return res, g, tt, internal


@pytest.mark.parametrize("mode", list(MODES))
def test_row_counts_cover_the_walks_boundaries(full, mode):
    """The scene holds what it is there for, read from the exported tile counts of the mode (= the Gaussians' row counts)."""
    cam, sc, kw, wts = full
    res, g, tt, internal = _run(kw, wts, mode)
    have = set(int(x) for x in tt)
    print(f"{mode}: row counts {sorted(have)}")
    # 17 is a prime above the 16 tiles of a grid row: no rect has it, only a masked rect (the cut-down lists) can
    need = [c for c in COUNTS if not (mode == "strict" and c == 17)]
    missing = [c for c in need if c not in have]
    assert not missing, f"{mode}: no Gaussian with {missing} rows (have {sorted(have)})"
    assert max(have) > 64, sorted(have)
    if mode != "strict":
        rect_word_masked = npy(internal("tile_mask")).view(np.uint64).reshape(-1) != 0
        assert rect_word_masked.any(), "no masked rect in the scene"
    # many rows stay untouched: the tiles behind the opaque splat end before their lists do
    nc = npy(internal("n_contrib")).view(np.uint32).reshape(H, W).astype(np.int64)
    rg = npy(internal("ranges")).view(np.uint32).reshape(-1, 2).astype(np.int64)
    top = nc.reshape(16, 16, 16, 16).max(axis=(1, 3)).reshape(-1)
    length = rg[:, 1] - rg[:, 0]
    untouched = int((length - top).sum())
    print(f"{mode}: {untouched} of {int(length.sum())} rows behind their tile's last contributor")
    assert untouched > 0.1 * length.sum(), (untouched, int(length.sum()))


def _gate(g, fw, res, wts, kw, label):
    """Every gradient tensor against the C oracle's backward on the forward state the library's backward was given, inside
    gpu_utils.strict_gate (rel 1e-4 + 2e-6 of the tensor's scale), with the allowance gpu_utils gives a conditioned tensor: three
    times what the REFERENCE'S OWN two summation orders differ by under the same gate, plus conditioned_allowance's constant for
    the three tensors behind computeCov2DCUDA's cancelling sums, plus SAME_STATE_GATE's share of alpha-threshold flips.

    The splats that fill the image take a term from each of the 65 536 pixels.  The C oracle adds them one after the other in
    float32 by default, and on this scene that sum is itself outside the gate against the same float32 terms added in double
    (oracle.backward: "exact", what it uses at the benchmark's sizes): 3 of the 387 elements of dL/dmeans3D, 33 of 774 of
    dL/dcov3D, 11 of 387 of dL/dscales at P = 129.  The comparison is against the double sum; the two orders' disagreement,
    counted here per tensor, is the reference's own error and sets the allowance.  dL/dmeans2D, dL/dcolour, dL/dopacity and
    dL/dSH -- what the row-sum stage writes or what is linear in it -- show no such disagreement and get no allowance.

    dL/drotation of an ISOTROPIC Gaussian is zero analytically: M = S R, dL/dM = 2 M dL/dSigma, and the quaternion terms are
    differences s * (dL/dM_ij - dL/dM_ji) that cancel for a symmetric dL/dSigma.  What either side computes there is the rounding
    of those terms -- up to 2 s^2 |dL/dSigma| each, a few dozen float32 roundings -- against no scale at all.  Those rows are
    bounded by 1e-5 s^2 max|dL/dcov3D row| and left out of the relative gate."""
    exact = oracle_backward_same_state(oracle, fw, res, wts, 0, parallel="exact")
    seq = oracle_backward_same_state(oracle, fw, res, wts, 0)
    sc = kw["scales"].numpy().astype(np.float64)
    iso = (sc[:, 0] == sc[:, 1]) & (sc[:, 1] == sc[:, 2])
    for k in GRAD_NAMES:
        want = np.asarray(exact[k], np.float64).copy()
        if want.size == 0:
            continue
        got, other = npy(g[k]).astype(np.float64).reshape(want.shape).copy(), np.asarray(seq[k], np.float64).reshape(want.shape).copy()
        if k == "rotations":
            dcov = np.abs(npy(g["cov3D"]).astype(np.float64).reshape(-1, 6)).max(axis=1)
            bound = 1e-5 * sc[:, 0] ** 2 * dcov
            assert (np.abs(got.reshape(-1, 4))[iso] <= bound[iso, None]).all(), f"{label}: dL/drotation of an isotropic Gaussian"
            for t_ in (got, want, other):
                t_.reshape(-1, 4)[iso] = 0.0
        own = count_outside(other.reshape(-1), want.reshape(-1))
        # ... and SAME_STATE_GATE's fraction for single (pixel, Gaussian) alpha-threshold flips (v_exp_f32 against expf), which it
        # caps at 1e-3 of the tensor's scale: held here wherever the oracle agrees with itself
        allow = 3 * own + conditioned_allowance(k, want.size) + int(SAME_STATE_GATE["max_outlier_frac"] * want.size)
        print(f"{label}: {k}: the oracle's two summation orders differ in {own} of {want.size} elements -> {allow} allowed")
        strict_gate(got.reshape(-1), want.reshape(-1), name=f"{label}: {k}", allow=allow)
        if own == 0 and k not in CONDITIONED:
            worst, scale = np.abs(got - want).max(), max(np.abs(want).max(), 1e-30)
            assert worst <= SAME_STATE_GATE["cap"] * scale, f"{label}: {k}: worst error {worst / scale:.3g} of the scale"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("P", [1, 2, 7, 8, 9, 31, 33, 65, 129])
def test_gradients_match_the_oracle(full, P, mode):
    cam, sc, _, wts = full
    kw = oracle_kwargs(cam, _take(sc, range(P)), deg=3, semantics=False)
    fw = oracle.forward(**kw)
    res, g, tt, internal = _run(kw, wts, mode)
    with switches(_C.test_switches(-1) | MODES[mode]()):
        b = restrict_oracle(internal, fw, kw)
    assert res["R"] == b.num_rendered
    assert (npy(res["radii"]) == fw.radii).all()
    assert (tt == b.tiles_touched).all()
    if res["R"]:
        assert (npy(internal("point_list")).view(np.uint32) == b.point_list).all()
    for k in ("color", "depth", "alpha"):
        image_close(npy(res[k]), getattr(fw, k), name=f"row-sum P{P} {mode}: {k}")
    _gate(g, fw, res, wts, kw, f"row-sum P{P} {mode}")
    fw.free()


@pytest.mark.parametrize("mode", list(MODES))
def test_gradients_do_not_depend_on_the_slot(full, mode):
    """k culled Gaussians in front of the scene move every Gaussian to another lane of its quad, another half of a pair and,
    for k >= 15, another wave: its rows are the same rows and are added in the same order, so every gradient row is
    byte-identical."""
    cam, sc, kw, wts = full
    _, g0, tt0, _ = _run(kw, wts, mode)
    for k in (1, 2, 3, 15, 16, 17):
        kw_k = oracle_kwargs(cam, _cat(_behind(k, seed=40 + k), sc), deg=3, semantics=False)
        res, g, tt, _ = _run(kw_k, wts, mode)
        assert (tt[:k] == 0).all() and (tt[k:] == tt0).all(), (mode, k)
        for name in GRAD_NAMES:
            if g0[name] is None or g0[name].numel() == 0:
                continue
            a, b = g[name][k:], g0[name]
            assert a.shape == b.shape, (name, a.shape, b.shape)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                f"{mode}: {name} of {int((a != b).any(dim=tuple(range(1, a.dim()))).sum())} Gaussians changed with {k} in front"
            assert (g[name][:k] == 0).all(), f"{mode}: {name}: culled Gaussians got a gradient"


def test_statistics_sink_and_masked_colour(full):
    """The two side outputs of the row-sum stage against what the returned gradients say."""
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc, kw, wts = full
    # ---- the densification statistics (norms of dL/dmean2D, visibility count, largest radius), through the drop-in API
    stats = scene.FlatStats([sc.P], "cuda")
    t = {k: getattr(sc, k).cuda().requires_grad_(True) for k in ["means3D", "scales", "rotations", "opacities", "shs"]}
    m2d = torch.zeros(sc.P, 3, device="cuda", requires_grad=True)
    r = GaussianRasterizer(settings(cam))
    r.stats_sink = stats.sink()
    color, radii, depth, alpha, _ = r(t["means3D"], m2d, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    torch.autograd.backward([color, depth, alpha], [wts["color"].cuda(), wts["depth"].cuda(), wts["alpha"].cuda()])
    torch.cuda.synchronize()
    gm, vis = m2d.grad, radii > 0
    assert vis.any() and not vis.all()
    want = torch.zeros(sc.P, 2, device="cuda")
    want[vis, 0] = torch.sqrt(gm[vis, 0] * gm[vis, 0] + gm[vis, 1] * gm[vis, 1])
    want[vis, 1] = gm[vis, 2].abs()
    assert torch.allclose(stats.xyz_gradient_accum, want, rtol=1e-6, atol=0.0)
    assert torch.equal(stats.denom.reshape(-1), vis.float())
    assert torch.equal(stats.max_radii2D.reshape(-1), torch.where(vis, radii.float(), torch.zeros_like(radii, dtype=torch.float32)))
    # ---- masked_color_out: dL/dcolour with the channels the forward clamped at zero cleared
    res, internal = raw_forward(kw)
    masked = torch.full((sc.P, 3), float("nan"), device="cuda")
    g = backward_with(kw, res, wts, masked_color_out=masked)
    torch.cuda.synchronize()
    v = res["radii"] > 0
    cl = internal("clamped").reshape(sc.P, 3).to(torch.bool) & v[:, None]  # (not written for culled Gaussians)
    assert cl.any(), "no clamped channel in the scene"
    assert torch.equal(masked, torch.where(cl, torch.zeros_like(g["colors"]), g["colors"]))
