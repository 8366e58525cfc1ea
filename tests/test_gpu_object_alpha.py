"""`-m gpu` tests of the object-alpha head (GaussianRasterizer.forward_with_object_alpha, include/sgr_object_alpha.h).

The yardstick is the path the head replaces: the library's plain ``forward`` over Gaussians [split, P) alone, in the same
switch mask, and its backward with the upstream gradient on alpha only.  Images are compared with np.array_equal (the same
expressions on the same list order: no tolerance), gradients with gpu_utils.grad_close at its defaults (the two backwards
sum the same terms in different orders), and rows [0, split) of every gradient must be exactly zero.  What the cases are
built to catch: an object layer that inherits the COMPOSITE's termination or its set of partial rows (objects behind an
opaque wall, for which the composite's backward writes no row at all), a backward that does not reproduce the layer's OWN
termination (opaque objects: a pixel finishes after two or three entries), and the two heads disturbing each other through
the row flags they share."""

import numpy as np
import pytest
import torch

from street_gaussians_amd import _C, rasterizer
from street_gaussians_amd import synthetic as syn

from gpu_utils import dev, grad_close, npy, oracle_backward_same_state, settings, switches
from helpers import oracle_kwargs, small_case

pytestmark = pytest.mark.gpu

FRAME_BG = torch.tensor([0.1, 0.3, 0.6])
GEOM = ("means3D", "opacities", "scales", "rotations")


def _leaves(sc, lo=0, hi=None, cov=False):
    """Leaf tensors (requires_grad) of GaussianRasterizer.forward for Gaussians [lo, hi) of scene `sc`."""
    hi = sc.P if hi is None else hi
    d = lambda t: dev(t[lo:hi]).requires_grad_(True)
    kw = dict(means3D=d(sc.means3D), means2D=torch.zeros(hi - lo, 3, device="cuda", requires_grad=True),
              opacities=d(sc.opacities), shs=d(sc.shs))
    if cov:
        kw["cov3D_precomp"] = d(_cov6(sc))
    else:
        kw["scales"], kw["rotations"] = d(sc.scales), d(sc.rotations)
    if sc.semantics.shape[1]:
        kw["semantics"] = d(sc.semantics)
    return kw


def _cov6(sc):
    import torch_ref as tr
    Sig = tr.cov3d_from_scale_rot(sc.scales.double(), sc.rotations.double(), 1.0)
    return torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], -1).float()


def _weight(cam, seed=11):
    g = torch.Generator().manual_seed(seed)
    return dev(torch.rand(1, cam.image_height, cam.image_width, generator=g) * 2.0 - 1.0)


def _names(cov):
    return ("means3D", "opacities", "cov3D_precomp") if cov else GEOM


def _yardstick(cam, sc, split, w, cov=False):
    """The parent path: plain forward over [split, P), backward of sum(w * alpha) -> (alpha image, {name: gradient})."""
    from diff_gaussian_rasterization import GaussianRasterizer
    kw = _leaves(sc, split, sc.P, cov=cov)
    _, _, _, alpha, _ = GaussianRasterizer(settings(cam, bg=FRAME_BG))(**kw)
    (alpha * w).sum().backward()
    torch.cuda.synchronize()
    return npy(alpha), {k: npy(kw[k].grad) for k in _names(cov)}


def _head(cam, sc, split, w, cov=False):
    """forward_with_object_alpha over the whole scene, backward of sum(w * acc_object).
    -> (dict of the six outputs + R, {name: gradient of full length P})"""
    from diff_gaussian_rasterization import GaussianRasterizer
    kw = _leaves(sc, cov=cov)
    color, radii, depth, alpha, sem, acc = GaussianRasterizer(settings(cam, bg=FRAME_BG)).forward_with_object_alpha(**kw, split=split)
    R = rasterizer.last_num_rendered()
    (acc * w).sum().backward()
    torch.cuda.synchronize()
    assert acc.shape == (1, cam.image_height, cam.image_width)
    # the object head never touches means2D, colours or semantics
    for k in ("means2D", "shs", "semantics"):
        assert k not in kw or kw[k].grad is None, k
    out = dict(color=npy(color), radii=npy(radii), depth=npy(depth), alpha=npy(alpha), semantic=npy(sem), acc=npy(acc), R=R)
    return out, {k: npy(kw[k].grad) for k in _names(cov)}


def _compare(grads, want, split, label):
    for k, b in want.items():
        a = grads[k]
        assert a.shape[0] == split + b.shape[0], (label, k)
        assert not a[:split].any(), f"{label}: {k} rows [0, split) are not zero"
        assert np.abs(b).max() > 0, (label, k)
        grad_close(a[split:], b, name=f"object alpha {label}: {k}")


# ---- 1. small general case ---------------------------------------------------------------------------------------------

SMALL = dict(P=300, W=50, H=37, S=2)  # 50 x 37: ragged edge tiles
SPLIT = 120


@pytest.mark.parametrize("mask", [0, _C.EXACT, _C.EXACT | _C.REF_RECT], ids=["default", "exact", "strict"])
def test_small_case_equals_the_subset_render_and_its_backward(mask):
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc = small_case(**SMALL)
    w = _weight(cam)
    with switches(mask):
        want_alpha, want = _yardstick(cam, sc, SPLIT, w)
        got, grads = _head(cam, sc, SPLIT, w)
        with torch.no_grad():
            kw = {k: v.detach() for k, v in _leaves(sc).items()}
            rast = GaussianRasterizer(settings(cam, bg=FRAME_BG))
            plain = rast(**kw)
            R = rasterizer.last_num_rendered()
            layers = rast.forward_layers(**kw, split=SPLIT)[5]
        torch.cuda.synchronize()
    assert want_alpha.max() > 0.5
    assert np.array_equal(got["acc"], want_alpha), "acc_object differs from the subset forward's alpha"
    assert np.array_equal(got["acc"], npy(layers.acc_rest)), "acc_object differs from forward_layers' acc_rest"
    for k, t in zip(("color", "radii", "depth", "alpha", "semantic"), plain):
        assert np.array_equal(got[k], npy(t)), f"composite {k} differs from forward's"
    assert got["R"] == R
    _compare(grads, want, SPLIT, f"small/{mask}")
    if mask == 0:
        # ... and against the reference algorithm itself (the C oracle) over the subset, upstream on alpha only, fed with the
        # alpha image the head's backward was given (gpu_utils.oracle_backward_same_state)
        from oracle import oracle
        okw = oracle_kwargs(cam, sc, bg=FRAME_BG, semantics=False)
        per = ("means3D", "opacities", "shs", "scales", "rotations")
        fw = oracle.forward(**{k: (v[SPLIT:] if k in per else v) for k, v in okw.items()})
        H, W = cam.image_height, cam.image_width
        wts = dict(color=torch.zeros(3, H, W), depth=torch.zeros(1, H, W), alpha=w.cpu(), semantic=None)
        g = oracle_backward_same_state(oracle, fw, dict(alpha=torch.from_numpy(got["acc"])), wts, 0)
        fw.free()
        for k, ok in (("means3D", "means3D"), ("opacities", "opacity"), ("scales", "scales"), ("rotations", "rotations")):
            grad_close(grads[k][SPLIT:], np.asarray(g[ok]).reshape(grads[k][SPLIT:].shape), name=f"object alpha small: oracle {k}")


# ---- 2. split = 0: the object layer is the whole frame -------------------------------------------------------------------

def test_split_zero_is_the_composites_alpha_head():
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc = small_case(**SMALL)
    w = _weight(cam)
    got, grads = _head(cam, sc, 0, w)
    assert np.array_equal(got["acc"], got["alpha"])
    kw = _leaves(sc)
    _, _, _, alpha, _ = GaussianRasterizer(settings(cam, bg=FRAME_BG))(**kw)
    (alpha * w).sum().backward()
    torch.cuda.synchronize()
    _compare(grads, {k: npy(kw[k].grad) for k in GEOM}, 0, "split0")


# ---- 3. occlusion, long lists and the layer's own termination ------------------------------------------------------------

def _stack_scene(arrangement):
    """The stacked scenes of tests/test_gpu_layers.py, with ellipsoids for its spheres: 32 x 32 px (four tiles), 700 Gaussians whose centres lie within 2 px
    of the tiles' common corner, so every tile's list holds all 700 -- several staging rounds.  100 OPAQUE splats (opacity
    0.99, ~20 px sigma: a pixel ends within a few entries) and 600 TRANSLUCENT ones (opacity 0.05-0.3, ~5 px sigma, depths
    5-20).  (a) opaque = layer 0 at depth 2: the objects are translucent BEHIND the wall; (b) the layers swapped: the objects
    are the opaque ones in front; (c) opaque = layer 0 at depth 10, between the others.  -> (cam, scene, split)"""
    fx = 35.0
    cam = syn.make_camera(32, 32, fx=fx)
    g = torch.Generator().manual_seed(3)
    n_op, n_tr = 100, 600
    z_op = torch.full((n_op,), 10.0 if arrangement == "c" else 2.0) + 0.001 * torch.arange(n_op)
    z_tr = torch.linspace(5.0, 20.0, n_tr)[torch.randperm(n_tr, generator=g)]

    def block(z, sigma_px, op_lo, op_hi):
        n = z.shape[0]
        off = (torch.rand(n, 2, generator=g) * 4.0 - 2.0) / fx  # +-2 px around the principal point
        means = torch.stack([off[:, 0] * z, off[:, 1] * z, z], 1)
        # (mildly anisotropic, unlike the layers test's spheres: the rotation gradient of a sphere is analytically zero, and
        # what float32 leaves of it -- 1e-8 of the scale gradient here -- is rounding that no relative gate can compare)
        scales = (sigma_px * z / fx)[:, None] * torch.tensor([0.85, 1.0, 1.15])
        rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)
        opac = op_lo + (op_hi - op_lo) * torch.rand(n, 1, generator=g)
        shs = torch.zeros(n, 16, 3)
        shs[:, 0] = torch.rand(n, 3, generator=g) * 2.0 - 1.0
        return [means, scales, rot, opac, shs]
    opaque, transl = block(z_op, 20.0, 0.99, 0.99), block(z_tr, 5.0, 0.05, 0.3)
    first, rest = (transl, opaque) if arrangement == "b" else (opaque, transl)
    means, scales, rot, opac, shs = [torch.cat([a, b], 0).contiguous() for a, b in zip(first, rest)]
    sc = syn.Scene(means, scales, rot, opac, shs, torch.zeros(n_op + n_tr, 0))
    return cam, sc, first[0].shape[0]


@pytest.mark.parametrize("mask", [0, _C.EXACT], ids=["default", "exact"])
@pytest.mark.parametrize("arrangement", ["a", "b", "c"])
def test_stacked_scenes(arrangement, mask):
    cam, sc, split = _stack_scene(arrangement)
    w = _weight(cam, seed=5)
    with switches(mask):
        want_alpha, want = _yardstick(cam, sc, split, w)
        got, grads = _head(cam, sc, split, w)
        last = _last_image(cam, sc, split)
    assert np.array_equal(got["acc"], want_alpha), arrangement
    assert want_alpha.max() > 0.5
    if arrangement == "b":
        # opaque objects: every pixel's layer ends within the first entries (two or three at the centre, a dozen in the
        # corners) although the list is 700 long
        assert 0 < last.max() < 100 and np.abs(got["acc"] - got["alpha"]).max() == 0.0, last.max()
    else:
        # translucent objects behind (a) / around (c) the wall: hidden in the composite, blending deep into the list alone
        assert np.abs(got["acc"] - got["alpha"]).max() > 0.0
        assert last.max() > 512, last.max()
    _compare(grads, want, split, f"stack {arrangement}/{mask}")


def _last_image(cam, sc, split):
    """The head's private per-pixel last position, through the binding (the layer's n_contrib)."""
    kw = oracle_kwargs(cam, sc, bg=FRAME_BG, semantics=False)
    e = torch.Tensor([])
    out = _C.rasterize_gaussians(dev(FRAME_BG), dev(sc.means3D), e, torch.zeros(sc.P, 0, device="cuda"), dev(sc.opacities),
                                 dev(sc.scales), dev(sc.rotations), 1.0, e, dev(cam.viewmatrix), dev(cam.projmatrix),
                                 kw["tanfovx"], kw["tanfovy"], kw["image_height"], kw["image_width"], dev(sc.shs), 3,
                                 dev(cam.campos), False, False)
    R, geom, binning, img = out[0], out[6], out[7], out[8]
    _, last = _C.layer_alpha_forward(sc.P, R, kw["image_height"], kw["image_width"], split, geom, binning, img)
    torch.cuda.synchronize()
    return npy(last)


# ---- 4. both heads in one graph ------------------------------------------------------------------------------------------

def test_both_heads_in_one_graph_do_not_disturb_each_other():
    from diff_gaussian_rasterization import GaussianRasterizer
    from street_gaussians_amd.scene import FlatStats
    cam, sc, split = _stack_scene("a")  # the wall in front: the two heads mark different sets of partial rows
    H, W = cam.image_height, cam.image_width
    lw = syn.loss_weights(cam, S=0)
    wc, wd, wa, wo = dev(lw["color"]), dev(lw["depth"]), dev(lw["alpha"]), _weight(cam, seed=5)
    comp_names = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")

    def graph(with_object, sink=None):
        kw = _leaves(sc)
        rast = GaussianRasterizer(settings(cam, bg=FRAME_BG))
        rast.stats_sink = sink
        if with_object:
            color, _, depth, alpha, _, acc = rast.forward_with_object_alpha(**kw, split=split)
            lo = (acc * wo).sum()
        else:
            color, _, depth, alpha, _ = rast(**kw)
            lo = None
        lc = (color * wc).sum() + (depth * wd).sum() + (alpha * wa).sum()
        return kw, lc, lo

    def grad(loss, kw, names, retain=True):
        g = torch.autograd.grad(loss, [kw[k] for k in names], retain_graph=retain)
        torch.cuda.synchronize()
        return {k: t.clone() for k, t in zip(names, g)}

    kw, lc, lo = graph(True)
    runs_c, runs_o = [], []
    runs_c.append(grad(lc, kw, comp_names)); runs_o.append(grad(lo, kw, GEOM))   # composite first, then object
    runs_o.append(grad(lo, kw, GEOM)); runs_c.append(grad(lc, kw, comp_names))   # the reverse
    runs_c.append(grad(lc, kw, comp_names)); runs_o.append(grad(lo, kw, GEOM))   # the first order again
    for runs, label in ((runs_c, "composite"), (runs_o, "object")):
        for r in runs[1:]:
            for k in r:
                assert torch.equal(r[k], runs[0][k]), f"{label} head: {k} changed with the order of the backwards"
    # each head differentiated alone
    kw1, lc1, _ = graph(False)
    alone_c = grad(lc1, kw1, comp_names, retain=False)
    kw2, _, lo2 = graph(True)
    alone_o = grad(lo2, kw2, GEOM, retain=False)
    for k in comp_names:
        assert torch.equal(alone_c[k], runs_c[0][k]), f"composite head: {k} differs from the plain forward's backward"
    for k in GEOM:
        assert torch.equal(alone_o[k], runs_o[0][k]), f"object head: {k} differs from the head differentiated alone"
        assert not alone_o[k][:split].any() and alone_o[k][split:].abs().max() > 0, k
    # one backward() over the sum of both losses: autograd adds the two heads
    stats_with = FlatStats([split, sc.P - split], "cuda")
    kw3, lc3, lo3 = graph(True, stats_with.sink())
    (lc3 + lo3).backward()
    torch.cuda.synchronize()
    for k in GEOM:
        want = npy(runs_c[0][k]).astype(np.float64) + npy(runs_o[0][k]).astype(np.float64)
        grad_close(npy(kw3[k].grad), want, name=f"object alpha both heads: {k}")
    # what the object head must never touch: means2D.grad, dL/dSH and the densification statistics
    stats_without = FlatStats([split, sc.P - split], "cuda")
    kw4, lc4, _ = graph(False, stats_without.sink())
    lc4.backward()
    torch.cuda.synchronize()
    assert torch.equal(kw3["means2D"].grad, kw4["means2D"].grad) and kw4["means2D"].grad.abs().max() > 0
    assert torch.equal(kw3["shs"].grad, kw4["shs"].grad)
    for a, b in zip(stats_with.sink(), stats_without.sink()):
        assert torch.equal(a, b) and a.abs().max() > 0


# ---- 5. empty object layers ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["splitP", "P0"])
def test_empty_object_layer(which):
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc = small_case(**SMALL)
    if which == "P0":
        sc = syn.Scene(*[t[:0].contiguous() for t in (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs, sc.semantics)])
    kw = _leaves(sc)
    rast = GaussianRasterizer(settings(cam, bg=FRAME_BG))
    color, radii, depth, alpha, sem, acc = rast.forward_with_object_alpha(**kw, split=sc.P)
    assert acc.shape == (1, 37, 50) and not npy(acc).any()
    assert acc.grad_fn is None and not acc.requires_grad  # no launch was recorded: nothing to differentiate
    with torch.no_grad():
        plain = rast(**kw)
    for a, b in zip((color, radii, depth, alpha, sem), plain):
        assert torch.equal(a, b)
    if sc.P:
        ((color * 0.5).sum() + (acc * 2.0).sum()).backward()  # the composite's graph is intact; the object head adds nothing
        torch.cuda.synchronize()
        assert kw["opacities"].grad.abs().max() > 0
        # the native calls themselves: zeros without a walk, zero gradients
        with torch.no_grad():
            d = {k: v.detach() for k, v in kw.items()}
            out = _C.rasterize_gaussians(dev(FRAME_BG), d["means3D"], torch.Tensor([]), d["semantics"], d["opacities"], d["scales"],
                                         d["rotations"], 1.0, torch.Tensor([]), dev(cam.viewmatrix), dev(cam.projmatrix),
                                         cam.tanfovx, cam.tanfovy, 37, 50, d["shs"], 3, dev(cam.campos), False, False)
            a, last = _C.layer_alpha_forward(sc.P, out[0], 37, 50, sc.P, out[6], out[7], out[8])
            g = _C.layer_alpha_backward(out[0], 37, 50, sc.P, d["means3D"], d["scales"], d["rotations"], 1.0, None, out[5],
                                        out[6], out[7], out[8], a, last, torch.ones_like(a), False)
        torch.cuda.synchronize()
        assert not npy(a).any() and not npy(last).any()
        assert g[4] is None
        for t in g[:4]:
            assert t.shape[0] == sc.P and not npy(t).any()


# ---- 6. cov3D_precomp in place of scales and rotations -------------------------------------------------------------------

def test_cov3d_precomp():
    cam, sc = small_case(**SMALL)
    w = _weight(cam)
    want_alpha, want = _yardstick(cam, sc, SPLIT, w, cov=True)
    got, grads = _head(cam, sc, SPLIT, w, cov=True)
    assert np.array_equal(got["acc"], want_alpha)
    assert set(want) == {"means3D", "opacities", "cov3D_precomp"}
    _compare(grads, want, SPLIT, "cov3D_precomp")


# ---- 7. the other list orders, the per-tile binning chain and the lazy mode -------------------------------------------------

@pytest.mark.parametrize("mask", [_C.LPT, _C.TILE_SORT], ids=["longest-first", "tile-sort"])
def test_other_binning_chains(mask):
    cam, sc = small_case(**SMALL)
    w = _weight(cam)
    with switches(mask):
        want_alpha, want = _yardstick(cam, sc, SPLIT, w)
        _head(cam, sc, SPLIT, w)
        got, grads = _head(cam, sc, SPLIT, w)  # the second forward of this thread under the mask
    assert np.array_equal(got["acc"], want_alpha)
    _compare(grads, want, SPLIT, f"chain/{mask}")


def test_lazy_mode():
    cam, sc = small_case(**SMALL)
    w = _weight(cam)
    prev = _C.set_lazy(False)
    try:
        want_alpha, want = _yardstick(cam, sc, SPLIT, w)
        ref, _ = _head(cam, sc, SPLIT, w)
        _C.set_lazy(True)
        seed, _ = _head(cam, sc, SPLIT, w)  # the first forward after the switch blocks and seeds the list capacity
        got, grads = _head(cam, sc, SPLIT, w)
        R, cap, flags = _C.lazy_status()
        assert flags == 0 and R == ref["R"] and got["R"] == cap > R, (R, cap, flags, got["R"])  # a lazy call returns the capacity
    finally:
        _C.set_lazy(prev)
        torch.cuda.synchronize()
    for k in ("color", "radii", "depth", "alpha", "semantic", "acc"):
        assert np.array_equal(got[k], ref[k]) and np.array_equal(seed[k], ref[k]), k
    assert np.array_equal(got["acc"], want_alpha)
    _compare(grads, want, SPLIT, "lazy")


# ---- 8. determinism ------------------------------------------------------------------------------------------------------

def test_repeated_calls_give_identical_gradients():
    cam, sc = small_case(**SMALL)
    w = _weight(cam)
    a_out, a = _head(cam, sc, SPLIT, w)
    b_out, b = _head(cam, sc, SPLIT, w)
    assert np.array_equal(a_out["acc"], b_out["acc"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.abs(a[k]).max() > 0, k
