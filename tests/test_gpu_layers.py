"""`-m gpu` tests of the layered forward (GaussianRasterizer.forward_layers, include/sgr_layers.h).

The yardstick for a layer image is the library's own forward, in the same switch mask, over that layer's Gaussians alone
with bg = the layer background: the same expressions on the same list order, so the comparison is np.array_equal -- there is
no tolerance.  The composite's outputs and num_rendered are compared with a plain forward of the whole set the same way.
What the cases are built to catch is a layer that inherits the COMPOSITE's termination: an opaque layer in front must not
end the layer behind it."""
import numpy as np
import pytest
import torch

from street_gaussians_amd import _C, rasterizer
from street_gaussians_amd import synthetic as syn

from gpu_utils import dev, image_close, npy, raw_forward, settings, switches
from helpers import oracle_kwargs, small_case

pytestmark = pytest.mark.gpu

LAYER_BG = torch.tensor([0.2, 0.5, 0.9])
FRAME_BG = torch.tensor([0.1, 0.3, 0.6])


def _args(sc, lo=0, hi=None):
    """Keyword arguments of GaussianRasterizer.forward / forward_layers for Gaussians [lo, hi) of scene `sc`."""
    hi = sc.P if hi is None else hi
    d = lambda t: dev(t[lo:hi])
    kw = dict(means3D=d(sc.means3D), means2D=torch.zeros(hi - lo, 3, device="cuda"), opacities=d(sc.opacities), shs=d(sc.shs),
              scales=d(sc.scales), rotations=d(sc.rotations))
    if sc.semantics.shape[1]:
        kw["semantics"] = d(sc.semantics)
    return kw


def _plain(cam, sc, lo, hi, bg):
    """The yardstick: the library's plain forward over Gaussians [lo, hi) -> dict of numpy arrays."""
    from diff_gaussian_rasterization import GaussianRasterizer
    with torch.no_grad():
        color, radii, depth, alpha, sem = GaussianRasterizer(settings(cam, bg=bg))(**_args(sc, lo, hi))
    R = rasterizer.last_num_rendered()
    torch.cuda.synchronize()
    return dict(color=npy(color), radii=npy(radii), depth=npy(depth), alpha=npy(alpha), semantic=npy(sem), R=R)


def _layered(cam, sc, split, layer_bg=LAYER_BG, clamp=False, frame_bg=FRAME_BG):
    from diff_gaussian_rasterization import GaussianRasterizer
    with torch.no_grad():
        color, radii, depth, alpha, sem, lay = GaussianRasterizer(settings(cam, bg=frame_bg)).forward_layers(
            **_args(sc), split=split, layer_background=None if layer_bg is None else dev(layer_bg), clamp=clamp)
    R = rasterizer.last_num_rendered()
    torch.cuda.synchronize()
    assert isinstance(lay, rasterizer.LayerImages)
    return dict(color=npy(color), radii=npy(radii), depth=npy(depth), alpha=npy(alpha), semantic=npy(sem), R=R,
                layers=[(npy(lay.rgb_first), npy(lay.acc_first)), (npy(lay.rgb_rest), npy(lay.acc_rest))])


def _check(cam, sc, split, label, layer_bg=LAYER_BG, got=None):
    """forward_layers against three plain forwards, bit for bit.  -> (layered result, [plain layer 0, plain layer 1])"""
    got = _layered(cam, sc, split, layer_bg) if got is None else got
    whole = _plain(cam, sc, 0, sc.P, FRAME_BG)
    for k in ("color", "radii", "depth", "alpha", "semantic"):
        assert np.array_equal(got[k], whole[k]), f"{label}: composite {k} differs from the plain forward"
    assert got["R"] == whole["R"], label
    subs = []
    for layer, (lo, hi) in enumerate(((0, split), (split, sc.P))):
        if lo == hi:  # an empty layer is the background colour, not a forward's zero fill: test_empty_layers_are_background
            subs.append(None)
            continue
        sub = _plain(cam, sc, lo, hi, layer_bg)
        rgb, acc = got["layers"][layer]
        assert rgb.shape == sub["color"].shape and acc.shape == sub["alpha"].shape
        assert np.array_equal(acc, sub["alpha"]), f"{label}: layer {layer} alpha differs from the forward over the subset"
        assert np.array_equal(rgb, sub["color"]), f"{label}: layer {layer} colour differs from the forward over the subset"
        subs.append(sub)
    return got, subs


# ---- 1. small general case ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [0, _C.EXACT, _C.EXACT | _C.REF_RECT], ids=["default", "exact", "strict"])
def test_layers_equal_subset_forwards_small(mask):
    cam, sc = small_case(P=300, W=50, H=37, S=2)  # 50 x 37: ragged edge tiles
    split = 120
    with switches(mask):
        got, subs = _check(cam, sc, split, f"small/{mask}")
    assert subs[0]["alpha"].max() > 0.5 and subs[1]["alpha"].max() > 0.5
    if mask == 0:
        # ... and against the reference algorithm itself (the C oracle) on the subsets, at image_close's defaults
        from oracle import oracle
        kw = oracle_kwargs(cam, sc, bg=LAYER_BG)
        per = ("means3D", "opacities", "shs", "scales", "rotations", "semantics")
        for layer, (lo, hi) in enumerate(((0, split), (split, sc.P))):
            fw = oracle.forward(**{k: (v[lo:hi] if k in per else v) for k, v in kw.items()}, internals=False)
            rgb, acc = got["layers"][layer]
            image_close(rgb, fw.color, name=f"layers small: oracle colour {layer}")
            image_close(acc, fw.alpha, name=f"layers small: oracle alpha {layer}")
            fw.free()


# ---- 2. occlusion and long lists ---------------------------------------------------------------------------------------

def _stack_scene(arrangement):
    """32 x 32 px (four tiles), 700 Gaussians whose centres lie within 2 px of the image centre -- the common corner of the
    four tiles -- so every tile's list holds all 700: three staging batches.  100 OPAQUE splats (opacity 0.99, ~20 px sigma:
    they cover the whole image and end a pixel within ~20 entries) and 600 TRANSLUCENT ones (opacity 0.05-0.3, ~5 px sigma,
    depths 5-20: a pixel 10-13 px from the centre collects ~1 % per entry and is still blending in the third batch).
    (a) opaque = layer 0 at depth 2; (b) the same with the layers swapped; (c) opaque = layer 0 at depth 10, between the
    others.  -> (cam, scene, split, index of the translucent layer)"""
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
        scales = (sigma_px * z / fx)[:, None].repeat(1, 3)
        rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)
        opac = op_lo + (op_hi - op_lo) * torch.rand(n, 1, generator=g)
        shs = torch.zeros(n, 16, 3)
        shs[:, 0] = torch.rand(n, 3, generator=g) * 2.0 - 1.0
        return [means, scales, rot, opac, shs]
    opaque, transl = block(z_op, 20.0, 0.99, 0.99), block(z_tr, 5.0, 0.05, 0.3)
    first, rest = (transl, opaque) if arrangement == "b" else (opaque, transl)
    means, scales, rot, opac, shs = [torch.cat([a, b], 0).contiguous() for a, b in zip(first, rest)]
    sc = syn.Scene(means, scales, rot, opac, shs, torch.zeros(n_op + n_tr, 0))
    return cam, sc, first[0].shape[0], (0 if arrangement == "b" else 1)


@pytest.mark.parametrize("mask", [0, _C.EXACT], ids=["default", "exact"])
@pytest.mark.parametrize("arrangement", ["a", "b", "c"])
def test_an_opaque_layer_does_not_end_the_other_one(arrangement, mask):
    cam, sc, split, far = _stack_scene(arrangement)
    with switches(mask):
        got, subs = _check(cam, sc, split, f"stack {arrangement}/{mask}")
        # the case exercises what it claims: every tile's list spans three batches, the composite ends inside the first,
        # and the translucent layer alone is still blending in the third
        _, internal = raw_forward(oracle_kwargs(cam, sc, bg=FRAME_BG, semantics=False))
        rg = npy(internal("ranges")).astype(np.int64).reshape(-1, 2)
        nc = npy(internal("n_contrib")).view(np.uint32)
        lo, hi = ((0, split), (split, sc.P))[far]
        far_sc = syn.Scene(*[t[lo:hi].contiguous() for t in (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs, sc.semantics)])
        _, internal_far = raw_forward(oracle_kwargs(cam, far_sc, bg=LAYER_BG, semantics=False))
        nc_far = npy(internal_far("n_contrib")).view(np.uint32)
    assert rg.shape[0] == 4 and (rg[:, 1] - rg[:, 0] > 512).all(), rg
    assert nc.max() < 256, nc.max()
    assert nc_far.max() > 512, nc_far.max()
    assert subs[far]["alpha"].max() > 0.5
    # the far layer really is hidden in the composite somewhere it is visible alone
    assert np.abs(got["layers"][far][1] - got["alpha"]).max() > 0.0


# ---- 3. empty layers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["split0", "splitP", "P0"])
def test_empty_layers_are_background(which):
    cam, sc = small_case(P=300, W=50, H=37, S=2)
    if which == "P0":
        sc = syn.Scene(*[t[:0].contiguous() for t in (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs, sc.semantics)])
    split = {"split0": 0, "splitP": sc.P, "P0": 0}[which]
    got, _ = _check(cam, sc, split, which)  # (the non-empty layer equals the plain forward of everything)
    empty = {"split0": [0], "splitP": [1], "P0": [0, 1]}[which]
    want = np.broadcast_to(LAYER_BG.numpy()[:, None, None], (3, 37, 50))
    for layer in empty:
        rgb, acc = got["layers"][layer]
        assert np.array_equal(rgb, want), (which, layer)
        assert acc.shape == (1, 37, 50) and not acc.any(), (which, layer)


def test_layer_background_defaults_to_white():
    cam, sc = small_case(P=300, W=50, H=37, S=0)
    got = _layered(cam, sc, 120, layer_bg=None)
    _check(cam, sc, 120, "white", layer_bg=torch.ones(3), got=got)


# ---- 4. clamp ----------------------------------------------------------------------------------------------------------

def test_clamp_is_torch_clamp_of_the_unclamped_images():
    cam, sc = small_case(P=300, W=50, H=37, S=0)
    sc.shs[:, 0, :] += 3.0  # SH colours around 1.5
    bg = torch.tensor([-0.3, 0.5, 1.4])  # ... and a background outside [0, 1] on both sides
    raw = _layered(cam, sc, 120, layer_bg=bg, clamp=False)
    clamped = _layered(cam, sc, 120, layer_bg=bg, clamp=True)
    for layer in range(2):
        rgb, acc = raw["layers"][layer]
        assert rgb.max() > 1.0 and rgb.min() < 0.0  # the clamp has something to do, on both sides
        assert np.array_equal(clamped["layers"][layer][0], torch.clamp(torch.from_numpy(rgb), 0.0, 1.0).numpy())
        assert np.array_equal(clamped["layers"][layer][1], acc)
    assert np.array_equal(clamped["color"], raw["color"])  # the composite is never clamped


# ---- 5. street frame ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def street():
    from street_gaussians_amd import scene as sg
    cam = syn.make_camera(320, 208, fx=2050.0 * 320 / 1920)
    raw = syn.make_street_segments(20000, cam, n_actors=4)
    segs = [sg.Segment(**{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items() if v is not None}) for d in raw]
    with torch.no_grad():
        means, rot, scl, opa, shs, _ = sg.compose(segs, 16, 0)
    sc = syn.Scene(means.cpu(), scl.cpu(), rot.cpu(), opa.cpu(), shs.cpu(), torch.zeros(means.shape[0], 0))
    return cam, sc, int(raw[0]["xyz"].shape[0])  # compose puts the background model's rows first


@pytest.mark.parametrize("mask", [0, _C.LPT, _C.TILE_SORT], ids=["default", "longest-first", "tile-sort"])
def test_street_frame_background_and_objects(street, mask):
    cam, sc, split = street
    assert 0 < split < sc.P
    with switches(mask):
        got, subs = _check(cam, sc, split, f"street/{mask}")
    assert subs[0]["alpha"].max() > 0.5 and subs[1]["alpha"].max() > 0.5  # background and actors are both on screen
    assert (subs[1]["alpha"] == 0).mean() > 0.3  # ... and the objects cover only part of it


# ---- 6. lazy mode ------------------------------------------------------------------------------------------------------

def test_lazy_call_gives_the_blocking_calls_layers():
    cam, sc = small_case(P=300, W=50, H=37, S=2)
    prev = _C.set_lazy(False)
    try:
        ref, _ = _check(cam, sc, 120, "blocking")
        _C.set_lazy(True)
        seed = _layered(cam, sc, 120)  # the first forward after the switch blocks and seeds the list capacity
        assert seed["R"] == ref["R"]
        lazy = _layered(cam, sc, 120)
        R, cap, flags = _C.lazy_status()
        assert flags == 0 and R == ref["R"] and lazy["R"] == cap > R, (R, cap, flags, lazy["R"])  # a lazy call returns the capacity
        for got in (seed, lazy):
            for k in ("color", "radii", "depth", "alpha", "semantic"):
                assert np.array_equal(got[k], ref[k]), k
            for layer in range(2):
                assert np.array_equal(got["layers"][layer][0], ref["layers"][layer][0]), layer
                assert np.array_equal(got["layers"][layer][1], ref["layers"][layer][1]), layer
    finally:
        _C.set_lazy(prev)
        torch.cuda.synchronize()


# ---- 7. grad handling --------------------------------------------------------------------------------------------------

def test_no_output_takes_part_in_autograd():
    from diff_gaussian_rasterization import GaussianRasterizer
    cam, sc = small_case(P=300, W=50, H=37, S=2)
    kw = {k: v.requires_grad_(True) for k, v in _args(sc).items()}
    rast = GaussianRasterizer(settings(cam, bg=FRAME_BG))
    with pytest.raises(ValueError, match="no_grad"):
        rast.forward_layers(**kw, split=120)
    with torch.no_grad():
        color, radii, depth, alpha, sem, lay = rast.forward_layers(**kw, split=120)
    for t in (color, radii, depth, alpha, sem) + tuple(lay):
        assert not t.requires_grad and t.grad_fn is None
    assert lay.rgb_first.shape == (3, 37, 50) and lay.acc_rest.shape == (1, 37, 50)
