"""`-m gpu`: the per-tile LDS sort form of the binning chain (sgr_test_switches bit 12, csrc/sgr_tile_sort.hip: index-order
emission, stable tile sort, one radix sort by depth per tile in LDS) must produce the SAME sorted lists as the default chain
(depth pre-sort of the Gaussians, depth-order emission, stable tile sort) -- which the rest of the suite holds entry for
entry against the oracle and the reference's kernels (rasterizer_impl.cu:70-138,286-321): keys, point_list, ranges,
n_contrib, every image and every gradient bit for bit.  Covers the code paths of the kernels (one wave per tile for lists
up to 1024 entries, SGR_TS_WAVE_CAP; the 512-thread LDS sort up to 4096, SGR_TS_MED_CAP; the 1024-thread LDS sort up to
8192, SGR_TS_BIG_CAP; the HBM ping-pong beyond), equal depths (the tie order is ascending Gaussian id), far depths (32-bit
keys) and the reference's tile rects."""
import numpy as np
import pytest
import torch

from gpu_utils import npy, raw_backward, raw_forward, switches
from helpers import oracle_kwargs
from street_gaussians_amd import _C
from street_gaussians_amd import synthetic as syn

pytestmark = pytest.mark.gpu

INTERNALS = [("keys", np.uint64), ("point_list", np.uint32), ("ranges", np.uint32), ("n_contrib", np.uint32),
             ("point_offsets", np.uint32), ("tiles_touched", np.uint32), ("hits", np.uint8)]


def _run(kw, wts, mask, hits_defined=None):
    with switches(mask):
        res, internal = raw_forward(kw)
        g = raw_backward(kw, res, wts)
        torch.cuda.synchronize()
        out = {"R": res["R"]}
        for k in ["color", "depth", "alpha", "semantic", "radii"]:
            out[k] = npy(res[k]).copy()
        for k, dt in INTERNALS:
            out["i_" + k] = npy(internal(k)).view(dt).copy()
        for k, v in g.items():
            out["g_" + k] = npy(v).copy()
    return out


def _same(a, b, label):
    assert a["R"] == b["R"], label
    # the hit record is defined up to the last batch a tile processed (include/sgr.h, export 15): compare where both forms
    # processed the list -- positions below the tile's highest n_contrib
    for k in a:
        if k == "R" or k == "i_hits":
            continue
        assert np.array_equal(a[k], b[k]), (label, k, int((np.asarray(a[k]) != np.asarray(b[k])).sum()))


def _scene(name):
    if name == "mid":  # a few hundred entries per tile: one wave per tile
        cam = syn.make_camera(480, 320, fx=512.5, yaw_deg=2.0)
        return cam, syn.make_scene(40000, cam, S=3, seed=3), 3
    if name == "fat_tiles":  # 12 x 8 tiles, ~60 k splats of ~10 px: thousands of entries per tile -> the workgroup-per-tile LDS sorts
        cam = syn.make_camera(192, 128, fx=200.0)
        return cam, syn.make_scene(60000, cam, S=0, seed=5, scale_px=0.02, zmin=1.0, zmax=20.0), 0
    if name == "beyond_lds":  # the longest lists: past 8192 entries (SGR_TS_BIG_CAP) a tile takes the HBM ping-pong
        cam = syn.make_camera(64, 48, fx=70.0)
        return cam, syn.make_scene(50000, cam, S=0, seed=6, scale_px=0.03, zmin=1.0, zmax=12.0), 0
    if name == "equal_depths":  # a wall of splats at a handful of depths: almost every comparison is a tie
        cam = syn.make_camera(320, 208, fx=340.0)
        sc = syn.make_scene(30000, cam, S=0, seed=7, scale_px=0.01, zmin=2.0, zmax=9.0)
        z = torch.round(sc.means3D[:, 2])
        sc.means3D[:, 0] *= z / sc.means3D[:, 2]
        sc.means3D[:, 1] *= z / sc.means3D[:, 2]
        sc.means3D[:, 2] = z
        return cam, sc, 0
    if name == "far":  # depths beyond the 27-bit keys: the kernel sorts on all 32 bits
        cam = syn.make_camera(160, 96, fx=170.0)
        sc = syn.make_scene(4000, cam, S=0, seed=31, scale_px=0.02, zmin=1.0, zmax=8.0)
        far = sc.means3D.clone()
        n = far[::7].shape[0]
        far[::7, :] = far[::7, :] * torch.tensor([1.0, 1.0, 0.0]) * 3000.0 + torch.tensor([0.0, 0.0, 1.0]) * torch.linspace(13000.0, 90000.0, n)[:, None]
        sc.means3D.copy_(far)
        sc.scales[::7] *= 4000.0
        return cam, sc, 0
    raise KeyError(name)


@pytest.mark.parametrize("mode", ["default", "strict"])
@pytest.mark.parametrize("name", ["mid", "fat_tiles", "beyond_lds", "equal_depths", "far"])
def test_tile_sort_form_gives_the_default_chains_lists(name, mode):
    cam, sc, S = _scene(name)
    kw = oracle_kwargs(cam, sc, bg=torch.tensor([0.2, 0.1, 0.4]))
    wts = syn.loss_weights(cam, S=S)
    base = (_C.EXACT | _C.REF_RECT) if mode == "strict" else 0
    a = _run(kw, wts, base)
    b = _run(kw, wts, base | _C.TILE_SORT)
    _same(a, b, f"{name}/{mode}")
    # the test must have exercised what its name says
    rg = a["i_ranges"].reshape(-1, 2).astype(np.int64)
    longest = int((rg[:, 1] - rg[:, 0]).max())
    want = {"mid": (65, 2048), "fat_tiles": (2049, 7168), "beyond_lds": (7169, 10 ** 9), "equal_depths": (65, 10 ** 9),
            "far": (2, 10 ** 9)}[name]
    assert want[0] <= longest <= want[1], (name, longest)
    if name == "equal_depths":
        keys = a["i_keys"]
        assert int((keys[1:] == keys[:-1]).sum()) > 1000  # real ties in the 64-bit keys


def test_tile_sort_form_is_deterministic_over_repeated_forwards():
    cam, sc, S = _scene("fat_tiles")
    kw = oracle_kwargs(cam, sc)
    wts = syn.loss_weights(cam, S=S)
    first = _run(kw, wts, _C.TILE_SORT)
    for _ in range(3):
        _same(first, _run(kw, wts, _C.TILE_SORT), "repeat")


@pytest.mark.parametrize("mode", ["default", "strict"])
def test_longest_first_tile_order_changes_nothing(mode):
    """The tile order of the blend launches (XCD-aware supertiles / longest list first / decided per frame: sgr_test_switches
    bits 15 / 14 / default) changes no output and no internal array, bit for bit (tiles are independent) -- on a street-like
    scene with an empty sky and actor clusters composed by scene.compose."""
    from street_gaussians_amd import scene as sg
    cam = syn.make_camera(480, 320, fx=512.5)
    raw = syn.make_street_segments(60000, cam, n_actors=5, S=3, seed=2)
    segs = [sg.Segment(**{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items() if v is not None}) for d in raw]
    with torch.no_grad():
        means, rot, scl, opa, shs, sem = sg.compose(segs, 16, 3)
    sc = syn.Scene(means.cpu(), scl.cpu(), rot.cpu(), opa.cpu(), shs.cpu(), sem.cpu())
    kw = oracle_kwargs(cam, sc)
    wts = syn.loss_weights(cam, S=3)
    base = (_C.EXACT | _C.REF_RECT) if mode == "strict" else 0
    a = _run(kw, wts, base | _C.NO_LPT)          # XCD-aware supertile order, no look at the lists
    b = _run(kw, wts, base | _C.LPT)             # always longest-first
    c = _run(kw, wts, base)                      # decided per frame (this scene: longest-first)
    _same(a, b, "lpt/" + mode)
    _same(a, c, "adaptive/" + mode)
    rg = a["i_ranges"].reshape(-1, 2).astype(np.int64)
    n = rg[:, 1] - rg[:, 0]
    assert (n == 0).sum() > 10 and n.max() > 4 * n.mean()  # empty sky tiles and tiles several times the mean


def _forward_into_image_buffer(kw, img):
    """sgr_forward through the ctypes binding with the CALLER's image buffer `img` (uint8, sgr_image_bytes): what
    _C.rasterize_gaussians does, except that the image buffer callback hands out `img`."""
    import ctypes as C
    from street_gaussians_amd import _native
    dev = torch.device("cuda")
    t = {k: kw[k].to(dev).float().contiguous() for k in ("means3D", "shs", "semantics", "opacities", "scales", "rotations",
                                                          "viewmatrix", "projmatrix", "campos", "bg")}
    P, H, W = t["means3D"].shape[0], kw["image_height"], kw["image_width"]
    S, M = t["semantics"].shape[1], t["shs"].shape[1]
    out = dict(color=torch.empty(3, H, W, device=dev), depth=torch.empty(1, H, W, device=dev),
               alpha=torch.empty(1, H, W, device=dev), semantic=torch.empty(S, H, W, device=dev),
               radii=torch.empty(P, dtype=torch.int32, device=dev))
    geom, binning = _C._Grow(dev), _C._Grow(dev)
    img_cb = _native.ALLOC_FN(lambda nbytes, _user: img.data_ptr() if nbytes <= img.numel() else 0)
    vp = lambda x: C.c_void_p(x.data_ptr())
    R = _native.check(_native.lib().sgr_forward(
        geom.cb, None, binning.cb, None, img_cb, None, P, kw["sh_degree"], M, S, vp(t["bg"]), W, H, vp(t["means3D"]),
        vp(t["shs"]), None, vp(t["semantics"]), vp(t["opacities"]), vp(t["scales"]), 1.0, vp(t["rotations"]), None,
        vp(t["viewmatrix"]), vp(t["projmatrix"]), vp(t["campos"]), kw["tanfovx"], kw["tanfovy"], 0, vp(out["color"]),
        vp(out["depth"]), vp(out["alpha"]), vp(out["semantic"]), vp(out["radii"]), 1, _C._stream(dev)))
    torch.cuda.synchronize()
    return dict(out, R=R, geom=geom.tensor, binning=binning.tensor, img=img)


def test_backward_walks_the_tiles_in_its_frames_order():
    """Every forward leaves a valid tile-order flag in its image buffer (sgr_pack_camera_kernel clears it; the tile-order
    launch sets it when it runs), and the backward follows that flag whatever the switches say by the time it runs.  The
    image buffer is handed in holding a VALID longest-first block from an earlier frame (a permutation of the tile ids, flag
    1); a forward under NO_LPT must leave the flag at 0, and a default-switch backward over that frame must give the
    gradients of a NO_LPT forward + backward bit for bit."""
    from street_gaussians_amd import _native
    cam, sc, S = _scene("mid")
    kw = oracle_kwargs(cam, sc, bg=torch.tensor([0.1, 0.3, 0.2]))
    wts = syn.loss_weights(cam, S=S)
    H, W = kw["image_height"], kw["image_width"]
    N, T = H * W, ((W + 15) // 16) * ((H + 15) // 16)
    prev = _C.binding()
    _C.set_binding("ctypes")
    try:
        with switches(_C.NO_LPT):
            ref, _ = raw_forward(kw)
            g_ref = {k: npy(v).copy() for k, v in raw_backward(kw, ref, wts).items()}

        # sgr_img_carve: n_contrib[N], then (256-byte aligned) the T ranges, the T tile ids of the order block, its flag word
        img = torch.zeros((_native.lib().sgr_image_bytes(W, H) + 3) // 4 * 4, dtype=torch.uint8, device="cuda")
        up = lambda a: (a + 255) // 256 * 256
        ranges_w = (up(up(img.data_ptr()) + 4 * N) - img.data_ptr()) // 4
        words = img.view(torch.int32)
        words[ranges_w + 2 * T:ranges_w + 3 * T] = torch.randperm(T, generator=torch.Generator().manual_seed(5)).int().cuda()
        words[ranges_w + 3 * T] = 1
        with switches(_C.NO_LPT):
            res = _forward_into_image_buffer(kw, img)
        assert res["R"] == ref["R"]
        ranges = _C.export_internal("ranges", kw["means3D"].shape[0], res["R"], H, W, res["geom"], res["binning"], img)
        assert torch.equal(words[ranges_w:ranges_w + 2 * T], ranges.view(-1))  # the offsets above are the carve's
        assert int(words[ranges_w + 3 * T]) == 0, "a NO_LPT forward left the previous frame's tile-order flag behind"
        for k in ("color", "depth", "alpha", "semantic", "radii"):
            assert torch.equal(res[k], ref[k]), k
        with switches(0):
            g = raw_backward(kw, res, wts)
            torch.cuda.synchronize()
        for k, v in g_ref.items():
            assert np.array_equal(npy(g[k]), v), (k, int((npy(g[k]) != v).sum()))
    finally:
        _C.set_binding(prev)


@pytest.mark.parametrize("mode", ["default", "strict"])
def test_32_bit_tile_keys_give_the_same_lists_as_the_16_bit_default(mode):
    """The instance list's tile keys are 16-bit whenever the frame has fewer than 65535 tiles (the tile sort then moves 6
    instead of 8 bytes per pair and pass); switch bit 18 keeps the 32-bit keys that larger frames take anyway.  Same keys,
    lists, ranges, images and gradients bit for bit -- also through the per-tile sort form, whose scratch shares the key
    buffers."""
    cam, sc, S = _scene("mid")
    kw = oracle_kwargs(cam, sc, bg=torch.tensor([0.2, 0.1, 0.4]))
    wts = syn.loss_weights(cam, S=S)
    base = (_C.EXACT | _C.REF_RECT) if mode == "strict" else 0
    a = _run(kw, wts, base)
    b = _run(kw, wts, base | _C.KEY32)
    _same(a, b, "key32/" + mode)
    c = _run(kw, wts, base | _C.KEY32 | _C.TILE_SORT)
    _same(a, c, "key32+tile_sort/" + mode)
    assert int(a["i_keys"].max() >> 32) < 65535  # the frame is one the default sorts on 16-bit keys
