"""CPU tests of the layered forward (include/sgr_layers.h, GaussianRasterizer.forward_layers): the entry point is declared,
bound and exported; it refuses bad layer arguments before it touches the GPU or an allocation callback; the Python method
is inference only; and the premise the whole feature rests on holds on the reference algorithm's own binning (the C
oracle): a tile's sorted list of a contiguous subset IS the frame's list with the other Gaussians taken out."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import oracle_kwargs, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGR_E_INVALID = 1  # include/sgr.h


@pytest.fixture(scope="module")
def native():
    from street_gaussians_amd import _native, build
    build.build()  # hipcc cross-compiles for gfx950; a no-op when the objects are up to date
    return _native


def test_entry_point_is_declared_bound_and_exported(native):
    text = open(os.path.join(ROOT, "include", "sgr_layers.h")).read()
    assert re.search(r"^int\s+sgr_forward_layers\s*\(", text, re.M)
    assert "typedef struct sgr_layer_images" in text
    for ref in ("street_gaussian_renderer.py:13-40", ":138-151", ":242-243"):
        assert ref in text, ref
    lib = C.CDLL(native.LIB_PATH)
    assert hasattr(lib, "sgr_forward_layers")
    rf, af = native.SIGNATURES["sgr_forward"]
    rl, al = native.SIGNATURES["sgr_forward_layers"]
    assert rl is rf and list(al) == list(af) + [C.c_void_p]
    lib.sgr_version.restype = C.c_int
    assert lib.sgr_version() >= 103


def _call_with_layers(native, P, li, calls):
    """sgr_forward_layers with null data pointers and allocation callbacks that record every invocation."""
    from street_gaussians_amd import _C

    def alloc(nbytes, _user):
        calls.append(int(nbytes))
        return None
    cb = native.ALLOC_FN(alloc)
    return native.lib().sgr_forward_layers(cb, None, cb, None, cb, None, P, 0, 0, 0, None, 32, 32, None, None, None, None,
                                           None, None, 1.0, None, None, None, None, None, 1.0, 1.0, 0, None, None, None, None,
                                           None, 0, None, C.byref(li) if li is not None else None), _C


def test_bad_layer_arguments_are_refused_before_anything_runs(native):
    from street_gaussians_amd._C import _LayerImages
    # addresses that are never dereferenced: the call must return before it reaches the GPU
    ok = dict(background=0x1000, color=(0x2000, 0x3000), alpha=(0x4000, 0x5000))

    def images(split, background=ok["background"], color=ok["color"], alpha=ok["alpha"]):
        return _LayerImages(split, background, 1, (C.c_void_p * 2)(*color), (C.c_void_p * 2)(*alpha))

    cases = [(images(-1), "split"), (images(9), "split"), (images(4, color=(0x2000, None)), "color[1]"),
             (images(4, alpha=(None, 0x5000)), "alpha[0]"), (images(4, background=None), "background")]
    for li, word in cases:
        calls = []
        rc, _ = _call_with_layers(native, 8, li, calls)
        assert rc == -SGR_E_INVALID, (word, rc)
        assert word in native.lib().sgr_last_error().decode(), (word, native.lib().sgr_last_error())
        assert calls == [], word


def test_forward_layers_is_inference_only():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from street_gaussians_amd import rasterizer
    assert hasattr(GaussianRasterizer, "forward_layers")
    assert rasterizer.LayerImages._fields == ("rgb_first", "acc_first", "rgb_rest", "acc_rest")
    st = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False)
    z = torch.zeros
    rast = GaussianRasterizer(st)
    # CPU tensors: the refusal comes before the device check (which would raise SgrError)
    with torch.enable_grad():
        with pytest.raises(ValueError, match="no_grad"):
            rast.forward_layers(z(4, 3), None, z(4, 1, requires_grad=True), shs=z(4, 1, 3), scales=z(4, 3),
                                rotations=z(4, 4), split=2)
    # the exactly-one-of checks are forward's
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        rast.forward_layers(z(4, 3), None, z(4, 1), scales=z(4, 3), rotations=z(4, 4), split=2)
    with pytest.raises(Exception, match="scale/rotation pair"):
        rast.forward_layers(z(4, 3), None, z(4, 1), shs=z(4, 1, 3), scales=z(4, 3), split=2)


def _subset(kw, lo, hi):
    per_gaussian = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "semantics")
    return {k: (v[lo:hi] if k in per_gaussian and v is not None else v) for k, v in kw.items()}


def test_a_subsets_tile_lists_are_the_frames_lists_filtered():
    """The premise, on the reference's own binning: for every tile, the full frame's (depth, index)-sorted list with the
    Gaussians of the other layer removed equals the list of a forward over the layer alone.  Integer equalities."""
    from oracle import oracle
    cam, sc = small_case(P=200, W=50, H=37)
    kw = oracle_kwargs(cam, sc)
    split, P = 80, 200
    full = oracle.forward(**kw)
    pl = np.asarray(full.point_list).astype(np.int64)
    rg = np.asarray(full.ranges).astype(np.int64)
    assert full.num_rendered > 0
    nonempty = [0, 0]
    for layer, (lo, hi) in enumerate(((0, split), (split, P))):
        sub = oracle.forward(**_subset(kw, lo, hi))
        spl = np.asarray(sub.point_list).astype(np.int64)
        srg = np.asarray(sub.ranges).astype(np.int64)
        assert srg.shape == rg.shape
        total = 0
        for t in range(rg.shape[0]):
            mine = pl[rg[t, 0]:rg[t, 1]]
            mine = mine[(mine >= lo) & (mine < hi)] - lo
            assert np.array_equal(mine, spl[srg[t, 0]:srg[t, 1]]), (layer, t)
            total += mine.size
            nonempty[layer] += bool(mine.size)
        assert total == sub.num_rendered == spl.size
        sub.free()
    full.free()
    assert min(nonempty) > 0  # both layers reach the lists: the equalities above compared something
