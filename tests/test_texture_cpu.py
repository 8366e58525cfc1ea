"""CPU pins of the cube-map lookup (include/sgr_texture.h, street_gaussians_amd/texture.py, the nvdiffrast drop-in):
the float64 restatement (torch_ref_texture.py) held to the reference's own face orientation -- `cube_to_dir` of
lib/models/sky_cubemap.py:154-161, cut out of its source and executed (its recorded outputs where the reference
checkout is absent) -- and the drop-in's refusals, which are all decided before any device is touched."""
import os
import re

import numpy as np
import pytest
import torch

import torch_ref_texture as tr
from golden.refpin import reference_path

SKY = "lib/models/sky_cubemap.py"  # under the reference checkout (golden/refpin.py)
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture", "cube_to_dir.npz")
SIZES = (1, 2, 5, 8)


def _reference_cube_to_dir():
    src = open(reference_path(SKY)).read()
    m = re.search(r"^def cube_to_dir\(.*?(?=^\S)", src, re.S | re.M)
    ns = {"torch": torch}
    exec(m.group(0), ns)
    return ns["cube_to_dir"]


def _grid(R, lo, hi, n):
    gy, gx = torch.meshgrid(torch.linspace(lo, hi, n, dtype=torch.float64), torch.linspace(lo, hi, n, dtype=torch.float64),
                            indexing="ij")
    return gx, gy


def _directions(cube_to_dir):
    """What cube_to_dir returns at the texel centres (latlong_to_cubemap's grid, :166-168) and at the texel corners of
    every face, for each R of SIZES."""
    out = {}
    for R in SIZES:
        for s in range(6):
            out[f"centres/{R}/{s}"] = cube_to_dir(s, *_grid(R, -1 + 1 / R, 1 - 1 / R, R))
            out[f"corners/{R}/{s}"] = cube_to_dir(s, *_grid(R, -1.0, 1.0, R + 1))
    return out


def _reference_directions():
    if os.path.exists(reference_path(SKY)):
        live = _directions(_reference_cube_to_dir())
        if os.environ.get("SGR_RECORD_REFERENCE_OUTPUTS") == "1":
            os.makedirs(os.path.dirname(RECORD), exist_ok=True)
            np.savez_compressed(RECORD, **{k: v.numpy() for k, v in live.items()})
        return live
    with np.load(RECORD) as rec:
        return {k: torch.from_numpy(rec[k]) for k in rec.files}


@pytest.fixture(scope="module")
def ref_dirs():
    return _reference_directions()


def test_record_matches_the_reference(ref_dirs):
    """Where the reference is present, the stored record still describes what cube_to_dir returns."""
    with np.load(RECORD) as rec:
        assert sorted(rec.files) == sorted(ref_dirs)
        for k, v in ref_dirs.items():
            assert torch.equal(torch.from_numpy(rec[k]), v), k


@pytest.mark.parametrize("R", SIZES)
def test_texel_centres_sample_their_own_texel(ref_dirs, R):
    """The direction cube_to_dir gives texel (s, row j, col i) is looked up at exactly that texel, weight 1."""
    tex = torch.randn(1, 6, R, R, 2, dtype=torch.float64)
    for s in range(6):
        d = ref_dirs[f"centres/{R}/{s}"]
        face, u, v = tr.face_uv(d)
        assert (face == s).all()
        j, i = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
        assert torch.allclose(u * R - 0.5, i.double(), atol=1e-9, rtol=0)
        assert torch.allclose(v * R - 0.5, j.double(), atol=1e-9, rtol=0)
        out = tr.texture_ref(tex, d.unsqueeze(0))[0]
        assert torch.allclose(out, tex[0, s], atol=1e-9, rtol=0)


def test_texel_dir_inverts_the_reference_orientation(ref_dirs):
    """The restatement's inverse map (which the seam table is derived from) is cube_to_dir at every texel centre."""
    for R in SIZES:
        for s in range(6):
            d = ref_dirs[f"centres/{R}/{s}"]
            for j in range(R):
                for i in range(R):
                    assert torch.allclose(torch.tensor(tr.texel_dir(s, R, i, j), dtype=torch.float64), d[j, i], atol=1e-12)


@pytest.mark.parametrize("R", SIZES)
def test_seam_table_joins_texels_that_share_an_edge_segment(ref_dirs, R):
    """A tap one texel across edge e of face f lands on a texel of another face whose square shares, in 3D, the edge
    segment of the border texel it continues -- the geometry of cube_to_dir at the texel corners."""
    table = tr.seam_table()

    def square(s, col, row):
        c = ref_dirs[f"corners/{R}/{s}"]  # [row corner, col corner, xyz]
        return {(0, col): (c[row, col], c[row + 1, col]), (1, col): (c[row, col + 1], c[row + 1, col + 1]),
                (2, row): (c[row, col], c[row, col + 1]), (3, row): (c[row + 1, col], c[row + 1, col + 1])}

    def same(a, b):
        return (torch.allclose(a[0], b[0], atol=1e-12) and torch.allclose(a[1], b[1], atol=1e-12)) or \
               (torch.allclose(a[0], b[1], atol=1e-12) and torch.allclose(a[1], b[0], atol=1e-12))

    for (f, e), (g, c0, c1, r0, r1) in table.items():
        assert g != f
        for k in range(R):
            col, row = (0, k) if e == 0 else (R - 1, k) if e == 1 else (k, 0) if e == 2 else (k, R - 1)
            own = square(f, col, row)
            seg = [v for (side, _), v in own.items() if side == e][0]
            gc, gr = c0 * (R - 1) + c1 * k, r0 * (R - 1) + r1 * k
            assert 0 <= gc < R and 0 <= gr < R
            assert any(same(seg, v) for v in square(g, gc, gr).values()), (f, e, k)
    # every edge of the cube is shared by exactly two faces, each pointing at the other
    for (f, e), (g, *_rest) in table.items():
        assert sum(table[(g, b)][0] == f for b in range(4)) == 1


def test_restatement_contract_details():
    """Zero and NaN directions give 0 and no taps; corner taps share their weight; weights sum to 1."""
    R, C = 3, 2
    tex = torch.randn(1, 6, R, R, C, dtype=torch.float64)
    uv = torch.tensor([[[[0.0, 0.0, 0.0], [float("nan"), 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.3, -0.2]]]])
    out = tr.texture_ref(tex, uv)
    assert (out[0, 0, :2] == 0).all()
    idx, w, valid = tr.tap_weights(uv, 1, R)
    assert valid.tolist() == [False, False, True, True]
    assert torch.allclose(w[2:].sum(-1), torch.ones(2, dtype=torch.float64))
    assert (idx[2] == -1).sum() == 1  # a cube corner direction: one footprint corner outside both edges


def test_drop_in_imports_and_refuses_before_touching_a_device():
    import nvdiffrast.torch as dr
    from street_gaussians_amd._native import SgrError
    tex = torch.zeros(1, 6, 4, 4, 3)
    uv = torch.ones(1, 2, 2, 3)
    for kw, name in ((dict(boundary_mode="wrap"), "boundary_mode"), (dict(boundary_mode="clamp"), "boundary_mode"),
                     (dict(boundary_mode="zero"), "boundary_mode"), (dict(filter_mode="nearest"), "filter_mode"),
                     (dict(filter_mode="linear-mipmap-linear"), "filter_mode"),
                     (dict(filter_mode="linear-mipmap-nearest"), "filter_mode"), (dict(uv_da=uv), "uv_da"),
                     (dict(mip_level_bias=torch.zeros(1, 2, 2)), "mip_level_bias"), (dict(mip=[tex]), "mip")):
        args = dict(filter_mode="linear", boundary_mode="cube")
        args.update(kw)
        with pytest.raises(NotImplementedError, match=name):
            dr.texture(tex, uv, **args)
    with pytest.raises(NotImplementedError, match="uv"):
        dr.texture(tex, uv.clone().requires_grad_(True), filter_mode="linear", boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="RasterizeCudaContext"):
        dr.RasterizeCudaContext()
    with pytest.raises(SgrError):
        dr.texture(tex, uv, filter_mode="linear", boundary_mode="cube")
    with pytest.raises(SgrError):
        dr.texture(tex, uv, boundary_mode="cube")  # 'auto' without uv_da resolves to linear


def test_workspace_query_refuses_keys_beyond_32_bits():
    from street_gaussians_amd import _native, build
    build.build()  # a no-op when the library is up to date
    L = _native.lib()
    assert L.sgr_texture_cube_workspace_bytes(1, 1, 1024, 3, 1920 * 1280) > 0
    assert L.sgr_texture_cube_workspace_bytes(1, 1, 26000, 3, 16) > 0
    assert L.sgr_texture_cube_workspace_bytes(1, 1, 27000, 3, 16) == 0  # 6 * 27001^2 > 2^32
    assert L.sgr_texture_cube_workspace_bytes(2, 1, 8, 3, 16) == 0  # Bt must be 1 or B
