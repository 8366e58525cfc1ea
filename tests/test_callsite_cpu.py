"""CPU pin of the drop-in boundary's ARGUMENT CONVENTIONS against the reference's own call sites:
tests/golden/callsite/*.npz hold what StreetGaussianRenderer.render_kernel
(/root/reference/lib/models/street_gaussian_renderer.py:122-260, with make_rasterizer, lib/utils/camera_utils.py:194-227) and
script/test_gaussian_rasterization.py pass to GaussianRasterizer -- captured by executing those sources with a recording
rasterizer (tests/golden/make_callsite_fixture.py).  Here: (a) where /root/reference exists the capture is repeated and
must reproduce the committed fixtures bit for bit, (b) the conventions the package relies on are asserted on the fixtures,
(c) the oracle accepts the captured argument sets as they are (BASELINE.json configs[0]: the smoke-test recipe on the CPU
path; the mixed input kinds and the scaling modifiers 0.6 / 1.5 of render_kernel); tests/test_gpu_callsite.py replays them through the HIP path."""
import glob
import os

import numpy as np
import pytest
import torch

from golden import make_callsite_fixture as mk
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = sorted(glob.glob(os.path.join(HERE, "golden", "callsite", "*.npz")))


def test_fixtures_are_committed():
    assert len(FIX) == 8


@pytest.mark.skipif(not os.path.exists("/root/reference/lib/models/street_gaussian_renderer.py"),
                    reason="reference checkout not present on this machine")
def test_capture_from_the_reference_source_reproduces_the_fixtures():
    calls = mk.capture_all()
    assert sorted(calls) == sorted(os.path.basename(p)[:-4] for p in FIX)
    for name, (st, kw) in calls.items():
        fst, fkw, meta = mk.load(os.path.join(HERE, "golden", "callsite", name + ".npz"))
        for k in mk.SETTINGS_FIELDS:
            if torch.is_tensor(st[k]):
                assert torch.equal(st[k].detach(), fst[k]), (name, k)
            else:
                assert st[k] == fst[k], (name, k)
        for k in mk.CALL_ARGS:
            if kw[k] is None:
                assert fkw[k] is None, (name, k)
            else:
                assert torch.equal(kw[k].detach(), fkw[k]), (name, k)
                assert kw[k].requires_grad == (k in meta["requires_grad"]), (name, k)


def test_argument_conventions_of_the_reference_call_sites():
    for path in FIX:
        name = os.path.basename(path)[:-4]
        st, kw, meta = mk.load(path)
        P = kw["means3D"].shape[0]
        assert set(kw) == set(mk.CALL_ARGS)  # keyword call with exactly these nine names (street_gaussian_renderer.py:230-240)
        assert st["prefiltered"] is False and st["bg"].shape == (3,) and st["viewmatrix"].shape == (4, 4)
        assert (kw["shs"] is None) != (kw["colors_precomp"] is None)
        assert (kw["scales"] is None) == (kw["rotations"] is None) != (kw["cov3D_precomp"] is None)
        assert kw["opacities"].shape == (P, 1)
        if name.startswith("render_kernel"):
            # sh_degree = the model's MAX degree (make_rasterizer(viewpoint_camera, pc.max_sh_degree, ...)), debug from cfg
            assert st["sh_degree"] == 3 and st["debug"] is False
            if "train" in name:
                # screen-space points: a [P, 3] zero tensor that requires grad (its .grad feeds the densification statistics)
                assert kw["means2D"].shape == (P, 3) and not kw["means2D"].any() and "means2D" in meta["requires_grad"]
            else:
                assert kw["means2D"] is None and kw["semantics"] is None
        if name == "render_kernel_train_normals_semantics":
            assert kw["semantics"].shape == (P, 3 + 16)  # cat(normals [P,3], semantic logits [P,16]) along dim -1
            assert torch.allclose(kw["semantics"][:, :3].norm(dim=1), torch.ones(P), atol=1e-5)
        if name == "render_kernel_train_python_sh_cov":
            assert kw["colors_precomp"].shape == (P, 3) and (kw["colors_precomp"] >= 0).all()  # clamp_min(sh2rgb + 0.5, 0)
            assert kw["cov3D_precomp"].shape == (P, 6)
        if name == "render_kernel_train_python_sh":
            # convert_SHs_python alone: colours from eval_sh, the covariance left to the rasterizer
            assert kw["colors_precomp"].shape == (P, 3) and (kw["colors_precomp"] >= 0).all()
            assert kw["scales"].shape == (P, 3) and kw["rotations"].shape == (P, 4) and st["scale_modifier"] == 1.0
        if name == "render_kernel_train_python_cov_mod06":
            # compute_cov3D_python alone: SH rows go down, cov3D_precomp = get_covariance(scaling_modifier) already holds
            # the modifier -- and the SAME modifier is in the settings, where the rasterizer must ignore it
            assert kw["shs"].shape == (P, 16, 3) and kw["cov3D_precomp"].shape == (P, 6) and st["scale_modifier"] == 0.6
        if name == "render_kernel_train_override_color_mod15":
            # override_color wins over SH; scales / rotations with scaling_modifier = 1.5 in the settings; normals only
            assert kw["colors_precomp"].shape == (P, 3) and kw["shs"] is None and kw["scales"].shape == (P, 3)
            assert st["scale_modifier"] == 1.5 and kw["semantics"].shape == (P, 3) and bool((st["bg"] == 1).all())
        if name.startswith("smoke_script"):
            # degree 0 with FOUR coefficients per Gaussian (M > (D+1)^2), un-normalised quaternions, debug=True
            assert st["sh_degree"] == 0 and kw["shs"].shape == (P, 4, 3) and st["debug"] is True and P == 10000
            assert (kw["rotations"][:, 0] == 1).all()


@pytest.mark.parametrize("name", ["smoke_script_call2_sem15", "render_kernel_train_python_sh_cov", "render_kernel_train_python_sh",
                                  "render_kernel_train_python_cov_mod06", "render_kernel_train_override_color_mod15"])
def test_oracle_runs_the_captured_call(name):
    st, kw, meta = mk.load(os.path.join(HERE, "golden", "callsite", name + ".npz"))
    fw = oracle.forward(means3D=kw["means3D"], opacities=kw["opacities"], viewmatrix=st["viewmatrix"],
                        projmatrix=st["projmatrix"], campos=st["campos"], bg=st["bg"], tanfovx=st["tanfovx"],
                        tanfovy=st["tanfovy"], image_height=st["image_height"], image_width=st["image_width"],
                        sh_degree=st["sh_degree"], scale_modifier=st["scale_modifier"], shs=kw["shs"],
                        colors_precomp=kw["colors_precomp"], scales=kw["scales"], rotations=kw["rotations"],
                        cov3D_precomp=kw["cov3D_precomp"], semantics=kw["semantics"])
    assert fw.num_rendered > 0 and np.isfinite(fw.color).all() and fw.color.shape == (3, st["image_height"], st["image_width"])
    assert fw.semantic.shape[0] == kw["semantics"].shape[1]
    assert (fw.alpha >= 0).all() and fw.alpha.max() <= 1.0 + 1e-5
    fw.free()
