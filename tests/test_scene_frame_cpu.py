"""CPU tests of the per-frame compose (include/sgr_scene_frame.h): the torch restatement (tests/torch_ref_scene_frame.py)
is pinned bit for bit against the reference's own PoseCorrection.correct_gaussian_xyz / correct_gaussian_rotation and
against its get_xyz / get_rotation with use_pose_correction = True on frame subsets -- live where the reference checkout
is present, else against the outputs recorded in tests/golden/scene_frame/pins.npz --, its gradients are checked in
float64, and the library must export the new entry points."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import torch_ref_scene_frame as fref
from golden.refpin import RECORD, reference_path
from test_scene_cpu import GU, _getters, _reference_fn, _segments

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PINS = os.path.join(HERE, "golden", "scene_frame", "pins.npz")
CP = "lib/models/camera_pose.py"
SGM = "lib/models/street_gaussian_model.py"
GMP = "lib/models/gaussian_model.py"
GMA = "lib/models/gaussian_model_actor.py"

# Refresh the record where the reference is present:
#     SGR_RECORD_REFERENCE_OUTPUTS=1 python -m pytest tests/test_scene_frame_cpu.py


class _Pins:
    """What the reference's code returned: live where its source is present (and the record must still agree), else
    the record.  Outputs are compared bit for bit."""

    def __init__(self, prefix, *required):
        self.prefix = prefix
        self.live = all(os.path.exists(reference_path(p)) for p in required)
        self.stored = dict(np.load(PINS)) if os.path.exists(PINS) else {}
        self.seen = {}
        if not self.live:
            assert any(k.startswith(prefix + ":") for k in self.stored), f"no recorded outputs for {prefix} in {PINS}"

    def equal(self, name, mine, fn):
        key = f"{self.prefix}:{name}"
        if self.live:
            theirs = fn()
            assert torch.equal(mine, theirs), key
            a = theirs.detach().contiguous().numpy()
            self.seen[key] = a
            if not RECORD:
                b = self.stored.get(key)
                assert b is not None and b.dtype == a.dtype and b.shape == a.shape and b.tobytes() == a.tobytes(), \
                    f"{PINS} is stale for {key} (re-record it)"
            return
        assert torch.equal(mine, torch.from_numpy(self.stored[key])), key

    def close(self):
        if RECORD and self.live:
            data = dict(np.load(PINS)) if os.path.exists(PINS) else {}
            data.update(self.seen)
            os.makedirs(os.path.dirname(PINS), exist_ok=True)
            np.savez(PINS, **data)


def _camera_pose_methods(cfg):
    ns = {"torch": torch, "cfg": cfg, "quaternion_raw_multiply": _reference_fn("quaternion_raw_multiply"),
          "quaternion_to_matrix": _reference_fn("quaternion_to_matrix"), "Camera": object}  # Camera: an annotation
    return _getters(CP, ["get_id", "correct_gaussian_xyz", "correct_gaussian_rotation"], ns, prop=False)


def _pose_correction(cfg, rots, trans):
    """A PoseCorrection stand-in running the reference's own methods (mode 'image': the id is camera.id)."""
    pc = types.SimpleNamespace(mode="image", pose_correction_rots=rots, pose_correction_trans=trans)
    for name, fn in _camera_pose_methods(cfg).items():
        setattr(pc, name, types.MethodType(fn, pc))
    return pc


def _corrections(g):
    """Three raw (not normalised) per-image corrections: a generic one, one near the identity, one far from unit norm."""
    rots = torch.stack([torch.randn(4, generator=g), torch.tensor([1.0, 1e-3, -2e-3, 5e-4]), torch.randn(4, generator=g) * 7])
    trans = torch.randn(3, 3, generator=g)
    return rots, trans


def test_restated_correction_matches_the_reference_methods():
    pin = _Pins("correction", CP, GU)
    g = torch.Generator().manual_seed(21)
    rots, trans = _corrections(g)
    xyz, rot = torch.randn(57, 3, generator=g) * 20, torch.nn.functional.normalize(torch.randn(57, 4, generator=g))
    cfg = types.SimpleNamespace(mode="train")
    pc = _pose_correction(cfg, rots, trans) if pin.live else None
    for cid in range(3):
        c = torch.cat([rots[cid], trans[cid]])
        cam = types.SimpleNamespace(id=cid)
        pin.equal(f"xyz{cid}", fref.correct_xyz(c, xyz), lambda: pc.correct_gaussian_xyz(cam, xyz))
        pin.equal(f"rotation{cid}", fref.correct_rotation(c, rot), lambda: pc.correct_gaussian_rotation(cam, rot))
    pin.close()


@pytest.mark.parametrize("case", ["background+obj_1", "actors_only"])
def test_restated_frame_matches_the_reference_getters_with_pose_correction(case):
    """get_xyz / get_rotation of the reference with use_pose_correction = True, on a frame whose graph_obj_list is a
    subset of the persistent actors (or whose background is not visible: the render_object pass)."""
    pin = _Pins(f"frame.{case}", CP, SGM, GMP, GMA, GU)
    S, M = 3, 4
    g = torch.Generator().manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=g)
    cfg = types.SimpleNamespace(mode="train")
    if pin.live:
        ns = {"torch": torch, "cfg": cfg, "quaternion_raw_multiply": _reference_fn("quaternion_raw_multiply"),
              "quaternion_to_matrix": _reference_fn("quaternion_to_matrix"), "GaussianModel": object,
              "GaussianModelActor": object}
        Base = type("Base", (), _getters(GMP, ["get_rotation", "get_xyz"], dict(ns)))
        Street = type("Street", (), _getters(SGM, ["get_rotation", "get_xyz"], dict(ns)))
    else:
        Base = Street = type("Stub", (), {})

    def model(n):
        m = Base()
        m._xyz, m._rotation = r(n, 3) * 5, r(n, 4)
        m.rotation_activation = torch.nn.functional.normalize
        return m
    bk, actors = model(30), [model(11), model(7), model(5)]
    poses = [r(7) for _ in actors]
    masks = [torch.rand(a._xyz.shape[0], generator=g) < 0.5 for a in actors]
    rots, trans = _corrections(g)
    cid = 2
    c = torch.cat([rots[cid], trans[cid]])
    frame = [1] if case == "actors_only" else [0, 2]  # indices into `actors`
    st = Street()
    st.background = bk
    st.get_visibility = (lambda name: name != "background") if case == "actors_only" else (lambda name: True)
    st.graph_obj_list = [f"obj_{k}" for k in frame]
    for k, a in enumerate(actors):
        setattr(st, f"obj_{k}", a)
    st.use_pose_correction = True
    st.viewpoint_camera = types.SimpleNamespace(id=cid)
    st.pose_correction = _pose_correction(cfg, rots, trans) if pin.live else None
    st.obj_rots = torch.cat([poses[k][:4].unsqueeze(0).expand(actors[k]._xyz.shape[0], -1) for k in frame], 0)
    st.obj_trans = torch.cat([poses[k][4:].unsqueeze(0).expand(actors[k]._xyz.shape[0], -1) for k in frame], 0)
    st.flip_mask = torch.cat([masks[k] for k in frame], 0)
    st.flip_axis = 1
    st.flip_matrix = torch.tensor([[0.0, 0.0, 1.0, 0.0]])

    def seg(m, **kw):
        n = m._xyz.shape[0]
        return dict(xyz=m._xyz, rotation=m._rotation, scaling=torch.zeros(n, 3), opacity=torch.zeros(n, 1),
                    features_dc=torch.zeros(n, 1, 3), features_rest=torch.zeros(n, M - 1, 3), **kw)
    models = [seg(bk)] + [seg(a, pose=p, flip_mask=fm) for a, p, fm in zip(actors, poses, masks)]
    segments = ([] if case == "actors_only" else [0]) + [1 + k for k in frame]
    xyz, rot = fref.compose_frame(models, M, S, segments=segments, correction=c)[:2]
    pin.equal("xyz", xyz, lambda: st.get_xyz)
    pin.equal("rotation", rot, lambda: st.get_rotation)
    pin.close()


def test_restatement_gradcheck_with_subset_poses_and_correction():
    models = _segments(dtype=torch.float64, S=3, M=4, seed=5)
    g = torch.Generator().manual_seed(6)
    corr = torch.cat([torch.randn(4, generator=g, dtype=torch.float64) * 2, torch.randn(3, generator=g, dtype=torch.float64)])
    corr.requires_grad_(True)
    poses = torch.randn(1, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    bk = {k: (v.clone().requires_grad_(True) if k in ("xyz", "rotation") else v) for k, v in models[0].items()}
    models[0] = bk

    def fn(c, p, x, q):
        ms = [dict(models[0], xyz=x, rotation=q)] + models[1:]
        return fref.compose_frame(ms, 4, 3, segments=[2, 0], poses=p, correction=c)[:2]
    assert torch.autograd.gradcheck(fn, (corr, poses, bk["xyz"], bk["rotation"]), eps=1e-6, atol=1e-5)
    # correction off and the full frame: the per-model restatement unchanged
    full = fref.compose_frame(models, 4, 3)
    import torch_ref_scene as ref
    for a, b in zip(full, ref.compose(models, 4, 3)):
        assert torch.equal(a, b)


def test_frame_abi_symbols_are_exported():
    from street_gaussians_amd import _native
    decl = open(os.path.join(ROOT, "include", "sgr_scene_frame.h")).read()
    names = re.findall(r"^int (sgr_scene_\w+)\(", decl, re.M)
    assert names == ["sgr_scene_compose_forward_ex", "sgr_scene_compose_backward_ex"]
    assert set(names) <= set(_native.SYMBOLS)
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libsgr_hip.so not built")
    L = C.CDLL(_native.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n


def test_flat_compose_rejects_a_repeated_or_unknown_segment_before_any_gpu_work():
    """FlatScene.compose validates `segments` on the host (a model's rows cannot be composed twice in one frame)."""
    from street_gaussians_amd.scene import FlatScene, Segment
    r = lambda *s: torch.randn(*s)
    segs = [Segment(r(4, 3), r(4, 4), r(4, 3), r(4, 1), r(4, 1, 3), r(4, 3, 3)),
            Segment(r(2, 3), r(2, 4), r(2, 3), r(2, 1), r(2, 1, 3), r(2, 3, 3), pose=r(7))]
    flat = FlatScene.from_segments(segs)
    with pytest.raises(ValueError, match="at most once"):
        flat.compose(4, 0, segments=[0, 1, 1])
    with pytest.raises(ValueError, match="out of range"):
        flat.compose(4, 0, segments=[2])
    with pytest.raises(ValueError, match=r"\[1, 7\]"):
        flat.compose(4, 0, segments=[1], poses=torch.zeros(2, 7))
