"""CPU tests of the per-frame actor poses' host side (street_gaussians_amd/actor_pose.py, include/sgr_actor_pose.h):
(a) where /root/reference exists the fixture (tests/golden/make_actor_pose_fixture.py) is regenerated from its source and
must reproduce the committed file bit for bit, (b) the fixture's own figures and edge cases are recomputed from its arrays,
(c) the host plan chooses exactly the indices and camera timestamps the reference chose, on every case, and its weights
are the float64 differences rounded once, (d) the torch restatement (tests/torch_ref_actor_pose.py) is within the gate in
float32 and float64, values and gradients, (e) the record layout of the header and of the binding agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torch_ref_actor_pose as rp
from golden import make_actor_pose_fixture as mk
from street_gaussians_amd import actor_pose
from street_gaussians_amd.actor_pose import ActorPoses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pins():
    assert os.path.exists(mk.OUT), "tests/golden/actor_pose/pins.npz is not committed"
    return mk.load()


def _actor_poses(c):
    t = lambda k: torch.from_numpy(c[k].copy())
    opt = bool(c["opt_track"])
    ot = t("opt_trans").requires_grad_(True) if opt else None
    orr = t("opt_rots").requires_grad_(True) if opt else None
    info = {int(i): dict(start_timestamp=float(s), end_timestamp=float(e))
            for i, s, e in zip(c["obj_ids"], c["obj_start"], c["obj_end"])}
    return ActorPoses(c["track_ids"], t("input_trans"), t("input_rots"), c["timestamps"],
                      {0: {"train_timestamps": list(c["cam_ts"])}}, info, opt_trans=ot, opt_rots=orr)


def _plan(ap, c):
    return ap.plan([int(i) for i in c["ids"]], float(c["timestamp"]), 0, is_val=bool(c["is_val"]))


@pytest.mark.skipif(not os.path.exists("/root/reference/lib/models/actor_pose.py"),
                    reason="reference checkout not present on this machine")
def test_regenerating_from_the_reference_source_reproduces_the_fixture(pins):
    d = mk.build()
    assert sorted(d) == sorted(pins)
    for k in d:
        a, b = np.asarray(d[k]), pins[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k


def test_fixture_holds_what_it_says(pins):
    d = pins
    assert os.path.getsize(mk.OUT) < 1 << 20
    names = [str(n) for n in d["names"]]
    e_ref = {k: 0.0 for k in mk.KINDS}
    for name in names:
        c = mk.case(d, name)
        for k in mk.KINDS:
            if k + "64" in c:
                assert c[k + "32"].dtype == np.float32 and c[k + "64"].dtype == np.float64
                err = np.abs(c[k + "32"].astype(np.float64) - c[k + "64"]) / mk.scale_of(k, c[k + "64"])
                e_ref[k] = max(e_ref[k], float(err.max()))
                assert mk.gate(k, c[k + "32"], c[k + "64"], float(d["e_ref_" + k]))[0]
        assert ("dtrans64" in c) == bool(c["opt_track"])
    for k in mk.KINDS:
        assert e_ref[k] == float(d["e_ref_" + k])
        assert 0 < e_ref[k] < 2e-6  # a few float32 ulps: anything larger means a case cancels and hides the rest
    # the edges the cases are there for
    c = mk.case(d, "on_entry")
    assert (c["timestamps"] == c["timestamp"]).any()
    c = mk.case(d, "tie")
    f1, f2 = c["idx"][0, 0, 0], c["idx"][0, 0, 2]
    assert abs(c["timestamps"][f1] - c["timestamp"]) == abs(c["timestamps"][f2] - c["timestamp"])
    assert mk.case(d, "before")["timestamp"] < mk.case(d, "before")["timestamps"].min()
    assert mk.case(d, "after")["timestamp"] > mk.case(d, "after")["timestamps"].max()
    c = mk.case(d, "offset")
    assert c["timestamps"].min() >= 1.5e9 and np.allclose(np.diff(c["timestamps"]), 0.1, atol=1e-6)
    assert not mk.case(d, "theta_zero")["opt_rots"].any() and mk.case(d, "theta_zero")["drots64"].any()
    assert (mk.case(d, "theta_flip")["opt_rots"] > 2.4).all()  # cos(theta2) < 0: the shortest-arc sign flip
    n = np.linalg.norm(mk.case(d, "mid_opt")["input_rots"].astype(np.float64), axis=-1)
    assert n.min() < 0.8 and n.max() > 1.5  # far from unit length
    c = mk.case(d, "antipodal_noopt")
    qa, qb = c["input_rots"][1, 1].astype(np.float64), c["input_rots"][2, 0].astype(np.float64)
    assert (qa * qb).sum() / np.linalg.norm(qa) / np.linalg.norm(qb) < -0.99999
    assert (mk.case(d, "val_two")["n_samples"] == 2).all() and np.isfinite(mk.case(d, "val_two")["outer_ts"]).all()
    assert (mk.case(d, "val_fallback")["n_samples"] == 1).all() and np.isnan(mk.case(d, "val_fallback")["outer_ts"]).all()
    assert (mk.case(d, "val_noopt")["n_samples"] == 1).all()
    assert len(mk.case(d, "k65")["ids"]) == 65 and mk.case(d, "k65")["track_ids"].shape == (4, 70)
    assert len(mk.case(d, "k1")["ids"]) == 1
    # each candidate of matrix_to_quaternion wins once
    for i, name in enumerate(("ego_w", "ego_x", "ego_y", "ego_z")):
        R = mk.case(d, name)["ego"][:3, :3].astype(np.float64)
        dd = [1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
              1 - R[0, 0] - R[1, 1] + R[2, 2]]
        assert int(np.argmax(dd)) == i


def test_plan_chooses_the_references_indices_exactly(pins):
    for name in (str(n) for n in pins["names"]):
        c = mk.case(pins, name)
        ap = _actor_poses(c)
        plan = _plan(ap, c)
        O = c["track_ids"].shape[1]
        assert np.array_equal(plan.records["n_samples"], c["n_samples"]), name
        cells, idx = plan.cells(), c["idx"].astype(np.int64)
        stamps, t = c["timestamps"], float(c["timestamp"])
        for k in range(len(plan)):
            rec = plan.records[k]
            outer = c["outer_ts"][k]
            if rec["n_samples"] == 2:
                T1, T2 = outer
                want_t = (T1, T2)
                assert (rec["Wa"], rec["Wb"], rec["Wd"], rec["R"]) == tuple(
                    np.float32(x) for x in (T2 - t, t - T1, T2 - T1, (t - T1) / (T2 - T1))), (name, k)
            else:
                want_t = (t,)
            for s, ts in enumerate(want_t):
                f1, c1, f2, c2 = idx[k, s]
                assert tuple(cells[k, s]) == (f1 * O + c1, f2 * O + c2, f1 * O + c1, f1 * O + c2), (name, k, s)
                t1, t2 = stamps[f1], stamps[f2]
                w = rec["s"][s]
                assert (w["wa"], w["wb"], w["wd"], w["r"]) == tuple(
                    np.float32(x) for x in (t2 - ts, ts - t1, t2 - t1, (ts - t1) / (t2 - t1))), (name, k, s)
    # a large common offset keeps the differences: 0.03 s after an entry at 1.5e9 s
    c = mk.case(pins, "offset")
    w = _plan(_actor_poses(c), c).records["s"][0, 0]
    assert abs(float(w["wb"]) - 0.03) < 1e-6 and abs(float(w["wd"]) - 0.1) < 1e-6


def test_plan_rejects_unknown_and_short_tracks(pins):
    c = mk.case(pins, "mid_opt")
    ap = _actor_poses(c)
    with pytest.raises(ValueError, match="obj_info"):
        ap.plan([0, 99], 10.2, 0)
    ids = c["track_ids"].copy()
    ids[ids == 2] = -1
    ids[1, 2] = 2  # one entry only
    c2 = dict(c, track_ids=ids)
    with pytest.raises(ValueError, match="two are needed"):
        _actor_poses(c2).plan([2], 10.2, 0)
    with pytest.raises(ValueError):
        ActorPoses(c["track_ids"], torch.zeros(5, 3, 3), torch.zeros(5, 3, 4), c["timestamps"], {}, {},
                   opt_trans=torch.zeros(5, 3, 3))
    assert len(ap.plan([], 10.2, 0)) == 0


def test_restatement_is_within_the_gate(pins):
    """Values and autograd gradients of tests/torch_ref_actor_pose.py against the reference's float64, in both dtypes.
    Measured here: float32 needs at most 1.0 x e_ref, float64 at most 0.67 x (its weights are the record's float32)."""
    need = {}
    for name in (str(n) for n in pins["names"]):
        c = mk.case(pins, name)
        ap = _actor_poses(c)
        plan = _plan(ap, c)
        t = lambda k: torch.from_numpy(c[k].copy())
        for dt in (torch.float32, torch.float64):
            if ap.opt_track:
                ap.opt_trans.grad = ap.opt_rots.grad = None
            out = rp.poses(plan.records, t("input_trans"), t("input_rots"), ap.opt_trans, ap.opt_rots, t("ego"), dt)
            assert out.dtype == dt
            res = {"rot": out[:, :4].detach().numpy(), "trans": out[:, 4:].detach().numpy()}
            if ap.opt_track:
                (out * t("g").to(dt)).sum().backward()
                res["dtrans"], res["drots"] = ap.opt_trans.grad.numpy(), ap.opt_rots.grad.numpy()
            for k, v in res.items():
                assert np.isfinite(v).all(), (name, k)
                ok, f = mk.gate(k, v, c[k + "64"], float(pins["e_ref_" + k]), c[k + "32"] if k[0] == "d" else None)
                need[(k, dt)] = max(need.get((k, dt), 0.0), f)
                assert ok, (name, k, dt, f)
    print({f"{k} {str(dt)[-2:]}": round(v, 3) for (k, dt), v in need.items()})
    assert max(need.values()) <= 2.0  # room to spare under the factor 4


def test_record_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "sgr_actor_pose.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype = {"int32_t": C.c_int32, "float": C.c_float}

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
        out = []
        for decl in (x.strip() for x in body.split(";") if x.strip()):
            ty, rest = decl.split(None, 1)
            for nm in (x.strip() for x in rest.split(",")):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", nm)
                out.append((m.group(1), ty, int(m.group(2)) if m.group(2) else None))
        return out

    def check(struct, cls, size):
        want = fields(struct)
        assert [f[0] for f in cls._fields_] == [w[0] for w in want]
        for (nm, ty), (_, cty, n) in zip(cls._fields_, want):
            base = actor_pose._CSample if cty == "sgr_actor_pose_sample" else ctype[cty]
            assert ty is (base * n if n else base) or (n and ty._type_ is base and ty._length_ == n), nm
        assert C.sizeof(cls) == size
        assert re.search(r"\} %s;\s*/\* %d bytes \*/" % (struct, size), text)

    check("sgr_actor_pose_sample", actor_pose._CSample, 32)
    check("sgr_actor_pose_record", actor_pose._CRecord, 96)
    assert actor_pose.RECORD_DTYPE.itemsize == 96
    off = {n: actor_pose.RECORD_DTYPE.fields[n][1] for n in actor_pose.RECORD_DTYPE.names}
    assert off == {"s": 0, "Wa": 64, "Wb": 68, "Wd": 72, "R": 76, "n_samples": 80, "pad": 84}
    for name, val in (("SGR_ACTOR_POSE_CONTRIB", actor_pose.CONTRIB), ("SGR_ACTOR_POSE_PARTS", actor_pose.PARTS)):
        assert int(re.search(r"#define %s (\d+)" % name, code).group(1)) == val
