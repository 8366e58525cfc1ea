"""Pins the per-frame actor poses to the reference's own Python and writes tests/golden/actor_pose/pins.npz.

Cut out of the reference's files when this runs and executed here (no GPU), nothing of their text kept: the methods of
``ActorPose`` that choose indices and interpolate (lib/models/actor_pose.py:83-173), the pose lines of ``parse_camera``
(lib/models/street_gaussian_model.py:260-265), and ``quaternion_raw_multiply``, ``quaternion_raw_multiply_theta``,
``quaternion_slerp``, ``matrix_to_quaternion``, ``_sqrt_positive_part`` (lib/utils/general_utils.py).  The only textual
changes are ``.cuda()`` and ``.float()`` -> ``.to(torch.get_default_dtype())``, so that the same text also runs in
float64.  ``roma`` is not a dependency of this project: ``quaternion_slerp``'s two ``roma.utils`` functions (the same
function up to rounding) are replaced by ``unitquat_slerp`` below, written from the closed form
q0 (x) exp(step * log(q0* (x) q1)) with the shortest arc.  The rotation interpolation is therefore pinned to that
definition; everything else -- index choice, both opt_track behaviours, the z-rotation factor, the lerp, the ego
composition, matrix_to_quaternion -- is pinned to the reference's executed text.

Each case is one frame of one scene, evaluated in float32 (what the reference computes) and in float64 on the same
float32 inputs, values and autograd gradients of sum(poses * g).  Run where /root/reference exists:

    python tests/golden/make_actor_pose_fixture.py

Keys of the file, per case ``<name>/``: inputs ``track_ids`` [F,O] int32 (-1 = empty), ``input_trans`` [F,O,3],
``input_rots`` [F,O,4] (w,x,y,z; NOT unit), ``timestamps`` [F] f64, ``cam_ts`` [n] f64 (the camera's train timestamps),
``obj_ids`` / ``obj_start`` / ``obj_end``, ``opt_track``, ``opt_trans`` / ``opt_rots`` (initial values), ``ids`` [K] (the
frame's actors in order), ``timestamp``, ``is_val``, ``ego`` [4,4], ``g`` [K,7]; what the reference chose: ``n_samples``
[K], ``idx`` [K,2,4] (frame1, column1, frame2, column2 of each sample's find_closest_indices; -1 where there is no second
sample), ``outer_ts`` [K,2] (find_closest_camera_timestamps, NaN where None); outputs ``rot32/64`` [K,4], ``trans32/64``
[K,3] and, with opt_track, ``dtrans32/64`` [F,O,3], ``drots32/64`` [F,O,1].  Global: ``names``, and ``e_ref_rot``,
``e_ref_trans``, ``e_ref_dtrans``, ``e_ref_drots`` = max over all cases of |ref_f32 - ref_f64| / scale; scale = the largest
|ref_f64| of the actor's own quaternion / translation for the outputs, of the case's whole tensor for a gradient.
"""
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden import make_callsite_fixture as mk  # noqa: E402

OUT = os.path.join(HERE, "actor_pose", "pins.npz")
REF = mk.REF
FACTOR = 4.0  # the gate is FACTOR * e_ref * scale (tests/golden/actor_pose/README.md)
KINDS = ("rot", "trans", "dtrans", "drots")
METHODS = ("find_closest_indices", "find_closest_camera_timestamps", "get_tracking_translation_",
           "get_tracking_translation", "get_tracking_rotation_", "get_tracking_rotation")
FUNCS = ("_sqrt_positive_part", "matrix_to_quaternion", "quaternion_raw_multiply", "quaternion_raw_multiply_theta",
         "quaternion_slerp")


# ---- the stand-in for roma.utils.unitquat_slerp / unitquat_slerp_fast (x, y, z, w) ------------------------------------
def _prod_xyzw(p, q):
    px, py, pz, pw = p.unbind(-1)
    qx, qy, qz, qw = q.unbind(-1)
    return torch.stack((pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
                        pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz), -1)


def _half_sinc(angle):
    """sin(angle / 2) / angle, by its series below 1e-3; the branch not taken is evaluated at 1."""
    small = angle.abs() < 1e-3
    safe = torch.where(small, torch.ones_like(angle), angle)
    return torch.where(small, 0.5 - angle ** 2 / 48, torch.sin(0.5 * safe) / safe)


def _norm(v):
    sq = (v * v).sum(-1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def unitquat_slerp(q0, q1, steps, shortest_arc=True):
    """q0 (x) exp(step * log(conj(q0) (x) q1)) for unit q0, q1 [B, 4] and steps [S] -> [S, B, 4]."""
    rel = _prod_xyzw(q0 * q0.new_tensor([-1.0, -1.0, -1.0, 1.0]), q1)
    if shortest_arc:
        rel = torch.where(rel[..., 3:] < 0, -rel, rel)
    angle = 2 * torch.atan2(_norm(rel[..., :3]), rel[..., 3])
    rotvec = rel[..., :3] / _half_sinc(angle)[..., None]
    rv = steps.reshape(-1, 1, 1) * rotvec[None]
    a = _norm(rv)
    e = torch.cat([rv * _half_sinc(a)[..., None], torch.cos(0.5 * a)[..., None]], -1)
    return _prod_xyzw(q0[None].expand_as(e), e)


# ---- the reference's text ----------------------------------------------------------------------------------------------
def _retype(src):
    return src.replace(".float()", ".to(torch.get_default_dtype())")


def reference_namespace(mode="train"):
    """-> (namespace with the cut-out functions, the ActorPose methods as a dict, the pose lines of parse_camera as a
    function (self, track_id) -> (obj_rot, obj_trans))."""
    cfg = types.SimpleNamespace(mode=mode)
    roma = types.SimpleNamespace(utils=types.SimpleNamespace(unitquat_slerp=unitquat_slerp, unitquat_slerp_fast=unitquat_slerp))
    ns = {"torch": torch, "np": np, "F": torch.nn.functional, "roma": roma, "Camera": object, "cfg": cfg}
    gu = os.path.join(REF, "lib/utils/general_utils.py")
    for name in FUNCS:
        exec(_retype(mk._func(gu, name)), ns)
    ap = os.path.join(REF, "lib/models/actor_pose.py")
    methods = {}
    for name in METHODS:
        exec(_retype(mk._func(ap, name, method=True)), ns)
        methods[name] = ns[name]
    src = open(os.path.join(REF, "lib/models/street_gaussian_model.py")).read()
    m = re.search(r"^( +)obj_rot = self\.actor_pose\.get_tracking_rotation\(.*?"
                  r"obj_trans = ego_pose\[:3, :3\] @ obj_trans \+ ego_pose\[:3, 3\][^\n]*\n", src, re.S | re.M)
    assert m, "parse_camera's pose lines"
    ind = len(m.group(1))
    body = "\n".join("    " + ln[ind:] for ln in m.group(0).rstrip("\n").split("\n"))
    exec("def world_pose(self, track_id):\n" + mk._nocuda(body) + "\n    return obj_rot, obj_trans\n", ns)
    return ns, methods, ns["world_pose"], cfg


# ---- cases -------------------------------------------------------------------------------------------------------------
SMALL = np.array([[0, 1, -1], [1, 0, 2], [0, 2, 1], [-1, 0, 1], [1, 0, 2]], np.int32)  # columns move between frames


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _ego(R, t=(12.5, -3.25, 1.75)):
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, t
    return E.astype(np.float32)


EGO_GENERIC = _ego(_rot((0.2, -0.5, 1.0), 0.8))
EGOS = {"ego_w": _ego(np.eye(3), (0.0, 0.0, 0.0)),  # each candidate of matrix_to_quaternion wins once
        "ego_x": _ego(_rot((0, 1, 0), 1e-3) @ _rot((1, 0, 0), np.pi)),
        "ego_y": _ego(_rot((0, 0, 1), 1e-3) @ _rot((0, 1, 0), np.pi)),
        "ego_z": _ego(_rot((1, 0, 0), 1e-3) @ _rot((0, 0, 1), np.pi))}


def _scene(rng, ids_table, stamps):
    F, O = ids_table.shape
    q = rng.standard_normal((F, O, 4))
    q = q / np.sqrt((q * q).sum(-1, keepdims=True)) * rng.uniform(0.5, 2.0, (F, O, 1))  # non-unit on purpose
    ids = sorted(int(i) for i in np.unique(ids_table) if i >= 0)
    fr = {i: np.nonzero((ids_table == i).any(1))[0] for i in ids}
    return dict(track_ids=ids_table.astype(np.int32), input_trans=(10.0 * rng.standard_normal((F, O, 3))).astype(np.float32),
                input_rots=q.astype(np.float32), timestamps=np.asarray(stamps, np.float64),
                obj_ids=np.asarray(ids, np.int32), obj_start=np.asarray([stamps[fr[i][0]] for i in ids], np.float64),
                obj_end=np.asarray([stamps[fr[i][-1]] for i in ids], np.float64))


def make_cases():
    """Seeded inputs made of draws and exactly rounded operations only, so they are the same everywhere."""
    rng = np.random.default_rng(20241017)
    cases = {}

    def add(name, sc, ids, t, opt=True, theta="rand", is_val=False, cam_ts=(), ego=EGO_GENERIC):
        F, O = sc["track_ids"].shape
        c = dict(sc)
        c["opt_track"] = np.bool_(opt)
        th = {"rand": rng.uniform(-0.3, 0.3, (F, O, 1)), "zero": np.zeros((F, O, 1)),
              "flip": 2.5 + rng.uniform(-0.05, 0.05, (F, O, 1))}[theta]
        c["opt_rots"] = th.astype(np.float32)
        c["opt_trans"] = (np.zeros((F, O, 3)) if theta == "zero" else rng.uniform(-0.1, 0.1, (F, O, 3))).astype(np.float32)
        c["ids"] = np.asarray(ids, np.int32)
        c["timestamp"], c["is_val"] = np.float64(t), np.bool_(is_val)
        c["cam_ts"] = np.asarray(cam_ts, np.float64)
        c["ego"] = ego
        c["g"] = rng.standard_normal((len(ids), 7)).astype(np.float32)
        cases[name] = c

    ts = 10.0 + 0.125 * np.arange(5)  # exact in binary: the midpoint of two entries is an exact tie
    small = _scene(rng, SMALL, ts)
    add("mid_opt", small, [0, 1, 2], ts[1] + 0.04)            # every (f1, c2) cell is another actor's cell
    add("mid_noopt", small, [0, 1, 2], ts[1] + 0.04, opt=False)
    add("late_opt", small, [1, 0, 2], ts[3] + 0.04)           # track 1's (f1, c2) cell is empty
    add("on_entry", small, [0, 1, 2], ts[2])
    add("tie", small, [0, 1, 2], 0.5 * (ts[1] + ts[2]))
    add("before", small, [0, 1, 2], ts[0] - 0.07)
    add("after", small, [0, 1, 2], ts[4] + 0.13)
    add("theta_zero", small, [0, 1, 2], ts[2] + 0.03, theta="zero")
    add("theta_flip", small, [0, 1, 2], ts[2] + 0.03, theta="flip")
    anti = dict(small)
    q = anti["input_rots"].astype(np.float64).copy()
    q[2, 0] = -q[1, 1] * 1.25 + 2e-3 * rng.standard_normal(4)  # track 0, frames 1 -> 2: a near-antipodal pair
    anti["input_rots"] = q.astype(np.float32)
    add("antipodal_noopt", anti, [0, 1], ts[1] + 0.05, opt=False)
    off = _scene(rng, SMALL, 1.5e9 + 0.1 * np.arange(5))
    add("offset", off, [0, 1, 2], off["timestamps"][2] + 0.03)
    for name, ego in EGOS.items():
        add(name, small, [0, 2], ts[2] + 0.03, ego=ego)
    cam = ts[0] + 0.05 + 0.1 * np.arange(6)
    add("val_two", small, [0, 1, 2], ts[2] + 0.02, is_val=True, cam_ts=cam)
    add("val_fallback", small, [0, 1, 2], ts[2] + 0.02, is_val=True, cam_ts=[ts[2] + 0.01])
    add("val_noopt", small, [0, 1], ts[2] + 0.02, opt=False, is_val=True, cam_ts=cam)
    add("k1", small, [1], ts[0] + 0.03)
    wide = np.full((4, 70), -1, np.int32)
    wide[:, :65] = 100 + np.arange(65)[None]                  # constant columns: theta1 and theta2 share their cell
    wide[0, 3] = wide[3, 7] = -1
    add("k65", _scene(rng, wide, 3.0 + 0.1 * np.arange(4)), 100 + np.arange(65), 3.0 + 0.1 * 1 + 0.037)
    return cases


# ---- evaluation ----------------------------------------------------------------------------------------------------------
def evaluate_case(c, dt):
    """The reference's text on one case in dtype ``dt`` -> dict(rot, trans[, dtrans, drots], idx, n_samples, outer_ts)."""
    ns, methods, world_pose, cfg = reference_namespace()
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    # quaternion_slerp imports cfg from lib.config when it is called
    held = {k: sys.modules.get(k) for k in ("lib", "lib.config")}
    sys.modules["lib"] = types.ModuleType("lib")
    sys.modules["lib.config"] = types.ModuleType("lib.config")
    sys.modules["lib.config"].cfg = cfg
    try:
        calls, outer = [], []

        def find_closest_indices(self, track_id, timestamp):
            r = methods["find_closest_indices"](self, track_id, timestamp)
            calls.append([int(x) for x in (*r[0], *r[1])])
            return r

        def find_closest_camera_timestamps(self, track_id, camera):
            r = methods["find_closest_camera_timestamps"](self, track_id, camera)
            outer.append([np.nan, np.nan] if r[0] is None else [float(r[0]), float(r[1])])
            return r

        ActorPose = type("ActorPose", (), dict(methods, find_closest_indices=find_closest_indices,
                                               find_closest_camera_timestamps=find_closest_camera_timestamps))
        ap = ActorPose()
        # what ActorPose.__init__ sets (actor_pose.py:13-30)
        ap.track_ids = torch.from_numpy(c["track_ids"]).to(dt)
        ap.input_trans = torch.from_numpy(c["input_trans"]).to(dt)
        ap.input_rots = torch.from_numpy(c["input_rots"]).to(dt)
        ap.timestamps = c["timestamps"]
        ap.camera_timestamps = {0: {"train_timestamps": list(c["cam_ts"])}}
        ap.opt_track = bool(c["opt_track"])
        if ap.opt_track:
            ap.opt_trans = torch.from_numpy(c["opt_trans"]).to(dt).requires_grad_(True)
            ap.opt_rots = torch.from_numpy(c["opt_rots"]).to(dt).requires_grad_(True)
        ap.obj_info = {int(i): {"start_timestamp": float(s), "end_timestamp": float(e),
                                "track_idx": torch.argwhere(ap.track_ids == int(i))}
                       for i, s, e in zip(c["obj_ids"], c["obj_start"], c["obj_end"])}
        camera = types.SimpleNamespace(meta={"timestamp": float(c["timestamp"]), "cam": 0, "is_val": bool(c["is_val"])},
                                       ego_pose=torch.from_numpy(c["ego"]).to(dt))
        model = types.SimpleNamespace(actor_pose=ap, viewpoint_camera=camera)
        rots, trans, idx, n_samples, outer_ts = [], [], [], [], []
        for tid in c["ids"]:
            del calls[:], outer[:]
            r, t = world_pose(model, int(tid))
            rots.append(r.reshape(4))  # [1, 4] with opt_track: opt_rots[f, c] has shape [1]
            trans.append(t)
            rc = calls[:len(calls) // 2]  # the rotation's calls; the translation repeats them
            assert calls[len(calls) // 2:] == rc and len(rc) in (1, 2)
            idx.append(rc + [[-1] * 4] * (2 - len(rc)))
            n_samples.append(len(rc))
            outer_ts.append(outer[0] if outer else [np.nan, np.nan])
        rots, trans = torch.stack(rots), torch.stack(trans)
        assert rots.dtype == dt and trans.dtype == dt
        out = dict(rot=rots.detach().numpy(), trans=trans.detach().numpy(), idx=np.asarray(idx, np.int32),
                   n_samples=np.asarray(n_samples, np.int32), outer_ts=np.asarray(outer_ts, np.float64))
        if ap.opt_track:
            g = torch.from_numpy(c["g"]).to(dt)
            ((torch.cat([rots, trans], 1) * g).sum()).backward()
            out["dtrans"], out["drots"] = ap.opt_trans.grad.numpy(), ap.opt_rots.grad.numpy()
        return out
    finally:
        torch.set_default_dtype(prev)
        for k, m in held.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m


def scale_of(kind, ref64):
    if kind in ("rot", "trans"):
        return np.abs(ref64).max(axis=-1, keepdims=True)
    return np.abs(ref64).max()


def build():
    cases = make_cases()
    d = {"names": np.asarray(list(cases))}
    e_ref = {k: 0.0 for k in KINDS}
    foreign = empty = False
    for name, c in cases.items():
        o32, o64 = evaluate_case(c, torch.float32), evaluate_case(c, torch.float64)
        for k in ("idx", "n_samples"):
            assert (o32[k] == o64[k]).all(), (name, k)
        for k, v in c.items():
            d[f"{name}/{k}"] = v
        for k in ("idx", "n_samples", "outer_ts"):
            d[f"{name}/{k}"] = o64[k]
        for k in KINDS:
            if k not in o64:
                continue
            assert o32[k].dtype == np.float32 and o64[k].dtype == np.float64
            d[f"{name}/{k}32"], d[f"{name}/{k}64"] = o32[k], o64[k]
            sc = scale_of(k, o64[k])
            assert np.all(sc > 0), (name, k)
            e_ref[k] = max(e_ref[k], float((np.abs(o32[k].astype(np.float64) - o64[k]) / sc).max()))
        if c["opt_track"]:  # whose cell is (frame1, column2)?
            own = dict(zip(c["ids"].tolist(), o64["idx"]))
            for tid, ix in own.items():
                other = int(c["track_ids"][ix[0][0], ix[0][3]])
                foreign |= other >= 0 and other != tid and other in own
                empty |= other < 0
    assert foreign and empty, "the (frame1, column2) cell must hit another actor's cell in one case and an empty one in another"
    for k in KINDS:
        d["e_ref_" + k] = np.float64(e_ref[k])
    return d


def load(path=OUT):
    return dict(np.load(path))


def case(d, name):
    """The entries of one case, without the prefix."""
    p = name + "/"
    return {k[len(p):]: v for k, v in d.items() if k.startswith(p)}


def gate(kind, x, ref64, e_ref, ref32=None):
    """|x - ref_f64| <= FACTOR * e_ref * scale; where the reference's float32 and float64 gradients are both exactly 0, x
    must be exactly 0.  -> (inside, the factor x would need)."""
    x = np.asarray(x, np.float64).reshape(ref64.shape)
    err = np.abs(x - ref64)
    sc = scale_of(kind, ref64)
    ok = bool((err <= FACTOR * e_ref * sc).all())
    if ref32 is not None:
        zero = (ref64 == 0) & (ref32 == 0)
        ok = ok and bool((x[zero] == 0).all())
    return ok, float((err / (e_ref * sc)).max())


if __name__ == "__main__":
    d = build()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: float(d["e_ref_" + k]) for k in KINDS})
