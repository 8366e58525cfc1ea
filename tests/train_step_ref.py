"""The reference leg of one whole training iteration (INTEGRATION.md sections 4, 5, 9, 11), built only from what the suite
already trusts, and the scenario both legs run on -- test infrastructure, CPU only (no GPU tensor is made here).

    torch_ref_actor_pose.poses -> torch_ref_scene_frame.compose_frame -> the C oracle (oracle.forward / oracle.backward;
    the object head is a forward over Gaussians [split, P) alone with the upstream gradient on alpha only)
    -> torch_ref_sky.render_step2 -> torch_ref_frame_loss.frame_loss

Everything before and after the rasterizer runs in float64 with autograd; the oracle is float32 C.  The two stages are
joined by hand, as autograd joins them in the product: the oracle's images enter the float64 head as leaves, the head's
image gradients are the oracle backward's upstream gradients (alpha's is the SUM of its two consumers, the sky composite
and the frame loss), and the oracle's input gradients (the object head's added to the composite's) are the upstream
gradients of the float64 compose.

The scenario: a 96 x 72 image (ragged tile rows and columns, 22 rows below the 50 the training sky-mask rule forces on),
an off-centre K and a yawed, pitched w2c, a background of 600 Gaussians and actors of 257 and 120 (SH degree 3, S = 3,
Fourier dimension 3 with an IDFT row, one flip mask), a cube map with R = 8, an affine colour correction, a camera pose
correction, and an ActorPoses table with optimised tracking whose second actor moves behind the camera.  Three frames:
F0 every model, object term off (the plain rasterizer call); F1 every model, the second actor behind the camera, object
term on; F2 the background only (`poses` is [0, 7], split == P, no object head)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

import torch_ref_actor_pose as rp
import torch_ref_frame_loss as rl
import torch_ref_scene_frame as fref
import torch_ref_sky as rs
from oracle import oracle
from street_gaussians_amd import synthetic as syn
from street_gaussians_amd.actor_pose import ActorPoses

H, W, M, S, R_CUBE = 72, 96, 16, 3, 8
COUNTS = (600, 257, 120)
LAMBDAS = dict(lambda_dssim=0.2, lambda_l1=1.0, lambda_sky=0.01, lambda_reg=0.1, lambda_depth_lidar=0.1)
SKY_SCALE = 1.3
FLIPPED = 1  # the model that carries a flip mask
OUT_NAMES = ("means3D", "rotations", "scales", "opacities", "shs", "semantics")
ORACLE_OF = {"means3D": "means3D", "rotations": "rotations", "scales": "scales", "opacities": "opacity", "shs": "sh",
             "semantics": "semantics"}
RAW = ("xyz", "rotation", "scaling", "opacity", "features_dc", "features_rest", "semantic")
FRAMES = (
    dict(name="F0", segments=[0, 1, 2], ids=[0, 1], timestamp=0.04, obj=False),
    dict(name="F1", segments=[0, 1, 2], ids=[0, 1], timestamp=1.04, obj=True),
    dict(name="F2", segments=[0], ids=[], timestamp=1.04, obj=True),  # obj asked for, but len(in_frame) > 1 is false
)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _tracklets(R_w2c, t_w2c, rng):
    """The tracklet table (the keys of tests/golden/make_actor_pose_fixture.py's cases): two tracks over four frames.
    Around t = 0.04 both actors stand in front of the camera; around t = 1.04 the second one is 7 m BEHIND it."""
    ego = np.eye(4)
    ego[:3, :3], ego[:3, 3] = _rot((0.2, -0.5, 1.0), 0.3), (1.5, -0.5, 0.25)
    in_cam = np.array([[[-0.5, 0.8, 6.0], [0.9, 1.0, 7.0]], [[-0.4, 0.8, 6.1], [0.95, 1.0, 7.1]],
                       [[0.3, 0.9, 5.5], [0.4, 1.0, -7.0]], [[0.35, 0.9, 5.4], [0.4, 1.0, -7.2]]])  # [F, O, 3]
    world = (in_cam - t_w2c) @ R_w2c                    # R^T (x_cam - t), row-vector form
    in_ego = (world - ego[:3, 3]) @ ego[:3, :3]         # E_R^T (x_world - E_t)
    F_, O = 4, 2
    q = rng.standard_normal((F_, O, 4))
    q = q / np.sqrt((q * q).sum(-1, keepdims=True)) * rng.uniform(0.5, 2.0, (F_, O, 1))  # non-unit, as the reference's
    stamps = np.array([0.0, 0.1, 1.0, 1.1])
    return dict(track_ids=np.array([[0, 1]] * F_, np.int32), input_trans=in_ego.astype(np.float32),
                input_rots=q.astype(np.float32), timestamps=stamps, cam_ts=np.zeros(0), obj_ids=np.array([0, 1], np.int32),
                obj_start=np.array([0.0, 0.0]), obj_end=np.array([1.1, 1.1]), opt_track=np.bool_(True),
                opt_trans=rng.uniform(-0.05, 0.05, (F_, O, 3)).astype(np.float32),
                opt_rots=rng.uniform(-0.3, 0.3, (F_, O, 1)).astype(np.float32), ego=ego.astype(np.float32))


def _background(n, K, R_w2c, t_w2c, g):
    """A street-like static model as raw parameters: centres behind the pixels of rows 34 and below (a little past the
    left, right and lower edges), depth uniform in 1/z over 3 .. 20 m, about 3 px wide -- the rows above stay empty sky."""
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    z = 1.0 / (1.0 / 20.0 + u(n) * (1.0 / 3.0 - 1.0 / 20.0))
    px, py = -5.0 + u(n) * (W + 10.0), 34.0 + u(n) * (H + 5.0 - 34.0)
    p_cam = torch.stack([(px - K[0, 2]) / K[0, 0] * z, (py - K[1, 2]) / K[1, 1] * z, z], 1)
    xyz = (p_cam - torch.from_numpy(t_w2c)[None]) @ torch.from_numpy(R_w2c)  # R^T (x_cam - t), row-vector form
    scaling = torch.log(0.03 * z)[:, None] + 0.4 * rn(n, 3)
    dc = 0.3 * rn(n, 1, 3) + 0.5
    f = lambda t: t.float().contiguous()
    return dict(xyz=f(xyz), rotation=f(rn(n, 4)), scaling=f(scaling), opacity=f(3.0 + 1.0 * rn(n, 1)), features_dc=f(dc),
                features_rest=f(0.09 * rn(n, M - 1, 3)), semantic=f(rn(n, S)), semantic_mode="logits")


def actor_poses(c, dev="cpu"):
    """An ActorPoses over the scenario's table, built like `_actor_poses` of tests/test_gpu_actor_pose.py."""
    t = lambda k: torch.from_numpy(c[k].copy()).to(dev)
    info = {int(i): dict(start_timestamp=float(s), end_timestamp=float(e))
            for i, s, e in zip(c["obj_ids"], c["obj_start"], c["obj_end"])}
    return ActorPoses(torch.from_numpy(c["track_ids"]).to(dev), t("input_trans"), t("input_rots"), c["timestamps"],
                      {0: {"train_timestamps": list(c["cam_ts"])}}, info, opt_trans=torch.nn.Parameter(t("opt_trans")),
                      opt_rots=torch.nn.Parameter(t("opt_rots")))


_SCENARIO = None


def scenario():
    """The scenario, made once (CPU float32 tensors; nothing in it is ever written)."""
    global _SCENARIO
    if _SCENARIO is not None:
        return _SCENARIO
    f = 0.95 * W
    K = torch.tensor([[f, 0.0, 0.5 * W + 3.25], [0.0, 1.02 * f, 0.5 * H - 2.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    R = _rot((1, 0, 0), math.radians(4.0)) @ _rot((0, 1, 0), math.radians(12.0))
    t = np.array([0.3, -0.1, 0.5])
    cam = syn.make_camera_general(W, H, K, R, t)
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3], w2c[:3, 3] = torch.from_numpy(R), torch.from_numpy(t)
    g = torch.Generator().manual_seed(8)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    models = [_background(COUNTS[0], K, R, t, g)]
    for k, n in enumerate(COUNTS[1:]):
        models.append(dict(xyz=r(n, 3) * 0.4, rotation=r(n, 4), scaling=-1.5 + 0.3 * torch.randn(n, 3, generator=torch.Generator().manual_seed(100 + k)), opacity=2.0 + r(n, 1),
                           features_dc=r(n, 3, 3) * 0.3, features_rest=r(n, 15, 3) * 0.05, semantic=r(n, 1),
                           pose=torch.zeros(7), idft=torch.tensor([0.7, -0.4, 0.2]), class_label=k % S,
                           semantic_mode="logits",
                           flip_mask=(torch.arange(n) % 3 == 1) if k + 1 == FLIPPED else None))
    sky_mask = torch.zeros(1, H, W, dtype=torch.bool)
    sky_mask[:, :30] = True  # (a pixel outside it that nothing covers sits on the loss's clamp, where it has a jump)
    lidar = torch.where(u(1, H, W) < 0.5, 2.0 + u(1, H, W) * 15.0, torch.zeros(1, H, W))
    lidar[:, :40] = 0.0  # LiDAR returns only where the background stands
    obj_bound = torch.zeros(1, H, W, dtype=torch.bool)
    obj_bound[:, 30:66, 20:80] = True
    sc = SimpleNamespace(
        H=H, W=W, M=M, S=S, cam=cam, K=K.float(), w2c=w2c.float(), models=models,
        tracklets=_tracklets(R, t, np.random.default_rng(20250317)),
        correction=torch.tensor([1.0, 0.01, -0.02, 0.005, 0.03, -0.02, 0.01]),
        cube=u(6, R_CUBE, R_CUBE, 3) * 1.4 - 0.2,
        affine=torch.cat([torch.eye(3) + 0.05 * r(3, 3), 0.02 * r(3, 1)], 1),
        perturb=u(2, H, W), gt=u(3, H, W), mask=u(1, H, W) < 0.8, sky_mask=sky_mask, obj_bound=obj_bound, lidar=lidar,
        bg=torch.zeros(3))
    sc.ap = actor_poses(sc.tracklets)  # the CPU instance: plans only
    _SCENARIO = sc
    return sc


def plan_of(ap, frame):
    return ap.plan(frame["ids"], frame["timestamp"], 0)


def object_head_on(frame):
    """The call-site rule of INTEGRATION.md section 4: the object term is asked for and the frame has an actor."""
    return bool(frame["obj"]) and len(frame["segments"]) > 1


def flip_masks(sc, frame, dev="cpu"):
    return [None if sc.models[i].get("flip_mask") is None else sc.models[i]["flip_mask"].to(dev) for i in frame["segments"]]


# ---- the float64 front: poses and compose ----------------------------------------------------------------------------
def leaves64(sc, override=None):
    """Fresh float64 leaves (requires_grad) of everything the iteration optimises; `override` replaces values by name
    (affine, cube, correction, opt_trans, opt_rots)."""
    o = override or {}
    leaf = lambda t: t.detach().cpu().double().clone().requires_grad_(True)
    L = SimpleNamespace(
        models=[{k: (leaf(v) if k in RAW else v) for k, v in m.items()} for m in sc.models],
        correction=leaf(o.get("correction", sc.correction)), cube=leaf(o.get("cube", sc.cube)),
        affine=leaf(o.get("affine", sc.affine)),
        opt_trans=leaf(o.get("opt_trans", torch.from_numpy(sc.tracklets["opt_trans"]))),
        opt_rots=leaf(o.get("opt_rots", torch.from_numpy(sc.tracklets["opt_rots"]))))
    for m in L.models:
        if m.get("idft") is not None:
            m["idft"] = m["idft"].double()
    return L


def ref_poses(sc, frame, opt_trans, opt_rots, dtype=torch.float64):
    plan = plan_of(sc.ap, frame)
    if len(plan) == 0:
        return torch.zeros(0, 7, dtype=dtype)
    t = lambda k: torch.from_numpy(sc.tracklets[k].copy())
    return rp.poses(plan.records, t("input_trans"), t("input_rots"), opt_trans, opt_rots, t("ego"), dtype)


def ref_compose(sc, frame, models, poses, correction):
    """compose_frame with the frame's flip masks (the persistent dicts carry them) -> the six outputs."""
    return fref.compose_frame(models, sc.M, sc.S, segments=frame["segments"], poses=poses if len(frame["ids"]) else None,
                              correction=correction)


# ---- the rasterizer stage: the C oracle ---------------------------------------------------------------------------------
def oracle_kwargs(sc, outs, lo=0):
    """The oracle's keyword arguments for rows [lo, P) of the six compose outputs (float32)."""
    f = lambda t: np.ascontiguousarray(np.asarray(t.detach().cpu() if hasattr(t, "detach") else t, np.float32)[lo:])
    means3D, rot, scales, opac, shs, sem = outs
    cam = sc.cam
    return dict(means3D=f(means3D), opacities=f(opac), viewmatrix=cam.viewmatrix, projmatrix=cam.projmatrix,
                campos=cam.campos, bg=sc.bg, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, image_height=sc.H,
                image_width=sc.W, sh_degree=3, shs=f(shs), scales=f(scales), rotations=f(rot), semantics=f(sem))


def split_of(sc, frame):
    return sc.models[frame["segments"][0]]["xyz"].shape[0]


def raster_forward(sc, frame, outs):
    """-> (fw, fw_obj): the oracle's forward over the frame, and over Gaussians [split, P) alone when the object head
    is on (else None)."""
    fw = oracle.forward(**oracle_kwargs(sc, outs))
    fw_obj = oracle.forward(**oracle_kwargs(sc, outs, lo=split_of(sc, frame))) if object_head_on(frame) else None
    return fw, fw_obj


def raster_backward(sc, frame, fw, fw_obj, d_color, d_depth, d_alpha, d_semantic=None, d_acc_obj=None):
    """-> (composite head's gradients, object head's gradients padded to P rows or None), by OUT_NAMES, plus
    "means2D" in the first.  A None upstream gradient is the zeros the product fills in."""
    z = lambda t, c: np.zeros((c, sc.H, sc.W), np.float32) if t is None else np.asarray(t, np.float32).reshape(c, sc.H, sc.W)
    g = oracle.backward(fw, z(d_color, 3), z(d_depth, 1), z(d_alpha, 1), z(d_semantic, sc.S))
    comp = {k: np.asarray(g[ORACLE_OF[k]], np.float64) for k in OUT_NAMES}
    comp["means2D"] = np.asarray(g["means2D"], np.float64)
    obj = None
    if fw_obj is not None and d_acc_obj is not None:
        go = oracle.backward(fw_obj, z(None, 3), z(None, 1), z(d_acc_obj, 1), None)
        split = split_of(sc, frame)
        obj = {}
        for k in ("means3D", "rotations", "scales", "opacities"):
            full = np.zeros_like(comp[k])
            full[split:] = np.asarray(go[ORACLE_OF[k]], np.float64).reshape(full[split:].shape)
            obj[k] = full
    return comp, obj


# ---- the float64 head: sky composite and frame loss ---------------------------------------------------------------------
def head(sc, frame, color, depth, a_sky, a_loss, acc_obj, cube, affine, rays=None):
    """render_step2 then frame_loss on float64 tensors.  `a_sky` / `a_loss`: the alpha image as its two consumers see it
    (the same values; two tensors so that each consumer's gradient can be read alone).  -> (image, terms dict)."""
    image = rs.render_step2(color, a_sky, cube, sc.K, sc.w2c, sky_mask=sc.sky_mask, train=True, white_background=True,
                            affine=affine, perturb=sc.perturb, d=rays)
    kw = dict(LAMBDAS, acc=a_loss, sky_mask=sc.sky_mask, sky_scale=SKY_SCALE, depth=depth, lidar_depth=sc.lidar.double())
    if acc_obj is not None:
        kw.update(acc_obj=acc_obj, obj_bound=sc.obj_bound)
    return image, rl.frame_loss(image, sc.gt.double(), sc.mask, **kw)


# ---- one iteration ------------------------------------------------------------------------------------------------------
def reference_step(sc, frame, override=None, backward=True):
    """One iteration of the reference leg.  -> a namespace: the leaves (with .grad after the backward), poses, the six
    compose outputs, the oracle's forwards (`fw`, `fw_obj`), the image, the terms, and -- with `backward` -- the image
    gradients (`d_color`, `d_depth`, `d_alpha_sky`, `d_alpha_loss`, `d_acc_obj`), the rasterizer's input gradients of
    both heads (`g_comp`, `g_obj`) and `means2D_grad`."""
    L = leaves64(sc, override)
    poses = ref_poses(sc, frame, L.opt_trans, L.opt_rots)
    outs = ref_compose(sc, frame, L.models, poses, L.correction)
    fw, fw_obj = raster_forward(sc, frame, outs)
    img_leaf = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy()).requires_grad_(True)
    color, depth, a_sky, a_loss = img_leaf(fw.color), img_leaf(fw.depth), img_leaf(fw.alpha), img_leaf(fw.alpha)
    acc_obj = img_leaf(fw_obj.alpha) if fw_obj is not None else None
    image, terms = head(sc, frame, color, depth, a_sky, a_loss, acc_obj, L.cube, L.affine)
    out = SimpleNamespace(leaves=L, poses=poses, outs=outs, fw=fw, fw_obj=fw_obj, image=image, terms=terms,
                          color=color, depth=depth, alpha=a_loss, acc_obj=acc_obj, loss=float(terms["loss"].detach()))
    if not backward:
        return out
    terms["loss"].backward()
    n = lambda t: None if t is None or t.grad is None else t.grad.numpy()
    out.d_color, out.d_depth, out.d_alpha_sky, out.d_alpha_loss, out.d_acc_obj = n(color), n(depth), n(a_sky), n(a_loss), n(acc_obj)
    out.g_comp, out.g_obj = raster_backward(sc, frame, fw, fw_obj, out.d_color, out.d_depth, out.d_alpha_sky + out.d_alpha_loss,
                                            None, out.d_acc_obj)
    out.means2D_grad = out.g_comp["means2D"]
    ups = []
    for k, o in zip(OUT_NAMES, outs):
        u = out.g_comp[k] + (out.g_obj[k] if out.g_obj is not None and k in out.g_obj else 0.0)
        ups.append(torch.from_numpy(np.asarray(u, np.float64).reshape(tuple(o.shape))))
    pairs = [(o, u) for o, u in zip(outs, ups) if o.requires_grad]
    torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
    return out


def model_rows(sc, frame):
    """{persistent model index: (first row, end row)} inside the frame's composed tensors."""
    rows, at = {}, 0
    for i in frame["segments"]:
        n = sc.models[i]["xyz"].shape[0]
        rows[i] = (at, at + n)
        at += n
    return rows
