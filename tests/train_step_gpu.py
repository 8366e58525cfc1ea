"""The product leg of one whole training iteration on the scenario of tests/train_step_ref.py, as INTEGRATION.md sections
4, 5, 9 and 11 write the call site:

    ActorPoses.poses -> FlatScene.compose(poses=, correction=, grad_sink=) -> GaussianRasterizer (forward_with_object_alpha
    when the object term is on and the frame has an actor) with a stats_sink -> composite_sky(cube_sink=) -> frame_loss
    -> loss.backward() -> SegmentedAdam.step / SkyAdam.step, torch.optim.Adam on the small leaves

-- shared by tests/test_gpu_train_step.py and tests/test_gpu_upstream_grads.py; imported only by `-m gpu` tests."""
import contextlib

import numpy as np
import torch

import train_step_ref as tsr
from gpu_utils import settings
from street_gaussians_amd import _C, scene
from street_gaussians_amd.losses import frame_loss
from street_gaussians_amd.optim import GROUPS, SegmentedAdam
from street_gaussians_amd.sky import SkyAdam, composite_sky

DEV = "cuda"
MODES = {"default": 0, "strict": _C.EXACT | _C.REF_RECT}


def mode_mask(mode):
    return _C.test_switches(-1) | MODES[mode]


def gpu_segments(sc):
    segs = []
    for m in sc.models:
        t = {k: m[k].to(DEV) for k in tsr.RAW}
        actor = m.get("pose") is not None
        segs.append(scene.Segment(pose=m["pose"].to(DEV) if actor else None, idft=m["idft"].to(DEV) if actor else None,
                                  class_label=m.get("class_label", 0), semantic_mode=m["semantic_mode"], **t))
    return segs


class Chain:
    """Everything one trainer holds: the flat scene and its SegmentedAdam (random moments, uneven step counts), the cube
    map and its SkyAdam, the statistics, the ActorPoses table, the correction and affine leaves, and one
    torch.optim.Adam(eps=1e-15) over the four small leaves."""

    def __init__(self, sc=None, seed=3):
        self.sc = sc = sc or tsr.scenario()
        self.flat = scene.FlatScene.from_segments(gpu_segments(sc))
        K = len(sc.models)
        rng = np.random.default_rng(seed)
        self.opt = SegmentedAdam(self.flat, [{g: float(10 ** rng.uniform(-4, -2)) for g in GROUPS} for _ in range(K)])
        for a in self.opt.exp_avg:
            gen = torch.Generator().manual_seed(seed + len(a))
            self.opt.exp_avg[a].copy_(torch.randn(self.opt.exp_avg[a].shape, generator=gen).to(DEV) * 1e-2)
            self.opt.exp_avg_sq[a].copy_(torch.rand(self.opt.exp_avg_sq[a].shape, generator=gen).to(DEV) * 1e-4)
        for st in self.opt.steps:
            for g in GROUPS:
                st[g] = int(rng.integers(0, 50))
        self.cube = sc.cube.to(DEV).clone().requires_grad_(True)
        self.sky_opt = SkyAdam(self.cube, 1e-3, eps=1e-15)
        self.stats = scene.FlatStats([m["count"] for m in self.flat.meta], DEV)
        self.ap = tsr.actor_poses(sc.tracklets, DEV)
        self.correction = sc.correction.to(DEV).clone().requires_grad_(True)
        self.affine = sc.affine.to(DEV).clone().requires_grad_(True)
        self.small = dict(opt_trans=self.ap.opt_trans, opt_rots=self.ap.opt_rots, correction=self.correction, affine=self.affine)
        self.adam = torch.optim.Adam([dict(params=[self.ap.opt_trans, self.ap.opt_rots], lr=1e-3),
                                      dict(params=[self.correction], lr=1e-4), dict(params=[self.affine], lr=1e-3)], eps=1e-15)
        d = lambda t: t.to(DEV).contiguous()
        self.K, self.w2c, self.perturb, self.gt, self.mask = d(sc.K), d(sc.w2c), d(sc.perturb), d(sc.gt), d(sc.mask)
        self.sky_mask, self.obj_bound, self.lidar = d(sc.sky_mask), d(sc.obj_bound), d(sc.lidar)
        self.ego = torch.from_numpy(sc.tracklets["ego"]).to(DEV)
        self.settings = settings(sc.cam, bg=sc.bg)
        self.masks = [None if m.get("flip_mask") is None else m["flip_mask"].to(DEV) for m in sc.models]

    # ---- the call site ---------------------------------------------------------------------------------------------
    def forward(self, frame, sinks, around_raster=contextlib.nullcontext, capture=False):
        """One forward as the call site writes it -> a dict of every tensor that crosses an op boundary.  `capture`:
        retain_grad() on all of them, and each consumer of alpha reads it through a view of its own (`alpha_sky`,
        `alpha_loss`), so that each consumer's gradient can be read next to their sum."""
        from diff_gaussian_rasterization import GaussianRasterizer
        sc, segs = self.sc, frame["segments"]
        plan = self.ap.plan(frame["ids"], frame["timestamp"], 0)
        poses = self.ap.poses(plan, self.ego)
        sink = self.opt.sink(segs) if sinks else None
        outs = self.flat.compose(sc.M, sc.S, flip_masks=[self.masks[i] for i in segs], segments=segs, poses=poses,
                                 correction=self.correction, grad_sink=sink)
        means3D, rot, scales, opac, shs, sem = outs
        rast = GaussianRasterizer(self.settings)
        rast.stats_sink = self.stats.sink(models=segs) if sinks else None
        m2d = torch.zeros(means3D.shape[0], 3, device=DEV, requires_grad=True)
        args = dict(shs=shs, scales=scales, rotations=rot, semantics=sem)
        with around_raster():
            if tsr.object_head_on(frame):
                color, radii, depth, alpha, semantic, acc_obj = rast.forward_with_object_alpha(
                    means3D, m2d, opac, **args, split=self.flat.meta[segs[0]]["count"])
            else:
                color, radii, depth, alpha, semantic = rast(means3D, m2d, opac, **args)
                acc_obj = None
            from street_gaussians_amd import rasterizer
            num_rendered = rasterizer.last_num_rendered()
        alpha_sky = alpha.view_as(alpha) if capture else alpha
        alpha_loss = alpha.view_as(alpha) if capture else alpha
        image = composite_sky(color, alpha_sky, self.cube, self.K, self.w2c, sky_mask=self.sky_mask, train=True,
                              white_background=True, affine=self.affine, perturb=self.perturb,
                              cube_sink=self.sky_opt.sink() if sinks else None)
        kw = dict(tsr.LAMBDAS, acc=alpha_loss, sky_mask=self.sky_mask, sky_scale=tsr.SKY_SCALE, depth=depth, lidar_depth=self.lidar)
        if acc_obj is not None:
            kw.update(acc_obj=acc_obj, obj_bound=self.obj_bound)
        loss, terms = frame_loss(image, self.gt, self.mask, **kw)
        t = dict(poses=poses, means3D=means3D, rotations=rot, scales=scales, opacities=opac, shs=shs, semantics=sem,
                 means2D=m2d, color=color, depth=depth, alpha=alpha, semantic=semantic, acc_obj=acc_obj, image=image,
                 alpha_sky=alpha_sky, alpha_loss=alpha_loss, radii=radii, loss=loss, terms=terms, num_rendered=num_rendered)
        if capture:
            for k, v in t.items():
                if isinstance(v, torch.Tensor) and v.requires_grad and not v.is_leaf:
                    v.retain_grad()
        return t

    def schedule(self, it):
        """The learning rates of iteration `it` (they change between iterations)."""
        for s in range(len(self.opt.lrs)):
            self.opt.lrs[s]["xyz"] *= 0.7
        self.opt.lrs[it % len(self.opt.lrs)]["opacity"] *= 3.0
        self.sky_opt.lr = 1e-3 * (0.8 ** it)
        for gi, group in enumerate(self.adam.param_groups):
            group["lr"] = (1e-3, 1e-4, 1e-3)[gi] * (0.9 ** it)

    def iterate(self, it, frame, sinks, around_raster=contextlib.nullcontext, torch_adam=True):
        """Path A (`sinks`): the three sinks armed.  Path B: no parameter sink, then opt.step, sky_opt.step() and
        scene.densification_stats.  -> the iteration's record (numpy copies; the small leaves' gradients before they are
        reset)."""
        self.schedule(it)
        segs = frame["segments"]
        t = self.forward(frame, sinks, around_raster)
        t["loss"].backward()
        rec = {"flat_grads": None}
        if not sinks:
            rec["flat_grads"] = {a: x.grad for a, x in self.flat.tensors.items()}
            scene.densification_stats([self.stats.views()[i] for i in segs], t["means2D"].grad, t["radii"])
        self.opt.step(segs)
        self.sky_opt.step()
        for x in self.flat.tensors.values():
            if sinks:
                assert x.grad is None
            x.grad = None
        self.cube.grad = None
        rec["small_grads"] = {k: (None if v.grad is None else v.grad.clone()) for k, v in self.small.items()}
        if torch_adam:
            self.adam.step()
        self.adam.zero_grad(set_to_none=True)
        rec["images"] = {k: t[k].detach() for k in ("color", "depth", "alpha", "semantic", "image", "radii")}
        rec["images"]["acc_obj"] = torch.zeros_like(t["alpha"]).detach() if t["acc_obj"] is None else t["acc_obj"].detach()
        rec["values"] = t["terms"].values
        rec["means2D_grad"] = t["means2D"].grad
        return rec

    # ---- state -------------------------------------------------------------------------------------------------------
    def state(self):
        """Everything an iteration may change, as numpy copies."""
        torch.cuda.synchronize()
        n = lambda x: x.detach().cpu().numpy().copy()
        out = {f"p.{a}": n(x) for a, x in self.flat.tensors.items()}
        out.update({f"m.{a}": n(x) for a, x in self.opt.exp_avg.items()})
        out.update({f"v.{a}": n(x) for a, x in self.opt.exp_avg_sq.items()})
        out.update(cube=n(self.cube), sky_m=n(self.sky_opt.exp_avg), sky_v=n(self.sky_opt.exp_avg_sq),
                   acc_stat=n(self.stats.xyz_gradient_accum), denom=n(self.stats.denom), max_radii=n(self.stats.max_radii2D))
        out.update({k: n(v) for k, v in self.small.items()})
        return out

    def counts(self):
        import copy
        return copy.deepcopy(self.opt.steps), self.sky_opt.step_count


def numpy_record(rec):
    """An iteration's record as numpy arrays (after a synchronisation)."""
    torch.cuda.synchronize()
    n = lambda x: None if x is None else x.detach().cpu().numpy().copy()
    out = {f"img.{k}": n(v) for k, v in rec["images"].items()}
    out.update({f"grad.{k}": n(v) for k, v in rec["small_grads"].items()})
    out.update(values=n(rec["values"]), means2D_grad=n(rec["means2D_grad"]))
    return out


def bytes_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
