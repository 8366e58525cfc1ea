"""`-m gpu` tests of HOW upstream gradients arrive at the library's autograd functions in a real graph, on the 96 x 72
scene of tests/train_step_ref.py (S = 3), in the default switch mask and in strict mode.

Subsets: _RasterizeGaussians and _ObjectAlpha call ctx.set_materialize_grads(False) and fill in the missing image gradients
by hand; every nonempty subset of {color, depth, alpha, semantic} as the outputs a loss uses must give, byte for byte, the
gradients of a backward that was handed explicit zero tensors for the others.  Heads: the same for the object head alone,
the composite alone (with an _ObjectAlpha that is handed None) and both.  Forms: every autograd function -- the
rasterizer, the object head, the sky composite, the frame loss, the actor poses, the compose backward and texture() -- fed
a stride-0 expand (what .sum().backward() makes), a permuted channel-last view and the gradient a larger graph computes,
against the same backward fed the .contiguous() copy, byte for byte.

Every tensor handed in starts at a storage offset that is a multiple of 4 elements."""
import itertools

import pytest
import torch

import train_step_ref as tsr
from gpu_utils import switches
from train_step_gpu import DEV, MODES, Chain, mode_mask

pytestmark = pytest.mark.gpu
SC = tsr.scenario()
IMAGES = ("color", "depth", "alpha", "semantic")
INPUTS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations", "semantics")
GEOM = ("means3D", "opacities", "scales", "rotations")


def _same_bytes(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


def _weights(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(tuple(shape), generator=g) - 0.5).to(DEV)


def _render(frame, object_head):
    """The frame's composed Gaussians as leaves, rendered -> (inputs by name, outputs by name)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    ch = Chain()
    with torch.no_grad():
        t = ch.forward(frame, sinks=False)
    ins = {k: t[k].detach().clone().requires_grad_(True) for k in tsr.OUT_NAMES}
    ins["means2D"] = torch.zeros(ins["means3D"].shape[0], 3, device=DEV, requires_grad=True)
    rast = GaussianRasterizer(ch.settings)
    args = dict(shs=ins["shs"], scales=ins["scales"], rotations=ins["rotations"], semantics=ins["semantics"])
    if object_head:
        out = rast.forward_with_object_alpha(ins["means3D"], ins["means2D"], ins["opacities"], **args, split=tsr.COUNTS[0])
        names = ("color", "radii", "depth", "alpha", "semantic", "acc_obj")
    else:
        out = rast(ins["means3D"], ins["means2D"], ins["opacities"], **args)
        names = ("color", "radii", "depth", "alpha", "semantic")
    return ch, ins, dict(zip(names, out))


def _grads(outs, ups, ins, names=INPUTS):
    g = torch.autograd.grad(outs, [ins[k] for k in names], grad_outputs=ups, retain_graph=True, allow_unused=True)
    torch.cuda.synchronize()
    return dict(zip(names, g))


# ---- subsets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_every_subset_of_the_rasterizers_images(mode):
    """15 nonempty subsets: the gradients of every input, means2D included, equal byte for byte those of a backward given
    explicit zeros for the images the loss does not use."""
    with switches(mode_mask(mode)):
        _, ins, out = _render(tsr.FRAMES[0], object_head=False)
        w = {k: _weights(out[k].shape, 11 + i) for i, k in enumerate(IMAGES)}
        every = _grads([out[k] for k in IMAGES], [w[k] for k in IMAGES], ins)
        for n in range(1, 5):
            for subset in itertools.combinations(IMAGES, n):
                got = _grads([out[k] for k in subset], [w[k] for k in subset], ins)
                want = _grads([out[k] for k in IMAGES], [w[k] if k in subset else torch.zeros_like(out[k]) for k in IMAGES], ins)
                for k in INPUTS:
                    assert got[k] is not None and torch.isfinite(got[k]).all(), (subset, k)
                    assert _same_bytes(got[k], want[k]), f"{subset}: d_{k} differs from the backward given explicit zeros"
                if n == 4:
                    assert all(_same_bytes(got[k], every[k]) for k in INPUTS)
        # each image moves something, and an unused one moves nothing that only it reaches
        only_sem = _grads([out["semantic"]], [w["semantic"]], ins)
        assert only_sem["semantics"].abs().max() > 0 and not only_sem["shs"].any()
        only_color = _grads([out["color"]], [w["color"]], ins)
        assert only_color["shs"].abs().max() > 0 and not only_color["semantics"].any()
        assert not _same_bytes(_grads([out["alpha"]], [w["alpha"]], ins)["opacities"], only_color["opacities"])


@pytest.mark.parametrize("mode", list(MODES))
def test_radii_alone_differentiate_nothing(mode):
    """The empty subset: a loss that reads radii only has no graph, so nothing is launched and nothing gets a gradient."""
    with switches(mode_mask(mode)):
        _, ins, out = _render(tsr.FRAMES[0], object_head=False)
        radii = out["radii"]
        assert not radii.requires_grad and radii.grad_fn is None and radii.dtype == torch.int32
        loss = radii.float().sum()
        assert not loss.requires_grad
        with pytest.raises(RuntimeError, match="does not require grad"):
            loss.backward()
        torch.cuda.synchronize()
        assert all(v.grad is None for v in ins.values())


# ---- heads -----------------------------------------------------------------------------------------------------------
class _NoGradient(torch.autograd.Function):
    """A consumer that reads its input and returns no gradient for it (what a loss does for an input it does not
    differentiate): the producer's backward is then handed None."""

    @staticmethod
    def forward(ctx, x):
        return x.sum()

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("mode", list(MODES))
def test_object_head_alone_composite_alone_and_both(mode):
    with switches(mode_mask(mode)):
        _, ins, out = _render(tsr.FRAMES[1], object_head=True)
        w = {k: _weights(out[k].shape, 21 + i) for i, k in enumerate(IMAGES + ("acc_obj",))}
        zeros = {k: torch.zeros_like(out[k]) for k in w}
        comp = [out[k] for k in IMAGES]
        # the object head alone
        obj = _grads([out["acc_obj"]], [w["acc_obj"]], ins)
        assert all(obj[k] is None for k in ("means2D", "shs", "semantics"))
        assert all(obj[k].abs().max() > 0 and not obj[k][:tsr.COUNTS[0]].any() for k in GEOM)
        # ... equals the backward of all five outputs with explicit zeros for the composite's four
        with_zeros = _grads(comp + [out["acc_obj"]], [zeros[k] for k in IMAGES] + [w["acc_obj"]], ins)
        for k in GEOM:
            assert torch.equal(with_zeros[k], obj[k]), f"object head alone: d_{k}"
        assert all(not with_zeros[k].any() for k in ("means2D", "shs", "semantics"))
        # the composite alone; and with an object head that takes part in the graph but is handed None
        alone = _grads(comp, [w[k] for k in IMAGES], ins)
        loss = sum((out[k] * w[k]).sum() for k in IMAGES) + _NoGradient.apply(out["acc_obj"])
        handed_none = _grads([loss], None, ins)
        for k in INPUTS:
            assert _same_bytes(handed_none[k], alone[k]), f"composite alone: d_{k} changes when _ObjectAlpha is handed None"
        # both: autograd's sum of the two
        both = _grads(comp + [out["acc_obj"]], [w[k] for k in IMAGES] + [w["acc_obj"]], ins)
        for k in INPUTS:
            want = alone[k] + obj[k] if k in GEOM else alone[k]
            assert torch.equal(both[k], want), f"both heads: d_{k}"
        # a subset of the composite's images next to the object head: None for color and semantic
        part = _grads([out["depth"], out["alpha"], out["acc_obj"]], [w["depth"], w["alpha"], w["acc_obj"]], ins)
        part_zeros = _grads(comp + [out["acc_obj"]], [zeros["color"], w["depth"], w["alpha"], zeros["semantic"], w["acc_obj"]], ins)
        for k in INPUTS:
            assert _same_bytes(part[k], part_zeros[k]), f"depth + alpha + object head: d_{k}"


# ---- forms -----------------------------------------------------------------------------------------------------------
def _expanded(shape, value):
    return torch.tensor(value, device=DEV).expand(tuple(shape))


def _permuted(shape, seed):
    """Random values in a permuted layout: an image's channel-last view (the first dimension is the fastest in memory);
    where that is no permutation (a leading dimension of 1), the last dimension is the slowest instead."""
    shape = tuple(shape)
    n = len(shape)
    view = _weights(shape[1:] + shape[:1], seed).permute(n - 1, *range(n - 1))
    if view.is_contiguous():
        view = _weights(shape[-1:] + shape[:-1], seed).permute(*range(1, n), 0)
    assert tuple(view.shape) == shape
    return view


def _check_forms(outs, ins, names, label, seed=31):
    """`outs`: the op's differentiable outputs.  Each form of upstream gradient against its .contiguous() copy."""
    forms = {"expand": [_expanded(o.shape, 0.37 + 0.1 * i) for i, o in enumerate(outs)]}
    if all(o.dim() >= 2 for o in outs):
        forms["permuted"] = [_permuted(o.shape, seed + i) for i, o in enumerate(outs)]
    for form, ups in forms.items():
        if form == "permuted":
            assert any(not u.is_contiguous() for u in ups if u.numel() > 1), label
        assert all(u.storage_offset() % 4 == 0 for u in ups)
        got = _grads(outs, ups, ins, names)
        want = _grads(outs, [u.contiguous() for u in ups], ins, names)
        for k in names:
            assert _same_bytes(got[k], want[k]), f"{label}: d_{k} differs for the {form} form"
            assert want[k] is None or torch.isfinite(want[k]).all(), (label, k)
    # the gradient a larger graph computes: non-leaf float32 results of other backward nodes
    w = [_weights(o.shape, seed + 10 + i) for i, o in enumerate(outs)]
    loss = sum((torch.tanh(o) * x).sum() for o, x in zip(outs, w)) * 1.5
    through = _grads([loss], None, ins, names)
    ups = torch.autograd.grad(loss, outs, retain_graph=True)
    want = _grads(outs, [u.contiguous().clone() for u in ups], ins, names)
    for k in names:
        assert _same_bytes(through[k], want[k]), f"{label}: d_{k} differs when the gradient comes out of a larger graph"


@pytest.mark.parametrize("mode", list(MODES))
def test_forms_rasterizer_and_object_head(mode):
    with switches(mode_mask(mode)):
        _, ins, out = _render(tsr.FRAMES[1], object_head=True)
        _check_forms([out[k] for k in IMAGES], ins, INPUTS, "_RasterizeGaussians")
        _check_forms([out["acc_obj"]], ins, GEOM, "_ObjectAlpha")


def test_forms_sky_composite_and_frame_loss():
    from street_gaussians_amd.losses import frame_loss
    from street_gaussians_amd.sky import composite_sky
    ch = Chain()
    with torch.no_grad():
        t = ch.forward(tsr.FRAMES[1], sinks=False)
    leaf = lambda x: x.detach().clone().requires_grad_(True)
    ins = dict(rgb=leaf(t["color"]), acc=leaf(t["alpha"]), cube=leaf(ch.cube), affine=leaf(ch.affine))
    image = composite_sky(ins["rgb"], ins["acc"], ins["cube"], ch.K, ch.w2c, sky_mask=ch.sky_mask, affine=ins["affine"], perturb=ch.perturb)
    _check_forms([image], ins, tuple(ins), "_SkyComposite")
    lin = dict(image=leaf(t["image"]), acc=leaf(t["alpha"]), depth=leaf(t["depth"]), acc_obj=leaf(t["acc_obj"]))
    loss, _ = frame_loss(lin["image"], ch.gt, ch.mask, **tsr.LAMBDAS, acc=lin["acc"], sky_mask=ch.sky_mask, sky_scale=tsr.SKY_SCALE,
                         acc_obj=lin["acc_obj"], obj_bound=ch.obj_bound, depth=lin["depth"], lidar_depth=ch.lidar)
    # a 0-dim upstream gradient: a stride-0 expand is itself; a view into a larger buffer (offset 4) and a larger graph
    names = tuple(lin)
    up = torch.tensor([9.0, 9.0, 9.0, 9.0, 0.7], device=DEV)[4]
    assert up.storage_offset() == 4 and up.dim() == 0
    got, want = _grads([loss], [up], lin, names), _grads([loss], [up.clone()], lin, names)
    through = _grads([(loss * 0.7)], None, lin, names)
    for k in names:
        assert _same_bytes(got[k], want[k]) and _same_bytes(through[k], want[k]), f"_FrameLoss: d_{k}"
        assert want[k].abs().max() > 0


def test_forms_poses_and_compose():
    ch = Chain()
    frame = tsr.FRAMES[1]
    poses = ch.ap.poses(ch.ap.plan(frame["ids"], frame["timestamp"], 0), ch.ego)
    _check_forms([poses], dict(opt_trans=ch.ap.opt_trans, opt_rots=ch.ap.opt_rots), ("opt_trans", "opt_rots"), "_Poses")
    leaf_poses = poses.detach().clone().requires_grad_(True)
    outs = ch.flat.compose(SC.M, SC.S, flip_masks=[ch.masks[i] for i in frame["segments"]], segments=frame["segments"], poses=leaf_poses,
                           correction=ch.correction)
    ins = dict(ch.flat.tensors, poses=leaf_poses, correction=ch.correction)
    _check_forms(list(outs), ins, tuple(ins), "compose")


def test_forms_texture():
    import nvdiffrast.torch as dr
    g = torch.Generator().manual_seed(5)
    tex = (torch.rand(1, 6, tsr.R_CUBE, tsr.R_CUBE, 3, generator=g)).to(DEV).requires_grad_(True)
    uv = torch.nn.functional.normalize(torch.randn(1, SC.H, SC.W, 3, generator=g), dim=-1).to(DEV)
    out = dr.texture(tex, uv, filter_mode="linear", boundary_mode="cube")
    _check_forms([out], dict(tex=tex), ("tex",), "texture")
