"""Torch restatement of Step 2 of the reference's ``StreetGaussianRenderer.render`` (street_gaussian_renderer.py:107-117),
the contract of include/sgr_sky.h: the sky mask of ``SkyCubeMap.forward`` (sky_cubemap.py:77-123), the rays of
``get_rays_torch`` (graphics_utils.py:186-207), the masked cube-map lookup with its fill and clamp, the composite,
``ColorCorrection.forward`` (color_correction.py:129-132) and the eval clamp.  The lookup is ``torch_ref_texture``'s.
Runs in the dtype of its inputs, on any device, with autograd."""
import torch

import torch_ref_texture as tr


def sky_mask_of(acc, sky_mask, train):
    """[H, W] bool: the guidance mask with its top 50 rows set (training), else (1 - acc) > 1e-3 on the detached acc."""
    H, W = acc.shape[-2:]
    if train and sky_mask is not None:
        m = sky_mask.reshape(H, W).clone()  # the reference writes into the caller's mask; this restatement does not
        m[:50, :] = True
        return m
    return (1 - acc.detach().reshape(H, W)) > 1e-3


def rays(H, W, K, R, T, perturb=None):
    """[H, W, 3] unit ray directions through (x + px, y + py), or the pixel centres when perturb is None: xy1 K^-T,
    minus T, times R, minus the origin -R^T T, normalised."""
    dt, dev = K.dtype, K.device
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev), indexing="ij")
    if perturb is None:
        px, py = torch.full_like(xs, 0.5), torch.full_like(ys, 0.5)
    else:
        px, py = perturb[0].to(dt), perturb[1].to(dt)
    pix = torch.stack([xs + px, ys + py, torch.ones_like(xs)], -1)
    cam = pix @ torch.inverse(K).T
    origin = -(R.T @ T)
    d = (cam - T) @ R - origin
    return d / d.norm(dim=-1, keepdim=True)


def sky_color(cube, d, mask, white_background):
    """[3, H, W]: the clamped lookup at the mask pixels, the fill elsewhere (the reference's masked branch)."""
    H, W = mask.shape
    tex = cube.reshape(1, 6, cube.shape[-2], cube.shape[-2], cube.shape[-1])
    fill = 1.0 if white_background else 0.0
    img = torch.full((H, W, tex.shape[-1]), fill, dtype=tex.dtype, device=tex.device)
    if bool(mask.any()):
        sel = d[mask].to(tex.dtype)
        img = img.index_put((mask,), tr.texture_ref(tex, sel[None, None])[0, 0])
    return img.permute(2, 0, 1).clamp(0.0, 1.0)


def color_correct(affine, img):
    return torch.einsum("ij,jhw->ihw", affine[:3, :3], img) + affine[:3, 3].unsqueeze(-1).unsqueeze(-1)


def render_step2(rgb, acc, cube, K, w2c, *, sky_mask=None, train=True, white_background=True, affine=None,
                 clamp_output=False, perturb=None, d=None):
    """The whole of Step 2 in the dtype of ``rgb``; perturb [2, H, W] is required when training (no random draws here).
    ``d`` [H, W, 3]: rays to use instead of the restatement's own."""
    H, W = rgb.shape[-2:]
    dt = rgb.dtype
    Km, Wm = K.to(dt), w2c.to(dt)
    mask = sky_mask_of(acc, sky_mask, train)
    if d is None:
        d = rays(H, W, Km, Wm[:3, :3], Wm[:3, 3], perturb if train else None)
    out = rgb + sky_color(cube.to(dt), d, mask, white_background) * (1 - acc)
    if affine is not None:
        out = color_correct(affine.to(dt), out)
    if clamp_output:
        out = out.clamp(0.0, 1.0)
    return out
