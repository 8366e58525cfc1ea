"""Restatement, in plain torch ops on any device / dtype, of how the reference composes ONE FRAME of its scene graph:
the frame's subset of the models (parse_camera, /root/reference/lib/models/street_gaussian_model.py:230-250) and the
camera pose correction of the background (get_xyz / get_rotation with use_pose_correction, :311-312, 340-341;
PoseCorrection.correct_gaussian_xyz / correct_gaussian_rotation, lib/models/camera_pose.py:89-114) -- test
infrastructure for street_gaussians_amd/scene.py, never imported by the product.  tests/test_scene_frame_cpu.py pins it
against the reference's own methods."""
import torch
import torch.nn.functional as F

import torch_ref_scene as ref


def correction_matrix(c):
    """[7] correction (rotation w, x, y, z not normalised, translation) -> the [4, 4] matrix of camera_pose.py:93-97."""
    rot = F.normalize(c[:4].unsqueeze(0), dim=-1)
    rot = ref.quaternion_to_matrix(rot).squeeze(0)
    m = torch.cat([rot, c[4:7][:, None]], dim=-1)
    padding = torch.tensor([[0, 0, 0, 1]], dtype=c.dtype, device=c.device)
    return torch.cat([m, padding], dim=0)


def correct_xyz(c, xyz):
    """correct_gaussian_xyz (camera_pose.py:89-101): [x, 1] @ M^T."""
    h = torch.cat([xyz, torch.ones_like(xyz[..., :1])], dim=-1)
    return (h @ correction_matrix(c).T)[:, :3]


def correct_rotation(c, rotation):
    """correct_gaussian_rotation (camera_pose.py:103-111): normalize(c_rot) (x) rotation, not renormalised."""
    q = F.normalize(c[:4].unsqueeze(0), dim=-1)
    return ref.quaternion_raw_multiply(q, rotation)


def compose_frame(models, M, S, segments=None, poses=None, correction=None):
    """models: the persistent segment dicts (fields of street_gaussians_amd.scene.Segment); segments: indices of the
    frame's models in rasterization order (None = all, in order); poses: [n_actors_in_frame, 7] replacing the actors'
    `pose` fields in frame order (None = keep them); correction: [7] applied to the static models."""
    idx = list(range(len(models))) if segments is None else list(segments)
    segs, a = [], 0
    for i in idx:
        d = dict(models[i])
        if d.get("pose") is not None and poses is not None:
            d["pose"] = poses[a]
            a += 1
        segs.append(d)
    outs = list(ref.compose(segs, M, S))
    if correction is None:
        return tuple(outs)
    xyzs, rots, row = [], [], 0
    for d in segs:
        n = d["xyz"].shape[0]
        x, r = outs[0][row:row + n], outs[1][row:row + n]
        if d.get("pose") is None:  # the background (get_visibility('background') branch of get_xyz / get_rotation)
            x, r = correct_xyz(correction, x), correct_rotation(correction, r)
        xyzs.append(x)
        rots.append(r)
        row += n
    outs[0], outs[1] = torch.cat(xyzs, 0), torch.cat(rots, 0)
    return tuple(outs)
