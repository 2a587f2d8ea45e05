"""The reference's libraries/NARF/pose_utils.py with its signatures: the turntable helpers in plain torch (a few tiny ops
each), `interpolate_pose` on the HIP kernel of libenarf_anim.so, and `transform_pose` (:129-148).

`transform_pose` is kept for callers that build part frames themselves; TriPlaneNARF.forward does the same arithmetic
inside enarf_prepare (one launch) instead."""
from copy import deepcopy
from typing import Tuple

import numpy as np
import torch


def rotation_matrix(theta: torch.Tensor) -> torch.Tensor:
    """(B,) angles -> (B, 4, 4) rotations about the y axis, [c 0 -s 0; 0 1 0 0; s 0 c 0; 0 0 0 1] (:10-21)"""
    c, s = torch.cos(theta), torch.sin(theta)
    z, o = torch.zeros_like(c), torch.ones_like(c)
    return torch.stack([c, z, -s, z, z, o, z, z, s, z, c, z, z, z, z, o], dim=-1).reshape(theta.shape[0], 4, 4)


def rotate_pose(pose_3d: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """R (pose - C) + C on the 4 x 4s, C zero but for the mean joint translation in its last column (:39-45);
    pose_3d (B, J, 4, 4), R (B, 4, 4)"""
    center = torch.zeros_like(pose_3d[:, :1])
    center[:, 0, :3, 3] = pose_3d[:, :, :3, 3].mean(dim=1)
    return torch.matmul(R[:, None], pose_3d - center) + center


def rotate_pose_by_angle(pose_3d: torch.Tensor, angle: torch.Tensor) -> torch.Tensor:
    return rotate_pose(pose_3d, rotation_matrix(angle))


def rotate_pose_randomly(pose_3d: torch.Tensor) -> torch.Tensor:
    """every pose turned by its own angle, uniform in [0, 2 pi) (:24-30)"""
    angle = pose_3d.new_empty((pose_3d.shape[0],)).uniform_(0, 2 * np.pi)
    return rotate_pose(pose_3d, rotation_matrix(angle))


def rotate_mesh_by_angle(pose_3d: torch.Tensor, meshes: Tuple[torch.Tensor, ...], angle: torch.Tensor):
    """the vertices (V, 3) of meshes = (vertices, triangles, ...) turned by angle (1,) about the y axis through the
    mean joint translation of pose_3d[0]; the other members are deep copies, as in the reference, so the result may be
    changed without touching the input (:118-126)"""
    vertices = meshes[0]
    center = pose_3d[0, :, :3, 3:].mean(dim=0)                      # (3, 1)
    R = rotation_matrix(angle)
    turned = torch.matmul(R[0, :3, :3], vertices.permute(1, 0) - center) + R[0, :3, 3:] + center
    return (turned.permute(1, 0),) + tuple(deepcopy(m) for m in meshes[1:])


def interpolate_pose(pose_3d, parents, num: int = 100, loop: bool = True, orbit=None):
    """num poses interpolated among the key poses pose_3d (K, J, 4, 4) over the skeleton `parents` (root first), as the
    reference's (:48-115): per joint, the parent-relative rotation is slerped along the short arc and the offset lerped,
    then forward kinematics down the tree. One launch of ops.interpolate_pose, computed in fp64.

    A device tensor gives a device tensor of the same dtype, with no synchronisation. A numpy array is copied to the
    current device and a numpy array of its dtype comes back (the reference's contract). A CPU tensor raises: there is no
    CPU path. `orbit` (not in the reference): num angles, frame i is also turned by orbit[i] as rotate_pose_by_angle does.

    Rotations run on the clock t = i K / num (loop) or i (K - 1) / (num - 1); translations on the reference's
    concatenated linspace blocks of num // K frames (loop, end point left out) or num // (K - 1) frames (end point
    included). Without loop the two clocks therefore differ slightly; this is kept. ValueError where the reference's
    concatenate raises - num not a multiple of K (loop) or K - 1 - and for K < 2 or num < 2 without loop, more than 64
    joints or parents that are not root-first; all checked before any device call."""
    from ... import _anim_lib, ops
    if not isinstance(pose_3d, np.ndarray):
        if orbit is not None and not isinstance(orbit, torch.Tensor):
            _anim_lib.check_pose_args(pose_3d.shape, parents, num, loop)
            if np.shape(orbit) != (int(num),):
                raise ValueError(f"interpolate_pose: orbit takes ({int(num)},) angles, got {np.shape(orbit)}")
            if not (isinstance(pose_3d, torch.Tensor) and pose_3d.is_cuda):
                raise _anim_lib.EnarfHipError("interpolate_pose takes device tensors (there is no CPU fallback); pose_3d is not one")
            orbit = torch.as_tensor(np.asarray(orbit, dtype=np.float64)).to(pose_3d.device)
        return ops.interpolate_pose(pose_3d, parents, num, loop, orbit)
    _anim_lib.check_pose_args(pose_3d.shape, parents, num, loop)
    if pose_3d.dtype not in (np.float32, np.float64):
        raise ValueError(f"interpolate_pose takes float32 or float64 key poses, got {pose_3d.dtype}")
    if orbit is not None and np.shape(orbit) != (int(num),):
        raise ValueError(f"interpolate_pose: orbit takes ({int(num)},) angles, got {np.shape(orbit)}")
    dev = torch.device("cuda", torch.cuda.current_device())
    if orbit is not None:
        orbit = (orbit if isinstance(orbit, torch.Tensor) else torch.as_tensor(np.asarray(orbit, dtype=np.float64))).to(dev)
    out = ops.interpolate_pose(torch.from_numpy(np.ascontiguousarray(pose_3d)).to(dev), parents, num, loop, orbit)
    return out.cpu().numpy()


def transform_pose(pose_to_camera, bone_length, origin_location, parent_id):
    par = torch.as_tensor(list(parent_id)[1:], dtype=torch.long, device=pose_to_camera.device)
    mid = (pose_to_camera[:, 1:, :, 3:] + pose_to_camera[:, par, :, 3:]) / 2
    if origin_location == "center":
        pose_to_camera = torch.cat([pose_to_camera[:, 1:, :, :3], mid], dim=-1)
    elif origin_location == "center_fixed":
        pose_to_camera = torch.cat([pose_to_camera[:, par, :, :3], mid], dim=-1)
    elif origin_location == "center+head":
        bone_length = torch.cat([bone_length, torch.ones(bone_length.shape[0], 1, 1, device=bone_length.device)], dim=1)
        _pose = torch.cat([pose_to_camera[:, par, :, :3], mid], dim=-1)
        pose_to_camera = torch.cat([_pose, pose_to_camera[:, 15][:, None]], dim=1)
    return pose_to_camera, bone_length
