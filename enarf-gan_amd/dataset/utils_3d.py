"""dataset/utils_3d.py of the reference: pose_to_image_coord and create_mask, with the masks drawn on the device by
libenarf_pose.so (contract in include/enarf_pose.h), plus a batched `bone_masks` that stays on the device.

create_mask takes the reference's arguments: the outputs of HumanPoseDataset.add_blank_part (28 joints) for the SMPL
property set. Other property sets raise NotImplementedError; there is no CPU path.
"""
from __future__ import annotations

from typing import Iterable

import numpy as np
import torch

from .. import _pose_lib
from .._loader import EnarfHipError, stream_of

# add_blank_part's joint list, and the first position of each of the 24 original joints in it
BLANK_IDX = [0, 0] + list(range(10)) + [9, 9] + list(range(10, 24))
ORIGINAL_POS = [BLANK_IDX.index(j) for j in range(24)]


def pose_to_image_coord(pose_to_camera, intrinsics):
    """(1, 3, num_joints): each joint's translation divided by its own z, then multiplied by the intrinsics (numpy)."""
    image_coord = pose_to_camera[:, :3, 3]
    image_coord = image_coord / image_coord[:, 2:3]
    image_coord = image_coord.transpose()[None]
    return np.matmul(intrinsics, image_coord)


def bone_masks(pose_to_camera: torch.Tensor, intrinsics: torch.Tensor, size: int, thickness: float = 0.5,
               outputs: Iterable[str] = ("mask",)):
    """Masks of a batch of poses on the device: {name: tensor} for `outputs` out of ("mask", "disparity",
    "part_disparity", "keypoint_mask", "pose_2d"). pose_to_camera (B, 24, 4, 4) and intrinsics (B, 3, 3) are device
    tensors (fp32 or fp64). One launch on the current stream."""
    return _pose_lib.bone_masks(pose_to_camera, intrinsics, size, thickness, outputs)


def _is_smpl(hpp) -> bool:
    from .dataset import SMPLProperty
    ref = SMPLProperty()
    try:
        return (list(hpp.prev_seq) == ref.prev_seq and np.array_equal(np.asarray(hpp.is_blank), ref.is_blank)
                and list(hpp.valid_keypoints) == ref.valid_keypoints)
    except (AttributeError, TypeError):
        return False


def create_mask(hpp, joint_mat_camera, joint_pos_image, size, thickness=1.5):
    """(disparity, mask, part_bone_disparity, keypoint_mask) of the first pose of the batch, as the reference returns
    them: float32 (S, S), (S, S), (19, S, S), (24, S, S). joint_mat_camera (1, 28, 4, 4) and joint_pos_image (1, 3, 28)
    are add_blank_part's outputs, numpy arrays (numpy results) or device tensors (device results)."""
    if not _is_smpl(hpp):
        raise NotImplementedError("create_mask draws on the device for the SMPL property set only")
    on_device = isinstance(joint_mat_camera, torch.Tensor)
    if on_device:
        if not isinstance(joint_pos_image, torch.Tensor) or joint_mat_camera.device.type != "cuda" \
                or joint_pos_image.device != joint_mat_camera.device:
            raise EnarfHipError("create_mask takes numpy arrays or device tensors on one device (no CPU fallback)")
        dev = joint_mat_camera.device
        mats = joint_mat_camera[0].to(torch.float64)
        pos = joint_pos_image[0, :2].to(torch.float64)
    else:
        if not torch.cuda.is_available():
            raise EnarfHipError("create_mask draws on the device and there is none (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
        mats = torch.from_numpy(np.asarray(joint_mat_camera[0], np.float64)).to(dev)
        pos = torch.from_numpy(np.asarray(joint_pos_image[0, :2], np.float64)).to(dev)
    if tuple(mats.shape) != (28, 4, 4) or tuple(pos.shape) != (2, 28):
        raise ValueError(f"create_mask takes add_blank_part's (1, 28, 4, 4) and (1, 3, 28), got {tuple(mats.shape)}, "
                         f"{tuple(pos.shape)}")
    pose = mats[ORIGINAL_POS].contiguous()                        # (24, 4, 4)
    jpos = pos.t()[ORIGINAL_POS].contiguous()                     # (24, 2)
    if not (torch.equal(mats[:, :3, 3].nan_to_num(7.0), pose[BLANK_IDX, :3, 3].nan_to_num(7.0))
            and torch.equal(pos.t().nan_to_num(7.0), jpos[BLANK_IDX].nan_to_num(7.0))):
        raise ValueError("create_mask takes add_blank_part's outputs: the blank joints must repeat their originals")
    lib = _pose_lib.load()
    S = int(size)
    with torch.cuda.device(dev):
        out = {"mask": torch.empty(1, S, S, device=dev), "disparity": torch.empty(1, S, S, device=dev),
               "part_disparity": torch.empty(1, _pose_lib.NUM_PARTS, S, S, device=dev),
               "keypoint_mask": torch.empty(1, _pose_lib.NUM_KEYPOINTS, S, S, device=dev)}
        _pose_lib.check(lib.enarf_pose_bone_masks(pose.data_ptr(), None, jpos.data_ptr(), 1, S, float(thickness),
                                                  out["mask"].data_ptr(), out["disparity"].data_ptr(),
                                                  out["part_disparity"].data_ptr(), out["keypoint_mask"].data_ptr(),
                                                  None, stream_of(dev)), "enarf_pose_bone_masks")
    res = (out["disparity"][0], out["mask"][0], out["part_disparity"][0], out["keypoint_mask"][0])
    return res if on_device else tuple(r.cpu().numpy() for r in res)
