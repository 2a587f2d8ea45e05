"""dataset/dataset.py of the reference, for the pose prior: SMPLProperty and HumanPoseDataset.

HumanPoseDataset reads a pose-only cache.pickle (formats.read_pose_cache), uploads it to the device once and draws the
bone masks there (libenarf_pose.so). `batches` serves collated batches with one gather and one mask launch each; its
order is the one DataLoader(ds, batch_size, shuffle, drop_last, generator) would take. Item by item, `__getitem__`
returns the reference's keys as device tensors. HumanDataset (images, blosc) is not part of this mirror.
"""
from __future__ import annotations

import os
from typing import Dict, Iterator, List, Optional

import numpy as np
import torch
from torch.utils.data import BatchSampler, Dataset, RandomSampler, SequentialSampler

from .. import _pose_lib, formats
from .._lib import EnarfHipError


class SMPLProperty:
    def __init__(self):
        self.is_blank = np.array([0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1])
        self.num_bone = 19
        self.prev_seq = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 11, 9, 10,
                         11, 12, 13, 16, 17, 18, 20, 21, 22, 23, 24, 25]
        self.num_joint = self.num_bone
        self.num_not_blank_bone = int(np.sum(self.is_blank == 0))
        self.valid_keypoints = [i for i in range(len(self.is_blank)) if i not in self.prev_seq or self.is_blank[i] == 0]
        self.num_valid_keypoints = len(self.valid_keypoints)


# the packed per-frame row of the device table: every field widened to fp64 (exact), one gather per batch
_FIELDS = (("pose_to_camera", (24, 4, 4)), ("intrinsics", (3, 3)), ("pose_to_world", (24, 4, 4)),
           ("bone_length", (23, 1)))


class HumanPoseDataset(Dataset):
    def __init__(self, size=128, data_root="", just_cache=False, num_repeat_in_epoch=100):
        self.size = size
        self.data_root = data_root
        self.just_cache = just_cache
        self.num_repeat_in_epoch = num_repeat_in_epoch
        self.hpp = SMPLProperty()
        self.create_cache()
        self.num_bone = 24
        self.num_bone_param = self.num_bone - 1
        self.num_valid_keypoints = self.hpp.num_valid_keypoints
        self.parents = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9,
                                 12, 13, 14, 16, 17, 18, 19, 20, 21])
        self.deterministic = False
        self._table = None

    def __len__(self):
        return len(self.pose_to_world) * self.num_repeat_in_epoch

    def create_cache(self):
        cache = formats.read_pose_cache(os.path.join(self.data_root, "cache.pickle"))
        self.intrinsics = cache.intrinsics
        self.inv_intrinsics = cache.inv_intrinsics
        self.pose_to_world = cache.pose_to_world
        self.pose_to_camera = cache.pose_to_camera
        if cache.canonical_pose is not None:
            self.canonical_pose = cache.canonical_pose

    def add_blank_part(self, joint_mat_camera, joint_pos_image):
        idx = [0, 0] + list(range(10)) + [9, 9] + list(range(10, 24))
        return joint_mat_camera[:, idx], joint_pos_image[:, :, idx]

    def scale_pose(self, pose, scale):
        pose[:, :3, 3] *= scale
        return pose

    def get_intrinsic(self, i):
        return self.intrinsics[i]

    def get_bone_length(self, pose):
        coordinate = pose[..., :3, 3]
        length = np.linalg.norm(coordinate[..., 1:, :] - coordinate[..., self.parents[1:], :], axis=-1)
        return length[..., None]

    def _device_table(self) -> torch.Tensor:
        """(N, 800) fp64 on the current device: each frame's fields of _FIELDS, uploaded once"""
        if self._table is None:
            if not torch.cuda.is_available():
                raise EnarfHipError("HumanPoseDataset draws its bone masks on the device and there is none")
            n = len(self.pose_to_world)
            cols = {"pose_to_camera": self.pose_to_camera, "intrinsics": self.intrinsics,
                    "pose_to_world": self.pose_to_world, "bone_length": self.get_bone_length(self.pose_to_world)}
            host = np.concatenate([np.asarray(cols[k], np.float64).reshape(n, -1) for k, _ in _FIELDS], axis=1)
            self._table = torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda", torch.cuda.current_device()))
            self._pose_2d_dtype = torch.from_numpy(np.zeros(0, np.result_type(self.pose_to_camera, self.intrinsics))).dtype
        return self._table

    def _draw(self, frames: torch.Tensor) -> Dict[str, torch.Tensor]:
        table = self._device_table()
        rows = table.index_select(0, frames.to(table.device, non_blocking=True))
        out, at = {}, 0
        for name, shape in _FIELDS:
            width = int(np.prod(shape))
            out[name] = rows[:, at:at + width].reshape(-1, *shape)
            at += width
        masks = _pose_lib.bone_masks(out["pose_to_camera"], out["intrinsics"], self.size, 0.5, ("mask", "pose_2d"))
        return {"bone_mask": masks["mask"],
                "pose_to_camera": out["pose_to_camera"].to(torch.float32),
                "bone_length": out["bone_length"].to(torch.float32),
                "pose_to_world": out["pose_to_world"].to(torch.float32),
                "intrinsics": out["intrinsics"].to(torch.float32),
                "pose_2d": masks["pose_2d"].to(self._pose_2d_dtype)}

    def __getitem__(self, i):
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError("HumanPoseDataset draws its masks on the device and cannot serve DataLoader workers: "
                               "iterate HumanPoseDataset.batches(batch_size) instead of a DataLoader")
        i = int(i) % len(self.pose_to_world)
        item = self._draw(torch.tensor([i]))
        return {k: v[0] for k, v in item.items()}

    def batch_order(self, batch_size: int, shuffle: bool = True, drop_last: bool = True,
                    generator: Optional[torch.Generator] = None) -> List[List[int]]:
        """The dataset indices of each batch, in DataLoader(self, batch_size, shuffle=shuffle, drop_last=drop_last,
        generator=generator)'s order: its iterator draws a base seed from the generator before the sampler's permutation."""
        torch.empty((), dtype=torch.int64).random_(generator=generator)
        n = len(self)
        sampler = RandomSampler(range(n), generator=generator) if shuffle else SequentialSampler(range(n))
        return list(BatchSampler(sampler, batch_size, drop_last))

    def batches(self, batch_size: int, shuffle: bool = True, drop_last: bool = True,
                generator: Optional[torch.Generator] = None) -> Iterator[Dict[str, torch.Tensor]]:
        """Collated batches (the keys of __getitem__, a leading batch dimension) on the device and its current stream."""
        n = len(self.pose_to_world)
        for idx in self.batch_order(batch_size, shuffle, drop_last, generator):
            yield self._draw(torch.tensor(idx, dtype=torch.int64) % n)
