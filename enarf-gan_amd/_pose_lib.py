"""ctypes binding of libenarf_pose.so (the C ABI declared in include/enarf_pose.h): the bone masks of the pose prior
(the reference's create_mask / pose_to_image_coord for the SMPL property set) on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable

from ._loader import EnarfHipError, Library, device_of, stream_of

ABI_VERSION = 1

NUM_JOINTS, NUM_BONES, NUM_PARTS, NUM_KEYPOINTS = 24, 27, 19, 24
MAX_SIZE = 4096
OUTPUTS = ("mask", "disparity", "part_disparity", "keypoint_mask", "pose_2d")

_p = C.c_void_p

# every symbol include/enarf_pose.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_pose_abi_version": (C.c_int, []),
    "enarf_pose_last_error": (C.c_char_p, []),
    "enarf_pose_bone_masks": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int, C.c_double, _p, _p, _p, _p, _p, _p]),
}

_library = Library("pose", ABI_VERSION, SIGNATURES, "The bone masks have no CPU fallback.")
load, check = _library.load, _library.check


def bone_masks(pose_to_camera, intrinsics, size: int, thickness: float = 0.5,
               outputs: Iterable[str] = ("mask",)) -> Dict[str, "torch.Tensor"]:
    """{name: device tensor} for each name in `outputs` (a subset of OUTPUTS): mask (B, S, S), disparity (B, S, S),
    part_disparity (B, 19, S, S), keypoint_mask (B, 24, S, S) fp32 and pose_2d (B, 24, 2) fp64, on pose_to_camera's
    device and its current stream. pose_to_camera (B, 24, 4, 4) and intrinsics (B, 3, 3) are device tensors, fp32 or
    fp64 (fp32 is widened to fp64, which is exact); the contract is in include/enarf_pose.h."""
    import torch
    outputs = tuple(outputs)
    bad = [o for o in outputs if o not in OUTPUTS]
    if bad or "mask" not in outputs:
        raise EnarfHipError(f"bone_masks: outputs must include 'mask' and name only {OUTPUTS}, got {outputs}")
    dev = device_of("bone_masks", (torch.float32, torch.float64), pose_to_camera=pose_to_camera, intrinsics=intrinsics)
    if pose_to_camera.dim() != 4 or tuple(pose_to_camera.shape[1:]) != (NUM_JOINTS, 4, 4):
        raise EnarfHipError(f"bone_masks takes (B, 24, 4, 4) pose_to_camera, got {tuple(pose_to_camera.shape)}")
    B = pose_to_camera.shape[0]
    if tuple(intrinsics.shape) != (B, 3, 3):
        raise EnarfHipError(f"bone_masks takes ({B}, 3, 3) intrinsics, got {tuple(intrinsics.shape)}")
    S = int(size)
    if not 1 <= S <= MAX_SIZE:
        raise EnarfHipError(f"bone_masks: size {S} outside [1, {MAX_SIZE}]")
    if not math.isfinite(float(thickness)):
        raise EnarfHipError(f"bone_masks: thickness {thickness} is not finite")
    lib = load()
    shapes = {"mask": (B, S, S), "disparity": (B, S, S), "part_disparity": (B, NUM_PARTS, S, S),
              "keypoint_mask": (B, NUM_KEYPOINTS, S, S), "pose_2d": (B, NUM_JOINTS, 2)}
    with torch.cuda.device(dev):
        pose = pose_to_camera.to(torch.float64).contiguous()
        K = intrinsics.to(torch.float64).contiguous()
        out = {o: torch.empty(shapes[o], dtype=torch.float64 if o == "pose_2d" else torch.float32, device=dev)
               for o in OUTPUTS if o in outputs}
        stream = stream_of(dev)
        ptr = lambda o: out[o].data_ptr() if o in out else None
        check(lib.enarf_pose_bone_masks(pose.data_ptr(), K.data_ptr(), None, B, S, float(thickness),
                                        *(ptr(o) for o in OUTPUTS), stream), "enarf_pose_bone_masks")
    return out
