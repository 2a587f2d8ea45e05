"""ctypes binding of libenarf_pose.so (the C ABI declared in include/enarf_pose.h): the bone masks of the pose prior
(the reference's create_mask / pose_to_image_coord for the SMPL property set) on the device.

Like `_lib`, `_mesh_lib` and `_raster_lib` there is no CPU fallback: a missing library, a CPU tensor or a failed call
raises EnarfHipError.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Iterable, Optional

from ._lib import EnarfHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libenarf_pose.so")
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

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libenarf_pose.so (once). Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (torch's HIP runtime first, as in _lib.load)
    if not os.path.exists(LIB_PATH):
        raise EnarfHipError(f"{LIB_PATH} is missing: build it with `python -m enarf_gan_amd.build` (hipcc, gfx950). "
                            "The bone masks have no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.enarf_pose_abi_version() != ABI_VERSION:
        raise EnarfHipError(f"libenarf_pose.so ABI {lib.enarf_pose_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().enarf_pose_last_error().decode(errors="replace")
        if rc == -2:
            raise NotImplementedError(f"{what}: {msg}")
        raise EnarfHipError(f"{what} failed (code {rc}): {msg}")


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
    for name, t in (("pose_to_camera", pose_to_camera), ("intrinsics", intrinsics)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise EnarfHipError(f"bone_masks takes device tensors (there is no CPU fallback); {name} is not one")
        if t.dtype not in (torch.float32, torch.float64):
            raise EnarfHipError(f"bone_masks takes fp32 or fp64 {name}, got {t.dtype}")
    if pose_to_camera.dim() != 4 or tuple(pose_to_camera.shape[1:]) != (NUM_JOINTS, 4, 4):
        raise EnarfHipError(f"bone_masks takes (B, 24, 4, 4) pose_to_camera, got {tuple(pose_to_camera.shape)}")
    B = pose_to_camera.shape[0]
    if tuple(intrinsics.shape) != (B, 3, 3):
        raise EnarfHipError(f"bone_masks takes ({B}, 3, 3) intrinsics, got {tuple(intrinsics.shape)}")
    if intrinsics.device != pose_to_camera.device:
        raise EnarfHipError("bone_masks: pose_to_camera and intrinsics are on different devices")
    S = int(size)
    if not 1 <= S <= MAX_SIZE:
        raise EnarfHipError(f"bone_masks: size {S} outside [1, {MAX_SIZE}]")
    if not math.isfinite(float(thickness)):
        raise EnarfHipError(f"bone_masks: thickness {thickness} is not finite")
    lib = load()
    dev = pose_to_camera.device
    shapes = {"mask": (B, S, S), "disparity": (B, S, S), "part_disparity": (B, NUM_PARTS, S, S),
              "keypoint_mask": (B, NUM_KEYPOINTS, S, S), "pose_2d": (B, NUM_JOINTS, 2)}
    with torch.cuda.device(dev):
        pose = pose_to_camera.to(torch.float64).contiguous()
        K = intrinsics.to(torch.float64).contiguous()
        out = {o: torch.empty(shapes[o], dtype=torch.float64 if o == "pose_2d" else torch.float32, device=dev)
               for o in OUTPUTS if o in outputs}
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ptr = lambda o: out[o].data_ptr() if o in out else None
        check(lib.enarf_pose_bone_masks(pose.data_ptr(), K.data_ptr(), None, B, S, float(thickness),
                                        *(ptr(o) for o in OUTPUTS), stream), "enarf_pose_bone_masks")
    return out
