"""ctypes binding of libenarf_anim.so (the C ABI declared in include/enarf_anim.h): the reference's interpolate_pose with
an optional turntable angle per frame, and the conversion of rendered frames to 8-bit images, on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

from ._loader import EnarfHipError, Library, device_of, stream_of

ABI_VERSION = 1

MAX_JOINTS = 64
MAX_SIZE = 4096

_p = C.c_void_p

# every symbol include/enarf_anim.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_anim_abi_version": (C.c_int, []),
    "enarf_anim_last_error": (C.c_char_p, []),
    "enarf_anim_interpolate_pose": (C.c_int, [_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p,
                                              _p]),
    "enarf_anim_compose_frames": (C.c_int, [_p, _p, _p, C.c_int64, C.c_float, C.c_int64, C.c_int, _p, _p, _p]),
}

_library = Library("anim", ABI_VERSION, SIGNATURES, "The animation kernels have no CPU fallback.")
load, check = _library.load, _library.check


def check_pose_args(shape: Sequence[int], parents, num: int, loop: bool) -> Tuple[int, int, list]:
    """(K, J, parents as a list of ints) of an interpolate_pose call, or ValueError; touches no device. The reference
    raises (from np.concatenate) when num is not a multiple of the number of segments; the other cases it cannot run."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 4 or shape[2:] != (4, 4) or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"interpolate_pose takes (K, J, 4, 4) key poses with K, J >= 1, got {shape}")
    K, J = shape[:2]
    if J > MAX_JOINTS:
        raise ValueError(f"interpolate_pose: {J} joints, at most {MAX_JOINTS} (one lane of a wavefront each)")
    par = [int(v) for v in parents]
    if len(par) != J:
        raise ValueError(f"interpolate_pose: {len(par)} parents for {J} joints")
    if par[0] != -1 or any(not 0 <= par[j] < j for j in range(1, J)):
        raise ValueError(f"interpolate_pose: parents must be root-first (parents[0] = -1, 0 <= parents[j] < j), got {par}")
    num = int(num)
    if num < 1:
        raise ValueError(f"interpolate_pose: num {num} < 1")
    if not loop and (K < 2 or num < 2):
        raise ValueError(f"interpolate_pose: without loop at least 2 key poses and 2 frames are needed, got {K} and {num}")
    segments = K if loop else K - 1
    if num % segments:
        raise ValueError(f"interpolate_pose: num {num} is not a multiple of the {segments} segments "
                         f"({'K' if loop else 'K - 1'}): the reference's blocks of num // segments frames do not fill it")
    return K, J, par


def interpolate_pose(key_poses, parents, num: int, loop: bool = True, orbit=None, want_f32: bool = False,
                     want_bone_length: bool = False):
    """(poses (num, J, 4, 4) fp64, the same rounded to fp32 or None, bone_length (num, J - 1, 1) fp32 or None) on
    key_poses' device and its current stream, one launch, no synchronisation. key_poses (K, J, 4, 4) is a device tensor,
    fp64 or fp32 (widened, which is exact); orbit None or a (num,) device tensor of angles; parents a host sequence. The
    contract is in include/enarf_anim.h."""
    import torch
    K, J, par = check_pose_args(key_poses.shape, parents, num, loop)
    num = int(num)
    if orbit is not None and tuple(orbit.shape) != (num,):
        raise ValueError(f"interpolate_pose: orbit takes ({num},) angles, got {tuple(orbit.shape)}")
    dev = device_of("interpolate_pose", (torch.float32, torch.float64), pose_3d=key_poses, orbit=orbit)
    lib = load()
    with torch.cuda.device(dev):
        key = key_poses.to(torch.float64).contiguous()
        angles = None if orbit is None else orbit.to(torch.float64).contiguous()
        poses = torch.empty((num, J, 4, 4), dtype=torch.float64, device=dev)
        poses32 = torch.empty((num, J, 4, 4), dtype=torch.float32, device=dev) if want_f32 else None
        bone = torch.empty((num, J - 1, 1), dtype=torch.float32, device=dev) if want_bone_length else None
        ptr = lambda t: None if t is None else t.data_ptr()
        check(lib.enarf_anim_interpolate_pose(key.data_ptr(), (C.c_int32 * J)(*par), K, J, num, int(bool(loop)), ptr(angles),
                                              poses.data_ptr(), ptr(poses32), ptr(bone), stream_of(dev)),
              "enarf_anim_interpolate_pose")
    return poses, poses32, bone


def check_compose_args(color_shape, mask_shape, background) -> Tuple[int, int]:
    """(F, S) of a compose_frames call, or ValueError; touches no device"""
    color_shape, mask_shape = tuple(color_shape), tuple(mask_shape)
    if len(color_shape) == 4:
        color_shape = color_shape[:2] + (color_shape[2] * color_shape[3],)
    if len(mask_shape) == 3:
        mask_shape = mask_shape[:1] + (mask_shape[1] * mask_shape[2],)
    if len(color_shape) != 3 or color_shape[1] != 3:
        raise ValueError(f"compose_frames takes (F, 3, n) or (F, 3, S, S) colour, got {color_shape}")
    F, _, n = color_shape
    S = int(round(n ** 0.5))
    if S * S != n or not 1 <= S <= MAX_SIZE:
        raise ValueError(f"compose_frames: {n} pixels a frame are not S x S with 1 <= S <= {MAX_SIZE}")
    if mask_shape != (F, n):
        raise ValueError(f"compose_frames takes ({F}, {n}) or ({F}, {S}, {S}) mask, got {mask_shape}")
    if hasattr(background, "shape"):
        b = tuple(background.shape)
        if len(b) == 4:
            b = b[:2] + (b[2] * b[3],)
        if b not in ((1, 3, n), (F, 3, n)):
            raise ValueError(f"compose_frames takes a scalar, (1, 3, {S}, {S}) or ({F}, 3, {S}, {S}) background, got "
                             f"{tuple(background.shape)}")
    else:
        float(background)
    return F, S


def compose_frames(color, mask, background=-1.0, want_masks: bool = True, out=None):
    """(frames (F, S, S, 3) uint8, masks (F, S, S) uint8 or None) on color's device and its current stream, one launch, no
    synchronisation. color (F, 3, n) or (F, 3, S, S) and mask (F, n) or (F, S, S) are fp32 device tensors; background a
    number, one shared (1, 3, S, S) image or (F, 3, S, S) images; `out` = (frames, masks or None) are contiguous uint8
    device tensors of those shapes to write into. The contract is in include/enarf_anim.h."""
    import torch
    F, S = check_compose_args(color.shape, mask.shape, background)
    bg: Optional["torch.Tensor"] = background if hasattr(background, "shape") else None
    dev = device_of("compose_frames", (torch.float32,), color=color, mask=mask, background=bg)
    lib = load()
    with torch.cuda.device(dev):
        color, mask = color.contiguous(), mask.contiguous()
        bg = None if bg is None else bg.contiguous()
        stride = 0 if bg is None or bg.shape[0] == 1 else 3 * S * S
        if out is None:
            frames = torch.empty((F, S, S, 3), dtype=torch.uint8, device=dev)
            masks = torch.empty((F, S, S), dtype=torch.uint8, device=dev) if want_masks else None
        else:
            frames, masks = out[0], (out[1] if want_masks else None)
            for t, shape in ((frames, (F, S, S, 3)), (masks, (F, S, S))):
                if t is not None and not (t.is_cuda and t.device == dev and t.dtype == torch.uint8 and t.is_contiguous()
                                          and tuple(t.shape) == shape):
                    raise ValueError(f"compose_frames: out takes contiguous uint8 tensors {(F, S, S, 3)} and {(F, S, S)} on {dev}")
        given = None
        if frames.data_ptr() % 4 or (masks is not None and masks.data_ptr() % 4):   # a slice at an odd byte: the stores
            given = (frames, masks)                                                # are dwords, so go through a copy
            frames, masks = torch.empty_like(frames), (None if masks is None else torch.empty_like(masks))
        check(lib.enarf_anim_compose_frames(color.data_ptr(), mask.data_ptr(), None if bg is None else bg.data_ptr(), stride,
                                            0.0 if bg is not None else float(background), F, S, frames.data_ptr(),
                                            None if masks is None else masks.data_ptr(), stream_of(dev)),
              "enarf_anim_compose_frames")
        if given is not None:
            given[0].copy_(frames)
            if masks is not None:
                given[1].copy_(masks)
            frames, masks = given
    return frames, masks
