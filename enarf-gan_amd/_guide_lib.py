"""ctypes binding of libenarf_guide.so (the C ABI declared in include/enarf_guide.h): the mask-guidance loss of the
GAN's generator (`nerf_patch_loss` of the reference's models/loss.py), forward and backward, on the device.

Loading, return codes and the device-argument checks are `_loader`'s. Shapes and the ratio are checked before anything
touches the device (ValueError), so those checks run without one.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

from ._loader import Library, device_of, stream_of

ABI_VERSION = 1

MAX_BLOCKS = 512                                     # ENARF_GUIDE_MAX_BLOCKS
WORK_BYTES = 2 * MAX_BLOCKS * 8 + (4 * 256 + 2 * MAX_BLOCKS) * 4     # ENARF_GUIDE_WORK_BYTES
STATE_INTS = 4 + MAX_BLOCKS                          # ENARF_GUIDE_STATE_INTS

_p = C.c_void_p
_i64 = C.c_int64

# every symbol include/enarf_guide.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_guide_abi_version": (C.c_int, []),
    "enarf_guide_last_error": (C.c_char_p, []),
    "enarf_guide_loss_fwd": (C.c_int, [_p, _p, _i64, C.c_int, C.c_int, _i64, C.c_int, C.c_double, _p, _p, _p, _p]),
    "enarf_guide_loss_bwd": (C.c_int, [_p, _p, _i64, C.c_int, C.c_int, _i64, C.c_int, C.c_double, _p, _p, _p, _p]),
}

_library = Library("guide", ABI_VERSION, SIGNATURES, "The mask-guidance loss has no CPU fallback.")
load, check = _library.load, _library.check


def geometry(n: int) -> Tuple[int, int]:
    """(chunk_len, chunks) of include/enarf_guide.h for n values"""
    blocks0 = min((n + 255) // 256, MAX_BLOCKS)
    chunk_len = ((n + blocks0 - 1) // blocks0 + 255) // 256 * 256
    return chunk_len, (n + chunk_len - 1) // chunk_len


def check_shapes(fake_mask, bone_mask, background_ratio: float) -> Tuple[int, int, int, int, bool]:
    """(B, s, S, k, with_push) of a loss call, or ValueError; needs no device. fake_mask is (..., s, s); bone_mask has
    the same shape, or both are 3-D, (B, s, s) against (B, S, S) with S // s >= 1 and S // (S // s) == s (what
    F.max_pool2d(bone_mask, rate, rate, 0) turns into the mask's size). k = int(N * background_ratio), as Python
    computes it."""
    if fake_mask.dim() < 2 or fake_mask.shape[-1] != fake_mask.shape[-2]:
        raise ValueError(f"fake_mask must be (..., s, s), got {tuple(fake_mask.shape)}")
    if fake_mask.dim() != bone_mask.dim():
        raise ValueError(f"fake_mask and bone_mask must have the same number of dimensions, got {tuple(fake_mask.shape)} "
                         f"and {tuple(bone_mask.shape)}")
    s = fake_mask.shape[-1]
    n = fake_mask.numel()
    if n == 0:
        raise ValueError(f"fake_mask {tuple(fake_mask.shape)} is empty")
    if n >= 1 << 31:
        raise ValueError(f"fake_mask holds {n} values, the limit is 2^31 - 1")
    if tuple(bone_mask.shape) == tuple(fake_mask.shape):
        S = s
    else:
        if fake_mask.dim() != 3:
            raise ValueError(f"a bone mask of another resolution takes 3-D masks, got {tuple(fake_mask.shape)} and "
                             f"{tuple(bone_mask.shape)}")
        if bone_mask.shape[0] != fake_mask.shape[0] or bone_mask.shape[1] != bone_mask.shape[2]:
            raise ValueError(f"bone_mask must be ({fake_mask.shape[0]}, S, S), got {tuple(bone_mask.shape)}")
        S = bone_mask.shape[-1]
        rate = S // s
        if rate < 1:
            raise ValueError(f"bone_mask side {S} is below the mask's {s}: a rate of 0")
        if S // rate != s:
            raise ValueError(f"a {S} x {S} bone mask pooled by {rate} is {S // rate} x {S // rate}, not {s} x {s}")
    with_push = background_ratio > 0
    k = int(n * background_ratio) if with_push else 0
    if k > n:
        raise ValueError(f"background_ratio {background_ratio} selects k = {k} of {n} values")
    return n // (s * s), s, S, k, with_push


def loss_fwd(fake_mask, bone_mask, background_ratio: float, coef: float):
    """((3,) fp32 device tensor [loss, push, bone], state for `loss_bwd`) on fake_mask's device and its current stream;
    no host synchronisation."""
    import torch
    B, s, S, k, with_push = check_shapes(fake_mask, bone_mask, background_ratio)
    dev = device_of("mask_guidance_loss", (torch.float32,), fake_mask=fake_mask, bone_mask=bone_mask)
    lib = load()
    with torch.cuda.device(dev):
        fake, bone = fake_mask.contiguous(), bone_mask.contiguous()
        work = torch.empty(WORK_BYTES // 8, dtype=torch.float64, device=dev)
        state = torch.empty(STATE_INTS, dtype=torch.int32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        stream = stream_of(dev)
        check(lib.enarf_guide_loss_fwd(fake.data_ptr(), bone.data_ptr(), B, s, S, k, int(with_push), float(coef),
                                       work.data_ptr(), state.data_ptr(), out.data_ptr(), stream), "enarf_guide_loss_fwd")
    return out, state


def loss_bwd(fake_mask, bone_mask, background_ratio: float, coef: float, state, up):
    """d fake_mask (fake_mask's shape) from the upstream gradient `up` of the loss (a 0-dim fp32 device tensor, read on
    the device) and the forward's `state`."""
    import torch
    B, s, S, k, with_push = check_shapes(fake_mask, bone_mask, background_ratio)
    dev = device_of("mask_guidance_loss backward", (torch.float32,), fake_mask=fake_mask, bone_mask=bone_mask, up=up)
    if up.numel() != 1:
        raise ValueError(f"the upstream gradient must be a scalar, got {tuple(up.shape)}")
    lib = load()
    with torch.cuda.device(dev):
        fake, bone, up = fake_mask.contiguous(), bone_mask.contiguous(), up.contiguous()
        d_fake = torch.empty_like(fake)
        stream = stream_of(dev)
        check(lib.enarf_guide_loss_bwd(fake.data_ptr(), bone.data_ptr(), B, s, S, k, int(with_push), float(coef),
                                       state.data_ptr(), up.data_ptr(), d_fake.data_ptr(), stream), "enarf_guide_loss_bwd")
    return d_fake.view(fake_mask.shape)
