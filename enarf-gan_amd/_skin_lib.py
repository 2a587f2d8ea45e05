"""ctypes binding of libenarf_skin.so (the C ABI declared in include/enarf_skin.h): the skin weights of mesh vertices from
the tri-plane's part probabilities, and linear-blend posing of the mesh in many poses at once, on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

from ._loader import EnarfHipError, Library, device_of, stream_of

ABI_VERSION = 1

MAX_PARTS = 32
FRAMES_PER_GROUP = 8
INFLUENCES = (4, 8)
PLANE_CH = 96          # feature channels that precede the part-probability planes in the NCHW tri-plane

_p = C.c_void_p


class WeightsArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("max_influences", C.c_int32), ("V", C.c_int64),
                ("clamp_mask", C.c_int32), ("uniform_part_weight", C.c_int32), ("coordinate_scale", C.c_float),
                ("vertices", _p), ("vert_stride", C.c_int64), ("comp_stride", C.c_int64),
                ("parts", _p), ("canonical_pose", _p), ("mask_planes", _p),
                ("joints", _p), ("weights", _p), ("kept_mass", _p), ("valid_bits", _p)]


class PoseArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("F", C.c_int32), ("max_influences", C.c_int32), ("coordinate_scale", C.c_float),
                ("V", C.c_int64), ("vertices", _p), ("vert_stride", C.c_int64), ("comp_stride", C.c_int64),
                ("joints", _p), ("weights", _p), ("parts_rest", _p), ("parts", _p), ("out", _p),
                ("out_frame_stride", C.c_int64)]


# every symbol include/enarf_skin.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_skin_abi_version": (C.c_int, []),
    "enarf_skin_last_error": (C.c_char_p, []),
    "enarf_skin_weights": (C.c_int, [C.POINTER(WeightsArgs), _p]),
    "enarf_skin_pose": (C.c_int, [C.POINTER(PoseArgs), _p]),
}

_library = Library("skin", ABI_VERSION, SIGNATURES, "The skinning kernels have no CPU fallback.")
load, check = _library.load, _library.check


def check_vertices(who: str, shape: Sequence[int]) -> int:
    """V of (V, 3) vertices, or ValueError"""
    shape = tuple(shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who} takes (V, 3) vertices (a transposed (3, V) view is read in place), got {shape}")
    return shape[0]


def check_rest(who: str, shape: Sequence[int]) -> int:
    """P of the rest pose's (1, P, 16) part records, or ValueError"""
    shape = tuple(shape)
    if len(shape) != 3 or shape[0] != 1 or shape[2] != 16:
        raise ValueError(f"{who} takes (1, P, 16) rest part frames (one identity), got {shape}")
    if not 1 <= shape[1] <= MAX_PARTS:
        raise ValueError(f"{who}: {shape[1]} parts, at most {MAX_PARTS} (one bit of the validity mask each)")
    return shape[1]


def check_weights_args(vert_shape, parts_shape, canonical_shape, tri_shape, max_influences) -> Tuple[int, int, int, int]:
    """(V, P, H, W) of a skin_weights call, or ValueError; touches no device"""
    who = "skin_weights"
    if max_influences not in INFLUENCES:
        raise ValueError(f"{who}: max_influences {max_influences!r}, takes 4 or 8")
    V, P = check_vertices(who, vert_shape), check_rest(who, parts_shape)
    canonical_shape, tri_shape = tuple(canonical_shape), tuple(tri_shape)
    if canonical_shape != (P, 4, 4):
        raise ValueError(f"{who} takes ({P}, 4, 4) canonical poses, got {canonical_shape}")
    if len(tri_shape) != 4 or tri_shape[1] != PLANE_CH + 3 * P or tri_shape[0] != 1:
        raise ValueError(f"{who} takes a (1, {PLANE_CH + 3 * P}, H, W) tri-plane, got {tri_shape}")
    H, W = tri_shape[2:]
    if H < 2 or W < 2 or 3 * P * H * W >= 2 ** 30:
        raise ValueError(f"{who}: planes {H} x {W} with {P} parts: H, W >= 2 and 3 P H W < 2^30 floats")
    return V, P, H, W


def check_pose_args(vert_shape, joints_shape, weights_shape, rest_shape, parts_shape, coordinate_scale) -> Tuple[int, int, int, int]:
    """(V, K, P, F) of a skin_pose call, or ValueError; touches no device"""
    who = "skin_pose"
    V, P = check_vertices(who, vert_shape), check_rest(who, rest_shape)
    joints_shape, weights_shape, parts_shape = tuple(joints_shape), tuple(weights_shape), tuple(parts_shape)
    if len(joints_shape) != 2 or joints_shape[0] != V or joints_shape[1] not in INFLUENCES or weights_shape != joints_shape:
        raise ValueError(f"{who} takes ({V}, 4 or 8) joints and weights, got {joints_shape} and {weights_shape}")
    if len(parts_shape) != 3 or parts_shape[1:] != (P, 16):
        raise ValueError(f"{who} takes (F, {P}, 16) target part frames, got {parts_shape}")
    if parts_shape[0] > 65535 * FRAMES_PER_GROUP:
        raise ValueError(f"{who}: {parts_shape[0]} frames, at most {65535 * FRAMES_PER_GROUP} a launch")
    if not float(coordinate_scale) > 0:
        raise ValueError(f"{who}: coordinate_scale {coordinate_scale!r} is not positive")
    return V, joints_shape[1], P, parts_shape[0]


def _vertex_strides(vertices):
    if vertices.shape[0] and min(vertices.stride()) < 0:
        vertices = vertices.contiguous()
    return vertices, vertices.stride(0), vertices.stride(1)


def skin_weights(vertices, parts_rest, canonical_pose, tri_nchw, max_influences: int = 4, clamp_mask: bool = False,
                 uniform_part_weight: bool = False, coordinate_scale: float = 1.0, return_valid_bits: bool = False):
    """(joints (V, K) int32, weights (V, K) fp32, kept_mass (V,) fp32[, valid_bits (V,) int32]) on the vertices' device and
    its current stream, one launch, no synchronisation. The contract is in include/enarf_skin.h."""
    import torch
    V, P, H, W = check_weights_args(vertices.shape, parts_rest.shape, canonical_pose.shape, tri_nchw.shape, max_influences)
    dev = device_of("skin_weights", (torch.float32,), vertices=vertices, parts_rest=parts_rest, canonical_pose=canonical_pose,
                    tri_plane=tri_nchw)
    K = int(max_influences)
    lib = load()
    with torch.cuda.device(dev):
        parts, cpose, tri = parts_rest.contiguous(), canonical_pose.contiguous(), tri_nchw.contiguous()
        vertices, vs, cstr = _vertex_strides(vertices)
        joints = torch.empty((V, K), dtype=torch.int32, device=dev)
        weights = torch.empty((V, K), dtype=torch.float32, device=dev)
        kept = torch.empty((V,), dtype=torch.float32, device=dev)
        bits = torch.empty((V,), dtype=torch.int32, device=dev) if return_valid_bits else None
        if V:
            a = WeightsArgs()
            a.P, a.H, a.W, a.max_influences, a.V = P, H, W, K, V
            a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
            a.coordinate_scale = float(coordinate_scale)
            a.vertices, a.vert_stride, a.comp_stride = vertices.data_ptr(), vs, cstr
            a.parts, a.canonical_pose = parts.data_ptr(), cpose.data_ptr()
            a.mask_planes = tri.data_ptr() + PLANE_CH * H * W * 4
            a.joints, a.weights, a.kept_mass = joints.data_ptr(), weights.data_ptr(), kept.data_ptr()
            a.valid_bits = None if bits is None else bits.data_ptr()
            check(lib.enarf_skin_weights(C.byref(a), stream_of(dev)), "enarf_skin_weights")
    del parts, cpose, tri, vertices
    return (joints, weights, kept, bits) if return_valid_bits else (joints, weights, kept)


def skin_pose(vertices, joints, weights, parts_rest, parts, coordinate_scale: float = 1.0, out=None):
    """out (F, V, 3) fp32 on the vertices' device and its current stream, one launch, no synchronisation. `out` may be a
    slice of a larger tensor: (F, V, 3) with each frame contiguous. The contract is in include/enarf_skin.h."""
    import torch
    V, K, P, F = check_pose_args(vertices.shape, joints.shape, weights.shape, parts_rest.shape, parts.shape, coordinate_scale)
    dev = device_of("skin_pose", (torch.float32, torch.int32), vertices=vertices, joints=joints, weights=weights,
                    parts_rest=parts_rest, parts=parts, out=out)
    if joints.dtype != torch.int32 or any(t.dtype != torch.float32 for t in (vertices, weights, parts_rest, parts)):
        raise EnarfHipError(f"skin_pose takes int32 joints and fp32 vertices, weights and part frames, got {joints.dtype}, "
                            f"{vertices.dtype}, {weights.dtype}, {parts_rest.dtype}, {parts.dtype}")
    if out is not None:
        if out.dtype != torch.float32 or tuple(out.shape) != (F, V, 3):
            raise ValueError(f"skin_pose: out must be ({F}, {V}, 3) fp32, got {tuple(out.shape)} {out.dtype}")
        if V and F and (out.stride(2) != 1 or out.stride(1) != 3 or (F > 1 and out.stride(0) < 3 * V)):
            raise ValueError(f"skin_pose: every frame of out must be contiguous and frames must not overlap, strides {out.stride()}")
    lib = load()
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
        if V and F:
            rest, tgt, jn, wn = parts_rest.contiguous(), parts.contiguous(), joints.contiguous(), weights.contiguous()
            vertices, vs, cstr = _vertex_strides(vertices)
            a = PoseArgs()
            a.P, a.F, a.max_influences, a.coordinate_scale, a.V = P, F, K, float(coordinate_scale), V
            a.vertices, a.vert_stride, a.comp_stride = vertices.data_ptr(), vs, cstr
            a.joints, a.weights, a.parts_rest, a.parts = jn.data_ptr(), wn.data_ptr(), rest.data_ptr(), tgt.data_ptr()
            a.out, a.out_frame_stride = out.data_ptr(), (out.stride(0) if F > 1 else 3 * V)
            check(lib.enarf_skin_pose(C.byref(a), stream_of(dev)), "enarf_skin_pose")
            del rest, tgt, jn, wn
    return out
