"""ctypes binding of libenarf_seg.so (the C ABI declared in include/enarf_seg.h): the part that owns a sample point, and
the composition of such labels along the rays of a march into a semantic map, on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

from ._loader import EnarfHipError, Library, device_of, stream_of

ABI_VERSION = 1

MAX_PARTS = 32
MAX_SAMPLES = 128
PLANE_CH = 96          # feature channels that precede the part-probability planes in the NCHW tri-plane

_p = C.c_void_p


class LabelArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("M", C.c_int64),
                ("clamp_mask", C.c_int32), ("uniform_part_weight", C.c_int32),
                ("points", _p), ("point_batch_stride", C.c_int64), ("point_stride", C.c_int64), ("comp_stride", C.c_int64),
                ("image_coord", _p), ("inv_intrinsics", _p), ("depth_min", _p), ("depth_max", _p), ("bins", _p),
                ("n", C.c_int32), ("Nf", C.c_int32),
                ("parts", _p), ("canonical_pose", _p), ("mask_planes", _p), ("mask_batch_stride", C.c_int64),
                ("label", _p), ("top", _p), ("second", _p), ("valid_bits", _p)]


class CompositeArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("n", C.c_int32), ("Nf", C.c_int32), ("P", C.c_int32),
                ("labels", _p), ("fine_weights", _p), ("palette", _p), ("color", _p), ("part_mass", _p), ("part_map", _p)]


# every symbol include/enarf_seg.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_seg_abi_version": (C.c_int, []),
    "enarf_seg_last_error": (C.c_char_p, []),
    "enarf_seg_labels": (C.c_int, [C.POINTER(LabelArgs), _p]),
    "enarf_seg_composite": (C.c_int, [C.POINTER(CompositeArgs), _p]),
}

_library = Library("seg", ABI_VERSION, SIGNATURES, "The segmentation kernels have no CPU fallback.")
load, check = _library.load, _library.check


def check_frame_args(parts_shape: Sequence[int], canonical_shape: Sequence[int], tri_shape: Sequence[int], B: int
                     ) -> Tuple[int, int, int, int]:
    """(P, H, W, floats from one image's part-probability planes to the next) of a labelling call over B images, or
    ValueError; touches no device"""
    parts_shape, canonical_shape, tri_shape = tuple(parts_shape), tuple(canonical_shape), tuple(tri_shape)
    if len(parts_shape) != 3 or parts_shape[2] != 16 or parts_shape[0] != B:
        raise ValueError(f"part_labels takes ({B}, P, 16) part frames, got {parts_shape}")
    P = parts_shape[1]
    if not 1 <= P <= MAX_PARTS:
        raise ValueError(f"part_labels: {P} parts, at most {MAX_PARTS} (one bit of the validity mask each)")
    if canonical_shape != (P, 4, 4):
        raise ValueError(f"part_labels takes ({P}, 4, 4) canonical poses, got {canonical_shape}")
    if len(tri_shape) != 4 or tri_shape[1] != PLANE_CH + 3 * P or tri_shape[0] not in (1, B):
        raise ValueError(f"part_labels takes a (1 or {B}, {PLANE_CH + 3 * P}, H, W) tri-plane, got {tri_shape}")
    H, W = tri_shape[2:]
    if H < 2 or W < 2 or 3 * P * H * W >= 2 ** 30:
        raise ValueError(f"part_labels: planes {H} x {W} with {P} parts: H, W >= 2 and 3 P H W < 2^30 floats")
    return P, H, W, (0 if tri_shape[0] == 1 else tri_shape[1] * H * W)


def check_point_args(shape: Sequence[int], points_last: bool) -> Tuple[int, int]:
    """(B, M) of explicit points, (B, 3, M) or with points_last (M, 3) / (B, M, 3); or ValueError"""
    shape = tuple(shape)
    if points_last:
        if len(shape) not in (2, 3) or shape[-1] != 3:
            raise ValueError(f"part_labels with points_last takes (M, 3) or (B, M, 3) points, got {shape}")
        return (1 if len(shape) == 2 else shape[0]), shape[-2]
    if len(shape) != 3 or shape[1] != 3:
        raise ValueError(f"part_labels takes (B, 3, M) points, got {shape}")
    return shape[0], shape[2]


def check_ray_args(coord_shape, inv_shape, dmin_shape, dmax_shape, bins_shape) -> Tuple[int, int, int]:
    """(B, n, Nf) of a ray-mode call, or ValueError"""
    coord_shape, bins_shape = tuple(coord_shape), tuple(bins_shape)
    if len(coord_shape) == 4 and coord_shape[1] == 1:
        coord_shape = (coord_shape[0],) + coord_shape[2:]
    if len(coord_shape) != 3 or coord_shape[1] != 3:
        raise ValueError(f"part_labels_on_rays takes (B, 3, n) or (B, 1, 3, n) image_coord, got {coord_shape}")
    B, _, n = coord_shape
    if tuple(inv_shape) not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"part_labels_on_rays takes (3, 3) or ({B}, 3, 3) inv_intrinsics, got {tuple(inv_shape)}")
    if tuple(dmin_shape) != (B, n) or tuple(dmax_shape) != (B, n):
        raise ValueError(f"part_labels_on_rays takes ({B}, {n}) depth_min and depth_max, got {tuple(dmin_shape)} and "
                         f"{tuple(dmax_shape)}")
    if len(bins_shape) != 3 or bins_shape[:2] != (B, n) or bins_shape[2] < 1:
        raise ValueError(f"part_labels_on_rays takes ({B}, {n}, Nf) bins, got {bins_shape}")
    return B, n, bins_shape[2]


def check_composite_args(labels_shape, weights_shape, palette_shape) -> Tuple[int, int, int, int]:
    """(B, n, Nf, P) of a semantic_composite call, or ValueError"""
    labels_shape, weights_shape, palette_shape = tuple(labels_shape), tuple(weights_shape), tuple(palette_shape)
    if len(labels_shape) != 3:
        raise ValueError(f"semantic_composite takes (B, n, Nf) labels, got {labels_shape}")
    B, n, Nf = labels_shape
    if not 2 <= Nf <= MAX_SAMPLES:
        raise ValueError(f"semantic_composite: Nf {Nf} outside [2, {MAX_SAMPLES}] (one wavefront per ray, two samples a lane)")
    if len(weights_shape) == 4 and weights_shape[1] == 1:
        weights_shape = (weights_shape[0],) + weights_shape[2:]
    if weights_shape != (B, n, Nf - 1):
        raise ValueError(f"semantic_composite takes ({B}, 1, {n}, {Nf - 1}) fine_weights for labels {labels_shape} (the last "
                         f"sample closes the last interval), got {weights_shape}")
    if len(palette_shape) != 2 or palette_shape[1] != 3 or not 1 <= palette_shape[0] <= MAX_PARTS:
        raise ValueError(f"semantic_composite takes a (P, 3) palette with P <= {MAX_PARTS}, got {palette_shape}")
    return B, n, Nf, palette_shape[0]


def _labels(a: LabelArgs, B: int, M: int, dev, return_valid_bits: bool, keep):
    import torch
    lib = load()
    with torch.cuda.device(dev):
        label = torch.empty((B, M), dtype=torch.int32, device=dev)
        top = torch.empty((B, M), dtype=torch.float32, device=dev)
        second = torch.empty((B, M), dtype=torch.float32, device=dev)
        bits = torch.empty((B, M), dtype=torch.int32, device=dev) if return_valid_bits else None
        if M and B:
            a.label, a.top, a.second = label.data_ptr(), top.data_ptr(), second.data_ptr()
            a.valid_bits = None if bits is None else bits.data_ptr()
            check(lib.enarf_seg_labels(C.byref(a), stream_of(dev)), "enarf_seg_labels")
    del keep
    return (label, top, second, bits) if return_valid_bits else (label, top, second)


def _frame_args(who, parts, canonical_pose, tri_nchw, B, clamp_mask, uniform_part_weight, dev_tensors):
    import torch
    P, H, W, mstride = check_frame_args(parts.shape, canonical_pose.shape, tri_nchw.shape, B)
    dev = device_of(who, (torch.float32,), parts=parts, canonical_pose=canonical_pose, tri_plane=tri_nchw, **dev_tensors)
    parts, cpose, tri = parts.contiguous(), canonical_pose.contiguous(), tri_nchw.contiguous()
    a = LabelArgs()
    a.B, a.P, a.H, a.W = B, P, H, W
    a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
    a.parts, a.canonical_pose = parts.data_ptr(), cpose.data_ptr()
    a.mask_planes, a.mask_batch_stride = tri.data_ptr() + PLANE_CH * H * W * 4, mstride
    return a, dev, [parts, cpose, tri]


def part_labels(points, parts, canonical_pose, tri_nchw, clamp_mask: bool = False, uniform_part_weight: bool = False,
                points_last: bool = False, return_valid_bits: bool = False):
    """(label int32, top fp32, second fp32[, valid_bits int32]), each (B, M), on the points' device and its current stream,
    one launch, no synchronisation. points (B, 3, M), or with `points_last` (M, 3) / (B, M, 3), read where they lie
    through their strides. The contract is in include/enarf_seg.h."""
    B, M = check_point_args(points.shape, points_last)
    a, dev, keep = _frame_args("part_labels", parts, canonical_pose, tri_nchw, B, clamp_mask, uniform_part_weight,
                               dict(points=points))
    st = points.stride()
    if M and min(st) < 0:
        points = points.contiguous()
        st = points.stride()
    a.M = M
    a.points = points.data_ptr() if M else None
    if points_last:
        a.point_batch_stride = 0 if points.dim() == 2 else st[0]
        a.point_stride, a.comp_stride = st[-2], st[-1]
    else:
        a.point_batch_stride, a.comp_stride, a.point_stride = st
    return _labels(a, B, M, dev, return_valid_bits, keep + [points])


def part_labels_on_rays(image_coord, inv_intrinsics, depth_min, depth_max, bins, parts, canonical_pose, tri_nchw,
                        clamp_mask: bool = False, uniform_part_weight: bool = False, return_valid_bits: bool = False):
    """The same outputs as (B, n, Nf) tensors for the fine samples of a march, the points formed in the kernel from the
    march's taps (depth_min, depth_max (B, n), bins (B, n, Nf)) exactly as the march forms them."""
    import torch
    B, n, Nf = check_ray_args(image_coord.shape, inv_intrinsics.shape, depth_min.shape, depth_max.shape, bins.shape)
    a, dev, keep = _frame_args("part_labels_on_rays", parts, canonical_pose, tri_nchw, B, clamp_mask, uniform_part_weight,
                               dict(image_coord=image_coord, inv_intrinsics=inv_intrinsics, depth_min=depth_min,
                                    depth_max=depth_max, bins=bins))
    coord = image_coord.reshape(B, 3, n).contiguous()
    Ki = inv_intrinsics if inv_intrinsics.dim() == 3 else inv_intrinsics[None].expand(B, -1, -1)
    Ki, dmin, dmax, bins = Ki.contiguous(), depth_min.contiguous(), depth_max.contiguous(), bins.contiguous()
    a.M, a.n, a.Nf, a.points = n * Nf, n, Nf, None
    a.image_coord, a.inv_intrinsics = coord.data_ptr(), Ki.data_ptr()
    a.depth_min, a.depth_max, a.bins = dmin.data_ptr(), dmax.data_ptr(), bins.data_ptr()
    out = _labels(a, B, n * Nf, dev, return_valid_bits, keep + [coord, Ki, dmin, dmax, bins])
    return tuple(t.view(B, n, Nf) for t in out)


def semantic_composite(labels, fine_weights, palette):
    """(color (B, 3, n) fp32, part_map (B, n) int32, part_mass (B, n) fp32) on the labels' device and its current stream,
    one launch, no synchronisation: labels (B, n, Nf) int32, fine_weights (B, 1, n, Nf - 1) or (B, n, Nf - 1) fp32 as the
    march returns them, palette (P, 3) fp32. The contract is in include/enarf_seg.h."""
    import torch
    B, n, Nf, P = check_composite_args(labels.shape, fine_weights.shape, palette.shape)
    dev = device_of("semantic_composite", (torch.float32, torch.int32), labels=labels, fine_weights=fine_weights,
                    palette=palette)
    if labels.dtype != torch.int32 or fine_weights.dtype != torch.float32 or palette.dtype != torch.float32:
        raise EnarfHipError(f"semantic_composite takes int32 labels and fp32 fine_weights and palette, got {labels.dtype}, "
                            f"{fine_weights.dtype}, {palette.dtype}")
    lib = load()
    with torch.cuda.device(dev):
        labels, weights, palette = labels.contiguous(), fine_weights.contiguous(), palette.contiguous()
        color = torch.empty((B, 3, n), dtype=torch.float32, device=dev)
        part_map = torch.empty((B, n), dtype=torch.int32, device=dev)
        part_mass = torch.empty((B, n), dtype=torch.float32, device=dev)
        if B * n:
            a = CompositeArgs()
            a.B, a.n, a.Nf, a.P = B, n, Nf, P
            a.labels, a.fine_weights, a.palette = labels.data_ptr(), weights.data_ptr(), palette.data_ptr()
            a.color, a.part_mass, a.part_map = color.data_ptr(), part_mass.data_ptr(), part_map.data_ptr()
            check(lib.enarf_seg_composite(C.byref(a), stream_of(dev)), "enarf_seg_composite")
    return color, part_map, part_mass
