"""ctypes binding of libenarf_nrm.so (the C ABI declared in include/enarf_nrm.h): the density of the articulated query with
its spatial gradient at sample points, and the composited field normal of every ray of a march, on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional, Sequence, Tuple

from ._loader import EnarfHipError, Library, device_of, rgb, stream_of

ABI_VERSION = 1

MAX_PARTS = 32
BLOCK = 256            # points (rays) a workgroup takes
MAX_SAMPLES = 128      # Nf
MAX_BATCH = 65535
PLANE_CH = 96          # feature channels that precede the part-probability planes in the NCHW tri-plane
FEAT_DIM = 32
PACK_BYTES = 112192    # one image's MLP pack (kPackBytes in csrc/enarf_device.h; enarf_mlp_pack_bytes() of libenarf_hip.so)
SHADES = {None: -1, "normal": 0, "lit": 1}
FLAG_VALID, FLAG_NORMAL, FLAG_FIELD = 1, 2, 4

_p = C.c_void_p


class GradientArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("N", C.c_int64),
                ("clamp_mask", C.c_int32), ("uniform_part_weight", C.c_int32), ("multiply_density_with_weight", C.c_int32),
                ("reserved", C.c_int32),
                ("points", _p), ("parts", _p), ("canonical_pose", _p),
                ("feat_cl", _p), ("feat_batch_stride", C.c_int64),
                ("mask_planes", _p), ("mask_batch_stride", C.c_int64),
                ("mlp_pack", _p), ("density", _p), ("gradient", _p)]


class RayArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("Nf", C.c_int32), ("n", C.c_int64), ("shade", C.c_int32), ("reserved", C.c_int32),
                ("mask_threshold", C.c_float), ("min_gradient", C.c_float),
                ("background", C.c_float * 3), ("reserved2", C.c_int32),
                ("gradient", _p), ("weights", _p), ("mask", _p), ("fallback", _p), ("flags_in", _p), ("points", _p),
                ("normals", _p), ("flags", _p), ("magnitude", _p), ("image", _p)]


# every symbol include/enarf_nrm.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_nrm_abi_version": (C.c_int, []),
    "enarf_nrm_last_error": (C.c_char_p, []),
    "enarf_nrm_field_gradient": (C.c_int, [C.POINTER(GradientArgs), _p]),
    "enarf_nrm_ray_normals": (C.c_int, [C.POINTER(RayArgs), _p]),
}

RayNormals = namedtuple("RayNormals", ("normals", "flags", "magnitude", "image"))

_library = Library("nrm", ABI_VERSION, SIGNATURES, "The field-normal kernels have no CPU fallback.")
load, check = _library.load, _library.check


def check_gradient_args(points_shape: Sequence[int], parts_shape, canonical_shape, tri_shape, feat_shape,
                        pack_shape) -> Tuple[int, int, int, int, int]:
    """(B, N, P, H, W) of a field_gradient call, or ValueError (NotImplementedError for B above 65535); touches no device"""
    who = "field_gradient"
    points_shape, parts_shape, canonical_shape = tuple(points_shape), tuple(parts_shape), tuple(canonical_shape)
    tri_shape, feat_shape, pack_shape = tuple(tri_shape), tuple(feat_shape), tuple(pack_shape)
    if len(points_shape) != 3 or points_shape[1] != 3 or points_shape[0] < 1:
        raise ValueError(f"{who} takes (B, 3, N) points, got {points_shape}")
    B, _, N = points_shape
    if B > MAX_BATCH:
        raise NotImplementedError(f"{who}: B = {B} above {MAX_BATCH}")
    if len(parts_shape) != 3 or parts_shape[0] != B or parts_shape[2] != 16:
        raise ValueError(f"{who} takes ({B}, P, 16) part records, got {parts_shape}")
    P = parts_shape[1]
    if not 1 <= P <= MAX_PARTS:
        raise ValueError(f"{who}: {P} parts, at most {MAX_PARTS} (one bit of the validity mask each)")
    if canonical_shape != (P, 4, 4):
        raise ValueError(f"{who} takes ({P}, 4, 4) canonical poses, got {canonical_shape}")
    if len(tri_shape) != 4 or tri_shape[1] != PLANE_CH + 3 * P or tri_shape[0] not in (1, B):
        raise ValueError(f"{who} takes a (1 or {B}, {PLANE_CH + 3 * P}, H, W) tri-plane, got {tri_shape}")
    H, W = tri_shape[2:]
    if H < 2 or W < 2 or 3 * P * H * W >= 2 ** 30 or PLANE_CH * H * W >= 2 ** 31:
        raise ValueError(f"{who}: planes {H} x {W} with {P} parts: H, W >= 2, 3 P H W < 2^30 and 96 H W < 2^31 floats")
    if feat_shape != (tri_shape[0], 3, H, W, FEAT_DIM):
        raise ValueError(f"{who} takes ({tri_shape[0]}, 3, {H}, {W}, {FEAT_DIM}) channel-last feature planes, got {feat_shape}")
    if len(pack_shape) != 2 or pack_shape[0] != B or pack_shape[1] != PACK_BYTES:
        raise ValueError(f"{who} takes the ({B}, {PACK_BYTES}) uint8 MLP pack of prepare, got {pack_shape}")
    return B, N, P, H, W


def field_gradient(points, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, clamp_mask: bool = False,
                   uniform_part_weight: bool = False, multiply_density_with_weight: bool = False):
    """(density (B, N), gradient (B, 3, N)) fp32 on the points' device and its current stream, one launch, no
    synchronisation; N = 0 launches nothing. The contract is in include/enarf_nrm.h."""
    import torch
    B, N, P, H, W = check_gradient_args(points.shape, parts.shape, canonical_pose.shape, tri_nchw.shape, feat_cl.shape,
                                        mlp_pack.shape)
    dev = device_of("field_gradient", (torch.float32,), points=points, parts=parts, canonical_pose=canonical_pose,
                    tri_plane=tri_nchw, feat_cl=feat_cl)
    device_of("field_gradient", (torch.uint8,), mlp_pack=mlp_pack)
    if mlp_pack.device != dev:
        raise EnarfHipError(f"field_gradient: mlp_pack is on {mlp_pack.device}, other arguments on {dev}")
    with torch.cuda.device(dev):
        density = torch.empty((B, N), dtype=torch.float32, device=dev)
        gradient = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
        if N == 0:
            return density, gradient
        lib = load()
        pts, prt, cpose, tri = points.contiguous(), parts.contiguous(), canonical_pose.contiguous(), tri_nchw.contiguous()
        fcl, pack = feat_cl.contiguous(), mlp_pack.contiguous()
        a = GradientArgs()
        a.B, a.P, a.H, a.W, a.N = B, P, H, W, N
        a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
        a.multiply_density_with_weight = int(bool(multiply_density_with_weight))
        a.points, a.parts, a.canonical_pose = pts.data_ptr(), prt.data_ptr(), cpose.data_ptr()
        a.feat_cl, a.feat_batch_stride = fcl.data_ptr(), (0 if fcl.shape[0] == 1 else 3 * H * W * FEAT_DIM)
        a.mask_planes = tri.data_ptr() + PLANE_CH * H * W * 4
        a.mask_batch_stride = 0 if tri.shape[0] == 1 else tri.shape[1] * H * W
        a.mlp_pack = pack.data_ptr()
        a.density, a.gradient = density.data_ptr(), gradient.data_ptr()
        check(lib.enarf_nrm_field_gradient(C.byref(a), stream_of(dev)), "enarf_nrm_field_gradient")
        del pts, prt, cpose, tri, fcl, pack
    return density, gradient


def _number(value, name: str) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"ray_normals takes a number as {name}, got {value!r}") from None


def check_ray_args(gradient, weights, mask, fallback, flags, points, shade) -> Tuple[int, int, int]:
    """(B, n, Nf) of a ray_normals call, or ValueError (NotImplementedError for Nf outside [2, 128] and B above 65535);
    shapes, dtypes and values only, touches no device"""
    import torch
    who = "ray_normals"
    named = dict(gradient=gradient, weights=weights, mask=mask)
    if fallback is not None:
        named["fallback"] = fallback
    if points is not None:
        named["points"] = points
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who} takes tensors; {name} is {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{who} takes torch.float32 {name}, got {t.dtype}")
    if mask.dim() < 2:
        raise ValueError(f"{who} takes a (B, n) mask (or (B, H, W)), got {tuple(mask.shape)}")
    B = mask.shape[0]
    n = mask.numel() // B if B else 0
    if B < 1:
        raise ValueError(f"{who} takes a (B, n) mask with B >= 1, got {tuple(mask.shape)}")
    w = tuple(weights.shape)
    if len(w) == 4 and w[1] == 1:
        w = (w[0],) + w[2:]
    if len(w) != 3 or w[:2] != (B, n):
        raise ValueError(f"{who} takes ({B}, {n}, Nf - 1) or ({B}, 1, {n}, Nf - 1) weights, got {tuple(weights.shape)}")
    Nf = w[2] + 1
    if not 2 <= Nf <= MAX_SAMPLES:
        raise NotImplementedError(f"{who}: Nf = {Nf} outside [2, {MAX_SAMPLES}]")
    if B > MAX_BATCH:
        raise NotImplementedError(f"{who}: B = {B} above {MAX_BATCH}")
    if n * Nf >= 2 ** 31:
        raise ValueError(f"{who}: n = {n} with Nf = {Nf}: n Nf must stay below 2^31")
    if tuple(gradient.shape) != (B, 3, n * Nf):
        raise ValueError(f"{who} takes a ({B}, 3, {n * Nf}) gradient (ray-major, sample-minor), got {tuple(gradient.shape)}")
    if (fallback is None) != (flags is None):
        raise ValueError(f"{who}: fallback normals go with their flags (both or neither)")
    if fallback is not None:
        if fallback.numel() != B * n * 3 or fallback.shape[0] != B or fallback.shape[-1] != 3:
            raise ValueError(f"{who} takes ({B}, {n}, 3) fallback normals, got {tuple(fallback.shape)}")
        if not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8:
            raise ValueError(f"{who} takes torch.uint8 flags")
        if flags.numel() != B * n or flags.shape[0] != B:
            raise ValueError(f"{who} takes ({B}, {n}) flags, got {tuple(flags.shape)}")
    if points is not None and (points.numel() != B * n * 3 or points.shape[0] != B or points.shape[-1] != 3):
        raise ValueError(f"{who} takes ({B}, {n}, 3) points, got {tuple(points.shape)}")
    if shade not in SHADES:
        raise ValueError(f"{who}: shade {shade!r} is none of {tuple(SHADES)}")
    if shade == "lit" and points is None:
        raise ValueError(f"{who}: shade='lit' takes points")
    return B, n, Nf


def ray_normals(gradient, weights, mask, fallback=None, flags=None, points=None, shade: Optional[str] = None,
                mask_threshold=0.5, min_gradient=0.0, background=1.0, want_magnitude: bool = False) -> RayNormals:
    """RayNormals(normals (B, n, 3) fp32, flags (B, n) uint8, magnitude (B, n) fp32 or None, image (B, n, 3) uint8 or None)
    on the inputs' device and its current stream, one launch, no synchronisation; with a (B, H, W) mask the outputs are
    (B, H, W[, 3]). The contract is in include/enarf_nrm.h."""
    import torch
    B, n, Nf = check_ray_args(gradient, weights, mask, fallback, flags, points, shade)
    bg = rgb(background, "ray_normals", "background")
    thr, ming = _number(mask_threshold, "mask_threshold"), _number(min_gradient, "min_gradient")
    dev = device_of("ray_normals", (torch.float32,), gradient=gradient, weights=weights, mask=mask, fallback=fallback,
                    points=points)
    if flags is not None and device_of("ray_normals", (torch.uint8,), flags=flags) != dev:
        raise EnarfHipError(f"ray_normals: flags is on {flags.device}, other arguments on {dev}")
    lead = tuple(mask.shape)
    with torch.cuda.device(dev):
        normals = torch.empty(lead + (3,), dtype=torch.float32, device=dev)
        out_flags = torch.empty(lead, dtype=torch.uint8, device=dev)
        magnitude = torch.empty(lead, dtype=torch.float32, device=dev) if want_magnitude else None
        image = torch.empty(lead + (3,), dtype=torch.uint8, device=dev) if shade is not None else None
        if n == 0:
            return RayNormals(normals, out_flags, magnitude, image)
        lib = load()
        keep = [None if t is None else t.contiguous() for t in (gradient, weights, mask, fallback, flags, points)]
        a = RayArgs()
        a.B, a.Nf, a.n, a.shade = B, Nf, n, SHADES[shade]
        a.mask_threshold, a.min_gradient = thr, ming
        a.background[:] = bg
        a.gradient, a.weights, a.mask, a.fallback, a.flags_in, a.points = (None if t is None else t.data_ptr() for t in keep)
        a.normals, a.flags = normals.data_ptr(), out_flags.data_ptr()
        a.magnitude = None if magnitude is None else magnitude.data_ptr()
        a.image = None if image is None else image.data_ptr()
        check(lib.enarf_nrm_ray_normals(C.byref(a), stream_of(dev)), "enarf_nrm_ray_normals")
        del keep
    return RayNormals(normals, out_flags, magnitude, image)
