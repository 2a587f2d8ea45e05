"""ctypes binding of libenarf_pgrad.so (the C ABI declared in include/enarf_pgrad.h): the gradient of the articulated query
with respect to its sample points and its part records, on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

from ._loader import EnarfHipError, Library, device_of, stream_of

ABI_VERSION = 1

MAX_PARTS = 32
BLOCK = 256            # points a workgroup takes
PLANE_CH = 96          # feature channels that precede the part-probability planes in the NCHW tri-plane
FEAT_DIM = 32
PACK_BYTES = 112192    # one image's MLP pack (kPackBytes in csrc/enarf_device.h; enarf_mlp_pack_bytes() of libenarf_hip.so)

_p = C.c_void_p


class QueryArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("N", C.c_int64),
                ("clamp_mask", C.c_int32), ("uniform_part_weight", C.c_int32), ("multiply_density_with_weight", C.c_int32),
                ("reserved", C.c_int32),
                ("points", _p), ("parts", _p), ("canonical_pose", _p),
                ("feat_cl", _p), ("feat_batch_stride", C.c_int64),
                ("mask_planes", _p), ("mask_batch_stride", C.c_int64),
                ("mlp_pack", _p), ("g_density", _p), ("g_color", _p),
                ("g_points", _p), ("g_parts", _p), ("workspace", _p)]


# every symbol include/enarf_pgrad.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_pgrad_abi_version": (C.c_int, []),
    "enarf_pgrad_last_error": (C.c_char_p, []),
    "enarf_pgrad_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64]),
    "enarf_pgrad_query": (C.c_int, [C.POINTER(QueryArgs), _p]),
}

_library = Library("pgrad", ABI_VERSION, SIGNATURES, "The pose-gradient kernels have no CPU fallback.")
load, check = _library.load, _library.check


def check_query_args(points_shape: Sequence[int], parts_shape, canonical_shape, tri_shape, feat_shape, pack_shape,
                     g_density_shape, g_color_shape) -> Tuple[int, int, int, int, int]:
    """(B, N, P, H, W) of a query_pose_bwd call, or ValueError; touches no device. A gradient's shape is None when the
    gradient is."""
    who = "query_pose_bwd"
    points_shape, parts_shape, canonical_shape = tuple(points_shape), tuple(parts_shape), tuple(canonical_shape)
    tri_shape, feat_shape, pack_shape = tuple(tri_shape), tuple(feat_shape), tuple(pack_shape)
    if len(points_shape) != 3 or points_shape[1] != 3 or points_shape[0] < 1:
        raise ValueError(f"{who} takes (B, 3, N) points, got {points_shape}")
    B, _, N = points_shape
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
    if g_density_shape is not None and tuple(g_density_shape) not in ((B, N), (B, 1, N)):
        raise ValueError(f"{who} takes ({B}, {N}) or ({B}, 1, {N}) g_density, got {tuple(g_density_shape)}")
    if g_color_shape is not None and tuple(g_color_shape) != (B, 3, N):
        raise ValueError(f"{who} takes ({B}, 3, {N}) g_color, got {tuple(g_color_shape)}")
    return B, N, P, H, W


def query_pose_bwd(points, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, g_density, g_color, clamp_mask: bool = False,
                   uniform_part_weight: bool = False, multiply_density_with_weight: bool = False):
    """(g_points (B, 3, N), g_parts (B, P, 16)) fp32 on the points' device and its current stream, two launches, no
    synchronisation. The contract is in include/enarf_pgrad.h."""
    import torch
    B, N, P, H, W = check_query_args(points.shape, parts.shape, canonical_pose.shape, tri_nchw.shape, feat_cl.shape,
                                     mlp_pack.shape, None if g_density is None else g_density.shape,
                                     None if g_color is None else g_color.shape)
    dev = device_of("query_pose_bwd", (torch.float32,), points=points, parts=parts, canonical_pose=canonical_pose,
                    tri_plane=tri_nchw, feat_cl=feat_cl, g_density=g_density, g_color=g_color)
    device_of("query_pose_bwd", (torch.uint8,), mlp_pack=mlp_pack)
    if mlp_pack.device != dev:
        raise EnarfHipError(f"query_pose_bwd: mlp_pack is on {mlp_pack.device}, other arguments on {dev}")
    lib = load()
    with torch.cuda.device(dev):
        g_points = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
        g_parts = torch.empty((B, P, 16), dtype=torch.float32, device=dev)
        pts, prt, cpose, tri = points.contiguous(), parts.contiguous(), canonical_pose.contiguous(), tri_nchw.contiguous()
        fcl, pack = feat_cl.contiguous(), mlp_pack.contiguous()
        gd = None if g_density is None else g_density.contiguous()
        gc = None if g_color is None else g_color.contiguous()
        ws_bytes = int(lib.enarf_pgrad_workspace_bytes(B, P, N))
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=dev)
        a = QueryArgs()
        a.B, a.P, a.H, a.W, a.N = B, P, H, W, N
        a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
        a.multiply_density_with_weight = int(bool(multiply_density_with_weight))
        a.points = pts.data_ptr() if N else None
        a.parts, a.canonical_pose = prt.data_ptr(), cpose.data_ptr()
        a.feat_cl, a.feat_batch_stride = fcl.data_ptr(), (0 if fcl.shape[0] == 1 else 3 * H * W * FEAT_DIM)
        a.mask_planes = tri.data_ptr() + PLANE_CH * H * W * 4
        a.mask_batch_stride = 0 if tri.shape[0] == 1 else tri.shape[1] * H * W
        a.mlp_pack = pack.data_ptr()
        a.g_density = gd.data_ptr() if (gd is not None and N) else None
        a.g_color = gc.data_ptr() if (gc is not None and N) else None
        a.g_points, a.g_parts, a.workspace = (g_points.data_ptr() if N else None), g_parts.data_ptr(), ws.data_ptr()
        check(lib.enarf_pgrad_query(C.byref(a), stream_of(dev)), "enarf_pgrad_query")
        del pts, prt, cpose, tri, fcl, pack, gd, gc, ws
    return g_points, g_parts
