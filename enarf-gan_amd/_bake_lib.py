"""ctypes binding of libenarf_bake.so (the C ABI declared in include/enarf_bake.h): the texture atlas of an extracted mesh -
the surface point of every texel, the RGBA8 texture from the colours or labels found there, and the deferred textured
shading of the fragment buffers rasterize_mesh returns - on the device.

Loading, return codes and the argument checks more than one binding makes are `_loader`'s. `bake_layout` and
`atlas_corners` restate the atlas layout on the host and need neither the library nor a device.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Tuple

from ._loader import Library, check_tensors, fragment_size, mesh_shapes, on_device, rgb, stream_of, texture_kind
from ._paint_lib import ShadedFragments

ABI_VERSION = 1

MIN_CELL = 6           # c
MIN_ATLAS = 6          # A
MAX_ATLAS = 8192
MAX_SIZE = 4096        # R

_p = C.c_void_p


class PointsArgs(C.Structure):
    _fields_ = [("A", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32), ("reserved", C.c_int32),
                ("V", C.c_int64), ("T", C.c_int64),
                ("vertices", _p), ("triangles", _p), ("points", _p), ("texel_face", _p)]


class ResolveArgs(C.Structure):
    _fields_ = [("count", C.c_int64), ("P", C.c_int32), ("unit", C.c_int32),
                ("neutral", C.c_float * 3), ("fill", C.c_float * 3),
                ("texel_face", _p), ("colors", _p), ("labels", _p), ("palette", _p), ("texture", _p), ("texture_f32", _p)]


class ShadeArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("A", C.c_int32), ("V", C.c_int64), ("T", C.c_int64),
                ("lit", C.c_int32), ("reserved", C.c_int32), ("background", C.c_float * 3), ("reserved2", C.c_float),
                ("pix_to_face", _p), ("bary", _p), ("normals", _p), ("vertices", _p), ("triangles", _p),
                ("texture", _p), ("texture_f32", _p), ("albedo", _p), ("shaded", _p), ("image", _p)]


# every symbol include/enarf_bake.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_bake_abi_version": (C.c_int, []),
    "enarf_bake_last_error": (C.c_char_p, []),
    "enarf_bake_layout": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "enarf_bake_points": (C.c_int, [C.POINTER(PointsArgs), _p]),
    "enarf_bake_resolve": (C.c_int, [C.POINTER(ResolveArgs), _p]),
    "enarf_bake_shade": (C.c_int, [C.POINTER(ShadeArgs), _p]),
}

BakeLayout = namedtuple("BakeLayout", ["cell", "cells_per_row", "capacity"])
BakedPoints = namedtuple("BakedPoints", ["points", "texel_face"])
BakedTexture = namedtuple("BakedTexture", ["texture", "texture_f32"])

_library = Library("bake", ABI_VERSION, SIGNATURES, "The texture bake has no CPU fallback.")
load, check = _library.load, _library.check


def bake_layout(T: int, size: int) -> BakeLayout:
    """BakeLayout(cell c, cells a row n, capacity 2 n n) of T triangles in an atlas of `size` texels a side: c is the
    largest integer >= 6 with 2 (size // c)^2 >= T. ValueError for a size outside [6, 8192] or a T outside [0, 2^31),
    NotImplementedError when the atlas is too small (the message says how large it must be). Pure host arithmetic."""
    try:
        T, A = int(T), int(size)
    except (TypeError, ValueError):
        raise ValueError(f"bake_layout takes a triangle count and an atlas size, got {T!r} and {size!r}") from None
    if not MIN_ATLAS <= A <= MAX_ATLAS:
        raise ValueError(f"bake_layout: atlas size {A} outside [{MIN_ATLAS}, {MAX_ATLAS}]")
    if not 0 <= T < 2 ** 31:
        raise ValueError(f"bake_layout: T = {T} outside [0, 2^31)")
    need = 1
    while 2 * need * need < T:
        need += 1
    c = A // need
    if c < MIN_CELL:
        raise NotImplementedError(f"bake_layout: {T} triangles need {need} cells of {MIN_CELL} texels a row: an atlas of at "
                                  f"least {need * MIN_CELL} texels a side, got {A}")
    n = A // c
    return BakeLayout(c, n, 2 * n * n)


def atlas_corners(T: int, size: int):
    """(T, 3, 2) float64 numpy: the (x, y) position of every triangle corner in atlas texels (exact integers), from the
    layout alone"""
    import numpy as np
    c, n, _ = bake_layout(T, size)
    t = np.arange(int(T), dtype=np.int64)
    q, h = t // 2, t & 1
    origin = np.stack([(q % n) * c, (q // n) * c], axis=-1)                                   # (T, 2)
    local = np.array([[[1, 1], [c - 3, 1], [1, c - 3]], [[c - 1, c - 1], [3, c - 1], [c - 1, 3]]], np.int64)
    return (origin[:, None, :] + local[h]).astype(np.float64)


def check_points_args(vertices, triangles, size, rows) -> Tuple[int, int, int, int, int]:
    """(V, T, A, row0, rows) of a bake_points call, or ValueError / NotImplementedError; touches no device"""
    import torch
    check_tensors("bake_points", dict(triangles=torch.int64), vertices=vertices, triangles=triangles)
    V, T = mesh_shapes("bake_points", vertices, triangles)
    bake_layout(T, size)
    A = int(size)
    if rows is None:
        row0, count = 0, A
    else:
        try:
            row0, stop = (int(x) for x in rows)
        except (TypeError, ValueError):
            raise ValueError(f"bake_points takes rows as (first, stop), got {rows!r}") from None
        count = stop - row0
        if row0 < 0 or count < 1 or stop > A:
            raise ValueError(f"bake_points: rows [{row0}, {stop}) outside the atlas of {A} rows")
    return V, T, A, row0, count


def bake_points(vertices, triangles, size: int, rows=None) -> BakedPoints:
    """BakedPoints(points (3, rows A) fp32, texel_face (rows, A) int32) of the atlas rows [rows[0], rows[1]) (all by
    default), on the mesh's device and its current stream, one launch, no synchronisation."""
    import torch
    V, T, A, row0, count = check_points_args(vertices, triangles, size, rows)
    dev = on_device("bake_points", vertices=vertices, triangles=triangles)
    lib = load()
    keep = [vertices.contiguous(), triangles.contiguous()]
    with torch.cuda.device(dev):
        out = BakedPoints(torch.empty(3, count * A, dtype=torch.float32, device=dev),
                          torch.empty(count, A, dtype=torch.int32, device=dev))
        a = PointsArgs()
        a.A, a.row0, a.rows, a.V, a.T = A, row0, count, V, T
        a.vertices, a.triangles = (t.data_ptr() if t.numel() else None for t in keep)
        a.points, a.texel_face = out.points.data_ptr(), out.texel_face.data_ptr()
        check(lib.enarf_bake_points(C.byref(a), stream_of(dev)), "enarf_bake_points")
    del keep
    return out


def check_resolve_args(texel_face, color, labels, palette, out) -> Tuple[tuple, int, int]:
    """(the shape of texel_face, M, P) of a bake_resolve call (P = 0 in colour mode), or ValueError; touches no device"""
    import torch
    if (color is None) == (labels is None):
        raise ValueError("bake_resolve takes exactly one of color and labels, got " + ("both" if color is not None else "neither"))
    named = dict(texel_face=texel_face)
    if color is not None:
        if palette is not None:
            raise ValueError("bake_resolve: a palette goes with labels, not with color")
        named["color"] = color
    else:
        if palette is None:
            raise ValueError("bake_resolve: labels need a (P, 3) palette")
        named.update(labels=labels, palette=palette)
    check_tensors("bake_resolve", dict(texel_face=torch.int32, labels=torch.int32), **named)
    shape = tuple(texel_face.shape)
    M = texel_face.numel()
    if len(shape) != 2 or not 1 <= M <= MAX_ATLAS * MAX_ATLAS:
        raise ValueError(f"bake_resolve takes (rows, A) texel_face of 1 to {MAX_ATLAS}^2 texels, got {shape}")
    P = 0
    if color is not None:
        if tuple(color.shape) != (3, M):
            raise ValueError(f"bake_resolve takes (3, {M}) color, got {tuple(color.shape)}")
    else:
        if labels.numel() != M or labels.dim() > 2:
            raise ValueError(f"bake_resolve takes {M} labels, got {tuple(labels.shape)}")
        if palette.dim() != 2 or palette.shape[1] != 3 or palette.shape[0] < 1:
            raise ValueError(f"bake_resolve takes a (P, 3) palette with P >= 1, got {tuple(palette.shape)}")
        P = palette.shape[0]
    if out is not None:
        tex, f32 = out
        if not isinstance(tex, torch.Tensor) or tex.dtype != torch.uint8 or tuple(tex.shape) != shape + (4,) or not tex.is_contiguous():
            raise ValueError(f"bake_resolve writes into a contiguous {shape + (4,)} uint8 texture")
        if f32 is not None and (not isinstance(f32, torch.Tensor) or f32.dtype != torch.float32
                                or tuple(f32.shape) != shape + (3,) or not f32.is_contiguous()):
            raise ValueError(f"bake_resolve writes into a contiguous {shape + (3,)} fp32 texture")
    return shape, M, P


def bake_resolve(texel_face, color=None, labels=None, palette=None, fill=0.0, neutral=0.5, want_float: bool = False,
                 unit: bool = False, out=None) -> BakedTexture:
    """BakedTexture(texture (rows, A, 4) uint8, texture_f32 (rows, A, 3) fp32 or None) of the texels texel_face (rows, A)
    names, one launch, no synchronisation. `out` = (texture, texture_f32 or None) writes into given contiguous tensors
    (rows of a whole atlas, say)."""
    import torch
    shape, M, P = check_resolve_args(texel_face, color, labels, palette, out)
    fl, nt = rgb(fill, "bake_resolve", "fill"), rgb(neutral, "bake_resolve", "neutral")
    dev = on_device("bake_resolve", texel_face=texel_face, color=color, labels=labels, palette=palette,
                    texture=None if out is None else out[0], texture_f32=None if out is None else out[1])
    lib = load()
    keep = [None if t is None else t.contiguous() for t in (texel_face, color, labels, palette)]
    with torch.cuda.device(dev):
        if out is not None:
            res = BakedTexture(out[0], out[1])
        else:
            res = BakedTexture(torch.empty(shape + (4,), dtype=torch.uint8, device=dev),
                               torch.empty(shape + (3,), dtype=torch.float32, device=dev) if want_float else None)
        a = ResolveArgs()
        a.count, a.P, a.unit = M, P, int(bool(unit))
        a.neutral[:], a.fill[:] = nt, fl
        a.texel_face, a.colors, a.labels, a.palette = (None if t is None else t.data_ptr() for t in keep)
        a.texture = res.texture.data_ptr()
        a.texture_f32 = None if res.texture_f32 is None else res.texture_f32.data_ptr()
        check(lib.enarf_bake_resolve(C.byref(a), stream_of(dev)), "enarf_bake_resolve")
    del keep
    return res


def check_shade_args(pix_to_face, bary, normals, vertices, triangles, texture) -> Tuple[int, int, int, int, bool]:
    """(R, V, T, A, the texture is fp32) of a shade_textured call, or ValueError / NotImplementedError; touches no device"""
    import torch
    check_tensors("shade_textured", dict(pix_to_face=torch.int64, triangles=torch.int64), pix_to_face=pix_to_face, bary=bary,
                  normals=normals, vertices=vertices, triangles=triangles)
    A, is_f32 = texture_kind("shade_textured", "texture", texture)
    R = fragment_size("shade_textured", MAX_SIZE, pix_to_face, bary, normals)
    V, T = mesh_shapes("shade_textured", vertices, triangles)
    bake_layout(T, A)
    return R, V, T, A, is_f32


def shade_textured(pix_to_face, bary, normals, vertices, triangles, texture, lit: bool = True, background=1.0
                   ) -> ShadedFragments:
    """ShadedFragments(image (R, R, 3) uint8, albedo (R, R, 3) fp32, shaded (R, R, 3) fp32) on the buffers' device and its
    current stream, one launch, no synchronisation; the contract is in include/enarf_bake.h."""
    import torch
    R, V, T, A, is_f32 = check_shade_args(pix_to_face, bary, normals, vertices, triangles, texture)
    bg = rgb(background, "shade_textured", "background")
    dev = on_device("shade_textured", pix_to_face=pix_to_face, bary=bary, normals=normals, vertices=vertices,
                    triangles=triangles, texture=texture)
    lib = load()
    keep = [t.contiguous() for t in (pix_to_face, bary, normals, vertices, triangles, texture)]
    ptr = lambda t: t.data_ptr() if t.numel() else None
    with torch.cuda.device(dev):
        out = ShadedFragments(torch.empty(R, R, 3, dtype=torch.uint8, device=dev),
                              torch.empty(R, R, 3, dtype=torch.float32, device=dev),
                              torch.empty(R, R, 3, dtype=torch.float32, device=dev))
        a = ShadeArgs()
        a.R, a.A, a.V, a.T, a.lit = R, A, V, T, int(bool(lit))
        a.background[:] = bg
        a.pix_to_face, a.bary, a.normals, a.vertices, a.triangles = (ptr(t) for t in keep[:5])
        a.texture, a.texture_f32 = (None, ptr(keep[5])) if is_f32 else (ptr(keep[5]), None)
        a.albedo, a.shaded, a.image = out.albedo.data_ptr(), out.shaded.data_ptr(), out.image.data_ptr()
        check(lib.enarf_bake_shade(C.byref(a), stream_of(dev)), "enarf_bake_shade")
    del keep
    return out
