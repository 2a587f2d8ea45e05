"""ctypes binding of libenarf_nmap.so (the C ABI declared in include/enarf_nmap.h): tangent-space normal maps in the texture
atlas of an extracted mesh - a vector per texel encoded in the frame of the texel's triangle, and the deferred shading of
the fragment buffers rasterize_mesh returns with such a map - on the device.

Loading, return codes and the argument checks more than one binding makes are `_loader`'s; the atlas layout is
`_bake_lib`'s. `tangent_frames` restates the frame on the host and needs neither the library nor a device.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Tuple

from ._bake_lib import MAX_ATLAS, MAX_SIZE, bake_layout
from ._loader import Library, check_tensors, fragment_size, mesh_shapes, on_device, rgb, stream_of, texture_kind

ABI_VERSION = 1

_p = C.c_void_p


class EncodeArgs(C.Structure):
    _fields_ = [("count", C.c_int64), ("V", C.c_int64), ("T", C.c_int64), ("negate", C.c_int32), ("min_length", C.c_float),
                ("texel_face", _p), ("vectors", _p), ("vertices", _p), ("triangles", _p), ("texture", _p), ("texture_f32", _p)]


class ShadeArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("A", C.c_int32), ("V", C.c_int64), ("T", C.c_int64),
                ("lit", C.c_int32), ("reserved", C.c_int32), ("background", C.c_float * 3), ("base_color", C.c_float * 3),
                ("pix_to_face", _p), ("bary", _p), ("normals", _p), ("vertices", _p), ("triangles", _p),
                ("normal_texture", _p), ("normal_texture_f32", _p), ("texture", _p), ("texture_f32", _p),
                ("albedo", _p), ("normal", _p), ("shaded", _p), ("image", _p)]


# every symbol include/enarf_nmap.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_nmap_abi_version": (C.c_int, []),
    "enarf_nmap_last_error": (C.c_char_p, []),
    "enarf_nmap_encode": (C.c_int, [C.POINTER(EncodeArgs), _p]),
    "enarf_nmap_shade": (C.c_int, [C.POINTER(ShadeArgs), _p]),
}

NormalMapTexture = namedtuple("NormalMapTexture", ["texture", "texture_f32"])
NormalMappedFragments = namedtuple("NormalMappedFragments", ["image", "albedo", "normal", "shaded"])

_library = Library("nmap", ABI_VERSION, SIGNATURES, "The normal-map kernels have no CPU fallback.")
load, check = _library.load, _library.check


def tangent_frames(vertices, triangles):
    """(tangent (T, 3), bitangent (T, 3), normal (T, 3) float64 numpy, valid (T,) bool): the frame of include/enarf_nmap.h
    for every triangle of a host mesh - t^ = s e1 / |e1| with s = -1 for odd triangles, n^ = unit(e1 x e2), b^ = t^ x n^ -
    and ((1, 0, 0), (0, 1, 0), (0, 0, 1)), valid False, where a triangle has none. glTF's TANGENT is (t^, -1)."""
    import numpy as np
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(triangles, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < len(v))).all(-1)
    p = v[np.where(inside[:, None], f, 0)] if len(v) else np.zeros((len(f), 3, 3))
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        c = np.cross(e1, e2)
        l1, lc = np.sqrt((e1 * e1).sum(-1)), np.sqrt((c * c).sum(-1))
        valid = inside & (l1 > 0) & np.isfinite(l1) & (lc > 0) & np.isfinite(lc)
        s = np.where(np.arange(len(f)) % 2 == 0, 1.0, -1.0)
        t = np.where(valid[:, None], s[:, None] * e1 / np.where(valid, l1, 1.0)[:, None], [1.0, 0.0, 0.0])
        n = np.where(valid[:, None], c / np.where(valid, lc, 1.0)[:, None], [0.0, 0.0, 1.0])
    return t, np.cross(t, n), n, valid


def check_encode_args(texel_face, vectors, vertices, triangles, min_length, out) -> Tuple[tuple, int, int, int, float]:
    """(the shape of texel_face, count, V, T, min_length) of an encode_normal_map call, or ValueError; touches no device"""
    import torch
    check_tensors("encode_normal_map", dict(texel_face=torch.int32, triangles=torch.int64), texel_face=texel_face,
                  vectors=vectors, vertices=vertices, triangles=triangles)
    shape = tuple(texel_face.shape)
    M = texel_face.numel()
    if len(shape) != 2 or M > MAX_ATLAS * MAX_ATLAS:
        raise ValueError(f"encode_normal_map takes (rows, A) texel_face of at most {MAX_ATLAS}^2 texels, got {shape}")
    if tuple(vectors.shape) != (3, M):
        raise ValueError(f"encode_normal_map takes (3, {M}) vectors (three planes), got {tuple(vectors.shape)}")
    V, T = mesh_shapes("encode_normal_map", vertices, triangles)
    try:
        ml = float(min_length)
    except (TypeError, ValueError):
        raise ValueError(f"encode_normal_map takes a number as min_length, got {min_length!r}") from None
    if not ml >= 0.0:
        raise ValueError(f"encode_normal_map: min_length must be >= 0, got {ml}")
    if out is not None:
        try:
            tex, f32 = out
        except (TypeError, ValueError):
            raise ValueError("encode_normal_map takes out as (texture, texture_f32 or None)") from None
        if not isinstance(tex, torch.Tensor) or tex.dtype != torch.uint8 or tuple(tex.shape) != shape + (4,) or not tex.is_contiguous():
            raise ValueError(f"encode_normal_map writes into a contiguous {shape + (4,)} uint8 texture")
        if f32 is not None and (not isinstance(f32, torch.Tensor) or f32.dtype != torch.float32
                                or tuple(f32.shape) != shape + (3,) or not f32.is_contiguous()):
            raise ValueError(f"encode_normal_map writes into a contiguous {shape + (3,)} fp32 texture")
    return shape, M, V, T, ml


def encode_normal_map(texel_face, vectors, vertices, triangles, negate: bool = True, min_length: float = 0.0,
                      want_float: bool = False, out=None) -> NormalMapTexture:
    """NormalMapTexture(texture (rows, A, 4) uint8, texture_f32 (rows, A, 3) fp32 or None) of the texels texel_face
    (rows, A) names, one launch, no synchronisation. `out` = (texture, texture_f32 or None) writes into given contiguous
    tensors (rows of a whole atlas, say)."""
    import torch
    shape, M, V, T, ml = check_encode_args(texel_face, vectors, vertices, triangles, min_length, out)
    dev = on_device("encode_normal_map", texel_face=texel_face, vectors=vectors, vertices=vertices, triangles=triangles,
                    texture=None if out is None else out[0], texture_f32=None if out is None else out[1])
    lib = load()
    keep = [t.contiguous() for t in (texel_face, vectors, vertices, triangles)]
    ptr = lambda t: t.data_ptr() if t.numel() else None
    with torch.cuda.device(dev):
        if out is not None:
            res = NormalMapTexture(out[0], out[1])
        else:
            res = NormalMapTexture(torch.empty(shape + (4,), dtype=torch.uint8, device=dev),
                                   torch.empty(shape + (3,), dtype=torch.float32, device=dev) if want_float else None)
        a = EncodeArgs()
        a.count, a.V, a.T, a.negate, a.min_length = M, V, T, int(bool(negate)), ml
        a.texel_face, a.vectors, a.vertices, a.triangles = (ptr(t) for t in keep)
        a.texture = ptr(res.texture)
        a.texture_f32 = None if res.texture_f32 is None else ptr(res.texture_f32)
        check(lib.enarf_nmap_encode(C.byref(a), stream_of(dev)), "enarf_nmap_encode")
    del keep
    return res


def check_shade_args(pix_to_face, bary, normals, vertices, triangles, normal_texture, texture):
    """(R, V, T, A, the normal texture is fp32, the albedo texture is fp32 or None without one) of a shade_normal_mapped
    call, or ValueError / NotImplementedError; touches no device"""
    import torch
    who = "shade_normal_mapped"
    check_tensors(who, dict(pix_to_face=torch.int64, triangles=torch.int64), pix_to_face=pix_to_face, bary=bary,
                  normals=normals, vertices=vertices, triangles=triangles)
    A, n_f32 = texture_kind(who, "normal_texture", normal_texture)
    t_f32 = None
    if texture is not None:
        At, t_f32 = texture_kind(who, "texture", texture)
        if At != A:
            raise ValueError(f"{who}: the normal texture has {A} texels a side, the albedo texture {At}: one atlas, one size")
    R = fragment_size(who, MAX_SIZE, pix_to_face, bary, normals)
    V, T = mesh_shapes(who, vertices, triangles)
    bake_layout(T, A)
    return R, V, T, A, n_f32, t_f32


def shade_normal_mapped(pix_to_face, bary, normals, vertices, triangles, normal_texture, texture=None, base_color=1.0,
                        lit: bool = True, background=1.0) -> NormalMappedFragments:
    """NormalMappedFragments(image (R, R, 3) uint8, albedo, normal, shaded (R, R, 3) fp32) on the buffers' device and its
    current stream, one launch, no synchronisation; the contract is in include/enarf_nmap.h."""
    import torch
    R, V, T, A, n_f32, t_f32 = check_shade_args(pix_to_face, bary, normals, vertices, triangles, normal_texture, texture)
    bg = rgb(background, "shade_normal_mapped", "background")
    base = rgb(base_color, "shade_normal_mapped", "base_color")
    dev = on_device("shade_normal_mapped", pix_to_face=pix_to_face, bary=bary, normals=normals, vertices=vertices,
                    triangles=triangles, normal_texture=normal_texture, texture=texture)
    lib = load()
    keep = [None if t is None else t.contiguous() for t in (pix_to_face, bary, normals, vertices, triangles, normal_texture, texture)]
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        out = NormalMappedFragments(torch.empty(R, R, 3, dtype=torch.uint8, device=dev),
                                    *(torch.empty(R, R, 3, dtype=torch.float32, device=dev) for _ in range(3)))
        a = ShadeArgs()
        a.R, a.A, a.V, a.T, a.lit = R, A, V, T, int(bool(lit))
        a.background[:], a.base_color[:] = bg, base
        a.pix_to_face, a.bary, a.normals, a.vertices, a.triangles = (ptr(t) for t in keep[:5])
        a.normal_texture, a.normal_texture_f32 = (None, ptr(keep[5])) if n_f32 else (ptr(keep[5]), None)
        a.texture, a.texture_f32 = (None, ptr(keep[6])) if t_f32 else (ptr(keep[6]), None)
        a.albedo, a.normal, a.shaded, a.image = (t.data_ptr() for t in (out.albedo, out.normal, out.shaded, out.image))
        check(lib.enarf_nmap_shade(C.byref(a), stream_of(dev)), "enarf_nmap_shade")
    del keep
    return out
