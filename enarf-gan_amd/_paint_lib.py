"""ctypes binding of libenarf_paint.so (the C ABI declared in include/enarf_paint.h): deferred shading of the fragment
buffers rasterize_mesh returns, with a colour or a part label per vertex, on the device.

Loading, return codes, the device-argument checks and the shape checks of a mesh and its fragment buffers are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Tuple

from ._loader import Library, check_tensors, device_of, fragment_size, mesh_shapes, rgb, stream_of

ABI_VERSION = 1

MAX_SIZE = 4096        # R

_p = C.c_void_p


class ShadeArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("P", C.c_int32), ("V", C.c_int64), ("T", C.c_int64),
                ("lit", C.c_int32), ("reserved", C.c_int32),
                ("neutral", C.c_float * 3), ("background", C.c_float * 3),
                ("pix_to_face", _p), ("bary", _p), ("normals", _p), ("vertices", _p), ("triangles", _p),
                ("vertex_colors", _p), ("vertex_labels", _p), ("palette", _p),
                ("albedo", _p), ("shaded", _p), ("image", _p)]


# every symbol include/enarf_paint.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_paint_abi_version": (C.c_int, []),
    "enarf_paint_last_error": (C.c_char_p, []),
    "enarf_paint_shade": (C.c_int, [C.POINTER(ShadeArgs), _p]),
}

ShadedFragments = namedtuple("ShadedFragments", ["image", "albedo", "shaded"])

_library = Library("paint", ABI_VERSION, SIGNATURES, "The deferred shading kernel has no CPU fallback.")
load, check = _library.load, _library.check


def check_shade_args(pix_to_face, bary, normals, vertices, triangles, vertex_colors, vertex_labels, palette
                     ) -> Tuple[int, int, int, int]:
    """(R, V, T, P) of a shade_fragments call (P = 0 in colour mode), or ValueError; shapes and dtypes only, touches no
    device"""
    import torch
    if (vertex_colors is None) == (vertex_labels is None):
        raise ValueError("shade_fragments takes exactly one of vertex_colors and vertex_labels, got "
                         + ("both" if vertex_colors is not None else "neither"))
    named = dict(pix_to_face=pix_to_face, bary=bary, normals=normals, vertices=vertices, triangles=triangles)
    if vertex_colors is not None:
        if palette is not None:
            raise ValueError("shade_fragments: a palette goes with vertex_labels, not with vertex_colors")
        named["vertex_colors"] = vertex_colors
    else:
        if palette is None:
            raise ValueError("shade_fragments: vertex_labels need a (P, 3) palette")
        named.update(vertex_labels=vertex_labels, palette=palette)
    who = "shade_fragments"
    check_tensors(who, dict(pix_to_face=torch.int64, triangles=torch.int64, vertex_labels=torch.int32), **named)
    R = fragment_size(who, MAX_SIZE, pix_to_face, bary, normals)
    V, T = mesh_shapes(who, vertices, triangles)
    P = 0
    if vertex_colors is not None:
        if tuple(vertex_colors.shape) != (V, 3):
            raise ValueError(f"shade_fragments takes ({V}, 3) vertex_colors, got {tuple(vertex_colors.shape)}")
    else:
        if tuple(vertex_labels.shape) != (V,):
            raise ValueError(f"shade_fragments takes ({V},) vertex_labels, got {tuple(vertex_labels.shape)}")
        if palette.dim() != 2 or palette.shape[1] != 3 or palette.shape[0] < 1:
            raise ValueError(f"shade_fragments takes a (P, 3) palette with P >= 1, got {tuple(palette.shape)}")
        P = palette.shape[0]
    return R, V, T, P


def shade_fragments(pix_to_face, bary, normals, vertices, triangles, vertex_colors=None, vertex_labels=None, palette=None,
                    lit: bool = True, background=1.0, neutral=0.5) -> ShadedFragments:
    """ShadedFragments(image (R, R, 3) uint8, albedo (R, R, 3) fp32, shaded (R, R, 3) fp32) on the buffers' device and its
    current stream, one launch, no synchronisation; the contract is in include/enarf_paint.h."""
    import torch
    R, V, T, P = check_shade_args(pix_to_face, bary, normals, vertices, triangles, vertex_colors, vertex_labels, palette)
    bg, nt = rgb(background, "shade_fragments", "background"), rgb(neutral, "shade_fragments", "neutral")
    dev = device_of("shade_fragments", (torch.float32, torch.int64, torch.int32), pix_to_face=pix_to_face, bary=bary,
                    normals=normals, vertices=vertices, triangles=triangles, vertex_colors=vertex_colors,
                    vertex_labels=vertex_labels, palette=palette)
    lib = load()
    keep = [t.contiguous() for t in (pix_to_face, bary, normals, vertices, triangles)]
    paint = [None if t is None else t.contiguous() for t in (vertex_colors, vertex_labels, palette)]
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        out = ShadedFragments(torch.empty(R, R, 3, dtype=torch.uint8, device=dev),
                              torch.empty(R, R, 3, dtype=torch.float32, device=dev),
                              torch.empty(R, R, 3, dtype=torch.float32, device=dev))
        a = ShadeArgs()
        a.R, a.P, a.V, a.T, a.lit = R, P, V, T, int(bool(lit))
        a.neutral[:], a.background[:] = nt, bg
        a.pix_to_face, a.bary, a.normals, a.vertices, a.triangles = (ptr(t) for t in keep)
        a.vertex_colors, a.vertex_labels, a.palette = (ptr(t) for t in paint)
        a.albedo, a.shaded, a.image = out.albedo.data_ptr(), out.shaded.data_ptr(), out.image.data_ptr()
        check(lib.enarf_paint_shade(C.byref(a), stream_of(dev)), "enarf_paint_shade")
    del keep, paint
    return out
