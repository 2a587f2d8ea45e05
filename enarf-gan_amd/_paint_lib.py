"""ctypes binding of libenarf_paint.so (the C ABI declared in include/enarf_paint.h): deferred shading of the fragment
buffers rasterize_mesh returns, with a colour or a part label per vertex, on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Tuple

from ._loader import Library, device_of, stream_of

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


def _rgb(value, name: str) -> Tuple[float, float, float]:
    """a number or three numbers -> three floats, or ValueError"""
    try:
        v = [float(value)] * 3 if not hasattr(value, "__len__") else [float(x) for x in value]
    except (TypeError, ValueError):
        raise ValueError(f"shade_fragments takes a number or three numbers as {name}, got {value!r}") from None
    if len(v) != 3:
        raise ValueError(f"shade_fragments takes a number or three numbers as {name}, got {len(v)} values")
    return v[0], v[1], v[2]


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
    want = dict(pix_to_face=torch.int64, triangles=torch.int64, vertex_labels=torch.int32)
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"shade_fragments takes tensors; {name} is {type(t).__name__}")
        if t.dtype != want.get(name, torch.float32):
            raise ValueError(f"shade_fragments takes {want.get(name, torch.float32)} {name}, got {t.dtype}")
    shape = tuple(pix_to_face.shape)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError(f"shade_fragments takes (R, R) pix_to_face, got {shape}")
    R = shape[0]
    if not 1 <= R <= MAX_SIZE:
        raise ValueError(f"shade_fragments: render size {R} outside [1, {MAX_SIZE}]")
    for name in ("bary", "normals"):
        if tuple(named[name].shape) != (R, R, 3):
            raise ValueError(f"shade_fragments takes ({R}, {R}, 3) {name}, got {tuple(named[name].shape)}")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"shade_fragments takes (V, 3) vertices, got {tuple(vertices.shape)}")
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"shade_fragments takes (T, 3) triangles, got {tuple(triangles.shape)}")
    V, T = vertices.shape[0], triangles.shape[0]
    if V >= 2 ** 31 or T >= 2 ** 31:
        raise ValueError(f"shade_fragments: V = {V}, T = {T}: both must lie in [0, 2^31)")
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
    bg, nt = _rgb(background, "background"), _rgb(neutral, "neutral")
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
