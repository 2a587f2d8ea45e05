"""ctypes binding of libenarf_raster.so (the C ABI declared in include/enarf_raster.h): hard-Phong rasterisation of one
mesh on the device.

Like `_lib` and `_mesh_lib` there is no CPU fallback: a missing library, a CPU tensor or a failed call raises
EnarfHipError.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import Optional

from ._lib import EnarfHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libenarf_raster.so")
ABI_VERSION = 1

_p = C.c_void_p

# every symbol include/enarf_raster.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_raster_abi_version": (C.c_int, []),
    "enarf_raster_last_error": (C.c_char_p, []),
    "enarf_raster_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "enarf_raster_mesh": (C.c_int, [_p, C.c_int64, _p, C.c_int64, _p, C.c_int, C.c_int, _p, _p, _p, _p, _p, _p, _p]),
}

RasterizedMesh = namedtuple("RasterizedMesh", ["image", "pix_to_face", "zbuf", "bary", "normals"])

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libenarf_raster.so (once). Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (torch's HIP runtime first, as in _lib.load)
    if not os.path.exists(LIB_PATH):
        raise EnarfHipError(f"{LIB_PATH} is missing: build it with `python -m enarf_gan_amd.build` (hipcc, gfx950). "
                            "The rasteriser has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.enarf_raster_abi_version() != ABI_VERSION:
        raise EnarfHipError(f"libenarf_raster.so ABI {lib.enarf_raster_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().enarf_raster_last_error().decode(errors="replace")
        if rc == -2:
            raise NotImplementedError(f"{what}: {msg}")
        raise EnarfHipError(f"{what} failed (code {rc}): {msg}")


def rasterize_mesh(vertices, triangles, intrinsics, img_size: int, render_size: int = 512) -> RasterizedMesh:
    """RasterizedMesh(image (R, R, 3) uint8, pix_to_face (R, R) int64, zbuf (R, R) fp32, bary (R, R, 3) fp32,
    normals (R, R, 3) fp32) on vertices' device; the contract is in include/enarf_raster.h."""
    import torch
    for name, t in (("vertices", vertices), ("triangles", triangles)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise EnarfHipError(f"rasterize_mesh takes device tensors (there is no CPU fallback); {name} is not one")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise EnarfHipError(f"rasterize_mesh takes fp32 (V, 3) vertices, got {tuple(vertices.shape)} {vertices.dtype}")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype != torch.int64:
        raise EnarfHipError(f"rasterize_mesh takes int64 (T, 3) triangles, got {tuple(triangles.shape)} {triangles.dtype}")
    if triangles.device != vertices.device:
        raise EnarfHipError("rasterize_mesh: vertices and triangles are on different devices")
    K = torch.as_tensor(intrinsics)
    if tuple(K.shape) not in ((3, 3), (1, 3, 3)):
        raise EnarfHipError(f"rasterize_mesh takes (3, 3) or (1, 3, 3) intrinsics, got {tuple(K.shape)}")
    lib = load()
    dev = vertices.device
    R = int(render_size)
    verts, tris = vertices.contiguous(), triangles.contiguous()
    V, T = verts.shape[0], tris.shape[0]
    with torch.cuda.device(dev):
        K = K.reshape(3, 3).to(device=dev, dtype=torch.float32).contiguous()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nbytes = lib.enarf_raster_workspace_bytes(V, T, R)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        image = torch.empty(R, R, 3, dtype=torch.uint8, device=dev) if nbytes else None
        out = RasterizedMesh(image, torch.empty(R, R, dtype=torch.int64, device=dev) if nbytes else None,
                             torch.empty(R, R, dtype=torch.float32, device=dev) if nbytes else None,
                             torch.empty(R, R, 3, dtype=torch.float32, device=dev) if nbytes else None,
                             torch.empty(R, R, 3, dtype=torch.float32, device=dev) if nbytes else None)
        ptr = lambda t: t.data_ptr() if t is not None else None   # sizes the library rejects: let it say why
        check(lib.enarf_raster_mesh(verts.data_ptr(), V, tris.data_ptr(), T, K.data_ptr(), int(img_size), R,
                                    ws.data_ptr(), *(ptr(t) for t in out), stream), "enarf_raster_mesh")
    return out
