"""ctypes binding of libenarf_raster.so (the C ABI declared in include/enarf_raster.h): hard-Phong rasterisation of one
mesh on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from ._loader import EnarfHipError, Library, device_of, stream_of

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

_library = Library("raster", ABI_VERSION, SIGNATURES, "The rasteriser has no CPU fallback.")
load, check = _library.load, _library.check


def rasterize_mesh(vertices, triangles, intrinsics, img_size: int, render_size: int = 512) -> RasterizedMesh:
    """RasterizedMesh(image (R, R, 3) uint8, pix_to_face (R, R) int64, zbuf (R, R) fp32, bary (R, R, 3) fp32,
    normals (R, R, 3) fp32) on vertices' device; the contract is in include/enarf_raster.h."""
    import torch
    dev = device_of("rasterize_mesh", (torch.float32,), vertices=vertices)
    if device_of("rasterize_mesh", (torch.int64,), triangles=triangles) != dev:
        raise EnarfHipError("rasterize_mesh: vertices and triangles are on different devices")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise EnarfHipError(f"rasterize_mesh takes fp32 (V, 3) vertices, got {tuple(vertices.shape)}")
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise EnarfHipError(f"rasterize_mesh takes int64 (T, 3) triangles, got {tuple(triangles.shape)}")
    K = torch.as_tensor(intrinsics)
    if tuple(K.shape) not in ((3, 3), (1, 3, 3)):
        raise EnarfHipError(f"rasterize_mesh takes (3, 3) or (1, 3, 3) intrinsics, got {tuple(K.shape)}")
    lib = load()
    R = int(render_size)
    verts, tris = vertices.contiguous(), triangles.contiguous()
    V, T = verts.shape[0], tris.shape[0]
    with torch.cuda.device(dev):
        K = K.reshape(3, 3).to(device=dev, dtype=torch.float32).contiguous()
        stream = stream_of(dev)
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
