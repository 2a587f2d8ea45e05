"""ctypes binding of libenarf_mesh.so (the C ABI declared in include/enarf_mesh.h): marching cubes on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C

from ._loader import EnarfHipError, Library, device_of, stream_of

ABI_VERSION = 1

_p = C.c_void_p

# every symbol include/enarf_mesh.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_mesh_abi_version": (C.c_int, []),
    "enarf_mesh_last_error": (C.c_char_p, []),
    "enarf_mesh_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "enarf_mesh_count": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p]),
    "enarf_mesh_emit": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, _p]),
}

_library = Library("mesh", ABI_VERSION, SIGNATURES, "Marching cubes has no CPU fallback.")
load, check = _library.load, _library.check


def marching_cubes(volume, iso: float):
    """(vertices (V, 3) fp32, triangles (T, 3) int64) on volume's device; the contract is in include/enarf_mesh.h."""
    import torch
    dev = device_of("marching_cubes", (torch.float32,), volume=volume)
    if volume.dim() != 3:
        raise EnarfHipError(f"marching_cubes takes an fp32 (X, Y, Z) volume, got {tuple(volume.shape)}")
    lib = load()
    vol = volume.contiguous()
    X, Y, Z = vol.shape
    with torch.cuda.device(dev):
        stream = stream_of(dev)
        nbytes = lib.enarf_mesh_workspace_bytes(X, Y, Z)
        if nbytes == 0:       # sizes the library rejects: let it say why
            check(lib.enarf_mesh_count(vol.data_ptr(), X, Y, Z, float(iso), None, None, stream), "enarf_mesh_count")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        check(lib.enarf_mesh_count(vol.data_ptr(), X, Y, Z, float(iso), ws.data_ptr(), totals.data_ptr(), stream),
              "enarf_mesh_count")
        V, T = (int(x) for x in totals.cpu())         # the one device -> host synchronisation
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        tris = torch.empty(T, 3, dtype=torch.int64, device=dev)
        if V:                                         # an empty surface launches no emit pass
            check(lib.enarf_mesh_emit(vol.data_ptr(), X, Y, Z, float(iso), ws.data_ptr(), verts.data_ptr(),
                                      tris.data_ptr(), stream), "enarf_mesh_emit")
    return verts, tris
