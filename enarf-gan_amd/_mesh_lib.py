"""ctypes binding of libenarf_mesh.so (the C ABI declared in include/enarf_mesh.h): marching cubes on the device.

Like `_lib` there is no CPU fallback: a missing library, a CPU tensor or a failed call raises EnarfHipError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import EnarfHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libenarf_mesh.so")
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

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libenarf_mesh.so (once). Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (torch's HIP runtime first, as in _lib.load)
    if not os.path.exists(LIB_PATH):
        raise EnarfHipError(f"{LIB_PATH} is missing: build it with `python -m enarf_gan_amd.build` (hipcc, gfx950). "
                            "Marching cubes has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.enarf_mesh_abi_version() != ABI_VERSION:
        raise EnarfHipError(f"libenarf_mesh.so ABI {lib.enarf_mesh_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().enarf_mesh_last_error().decode(errors="replace")
        if rc == -2:
            raise NotImplementedError(f"{what}: {msg}")
        raise EnarfHipError(f"{what} failed (code {rc}): {msg}")


def marching_cubes(volume, iso: float):
    """(vertices (V, 3) fp32, triangles (T, 3) int64) on volume's device; the contract is in include/enarf_mesh.h."""
    import torch
    if not isinstance(volume, torch.Tensor) or volume.device.type != "cuda":
        raise EnarfHipError("marching_cubes takes a device tensor (there is no CPU fallback)")
    if volume.dim() != 3 or volume.dtype != torch.float32:
        raise EnarfHipError(f"marching_cubes takes an fp32 (X, Y, Z) volume, got {tuple(volume.shape)} {volume.dtype}")
    lib = load()
    vol = volume.contiguous()
    X, Y, Z = vol.shape
    dev = vol.device
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
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
