"""What the ctypes bindings of the HIP libraries share (`_lib` and the `_<stem>_lib` modules, one per row of
build.ALL_LIBRARIES): loading a library and checking its ABI, turning a return code into an exception, the checks every
op makes on its device arguments, and the shape and dtype checks the mesh-shading bindings (`_paint_lib`, `_bake_lib`,
`_nmap_lib`, and `rgb` for `_geom_lib` and `_nrm_lib`) make before they touch a device: those raise ValueError.

There is no CPU fallback anywhere: a missing library, a CPU tensor or a failed call raises EnarfHipError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_NAMES = {"torch.float32": "fp32", "torch.float64": "fp64", "torch.int64": "int64", "torch.int32": "int32"}


class EnarfHipError(RuntimeError):
    pass


class Library:
    """libenarf_<stem>.so next to the sources: `signatures` is name -> (restype, argtypes) of every symbol the public
    header declares, `no_fallback` the sentence that ends the message when the library has not been built."""

    def __init__(self, stem: str, abi_version: int, signatures: dict, no_fallback: str):
        self.path = os.path.join(_CSRC, f"libenarf_{stem}.so")
        self.name = f"libenarf_{stem}.so"
        self.prefix = "enarf_" if stem == "hip" else f"enarf_{stem}_"
        self.abi_version, self.signatures, self.no_fallback = abi_version, signatures, no_fallback
        self.lib: Optional[C.CDLL] = None

    def load(self) -> C.CDLL:
        """Load the library (once). Raises if it has not been built: there is no fallback path."""
        if self.lib is not None:
            return self.lib
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so). It must be in the process BEFORE this
        # library is dlopen'ed so that both resolve to ONE runtime; loaded the other way round, this library binds
        # /opt/rocm's copy and its launches fail with "no ROCm-capable device is detected" next to torch's.
        import torch  # noqa: F401
        if not os.path.exists(self.path):
            raise EnarfHipError(f"{self.path} is missing: build it with `python -m enarf_gan_amd.build` (hipcc, gfx950). "
                                f"{self.no_fallback}")
        lib = C.CDLL(self.path)
        for name, (res, args) in self.signatures.items():
            fn = getattr(lib, name)      # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        abi = getattr(lib, self.prefix + "abi_version")()
        if abi != self.abi_version:
            raise EnarfHipError(f"{self.name} ABI {abi} != {self.abi_version}")
        self.lib = lib
        return lib

    def check(self, rc: int, what: str) -> None:
        """A call's own return code: -2 is NotImplementedError, any other failure EnarfHipError, with the library's text"""
        if rc != 0:
            msg = getattr(self.load(), self.prefix + "last_error")().decode(errors="replace")
            if rc == -2:
                raise NotImplementedError(f"{what}: {msg}")
            raise EnarfHipError(f"{what} failed (code {rc}): {msg}")


def device_of(who: str, dtypes, **tensors):
    """The one device the named tensors are on (a None is skipped), or EnarfHipError: each must be a device tensor of one
    of `dtypes`."""
    import torch
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise EnarfHipError(f"{who} takes device tensors (there is no CPU fallback); {name} is not one")
        if t.dtype not in dtypes:
            raise EnarfHipError(f"{who} takes {' or '.join(_NAMES[str(d)] for d in dtypes)} {name}, got {t.dtype}")
        if dev is not None and t.device != dev:
            raise EnarfHipError(f"{who}: {name} is on {t.device}, other arguments on {dev}")
        dev = t.device
    return dev


def stream_of(dev) -> C.c_void_p:
    """torch's current HIP stream on `dev`, as the C ABI takes it"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def rgb(value, who: str, name: str) -> Tuple[float, float, float]:
    """a number or three numbers -> three floats, or ValueError"""
    try:
        v = [float(value)] * 3 if not hasattr(value, "__len__") else [float(x) for x in value]
    except (TypeError, ValueError):
        raise ValueError(f"{who} takes a number or three numbers as {name}, got {value!r}") from None
    if len(v) != 3:
        raise ValueError(f"{who} takes a number or three numbers as {name}, got {len(v)} values")
    return v[0], v[1], v[2]


def check_tensors(who: str, want: dict, **named) -> None:
    """each named argument is a tensor of the dtype `want` gives it (fp32 where it gives none), or ValueError"""
    import torch
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who} takes tensors; {name} is {type(t).__name__}")
        if t.dtype != want.get(name, torch.float32):
            raise ValueError(f"{who} takes {want.get(name, torch.float32)} {name}, got {t.dtype}")


def on_device(who: str, **named):
    """the one device of the tensors (a None is skipped), or ValueError; `device_of` is the EnarfHipError form"""
    dev = None
    for name, t in named.items():
        if t is None:
            continue
        if t.device.type != "cuda":
            raise ValueError(f"{who} takes device tensors (there is no CPU fallback); {name} is on {t.device}")
        if dev is not None and t.device != dev:
            raise ValueError(f"{who}: {name} is on {t.device}, other arguments on {dev}")
        dev = t.device
    return dev


def mesh_shapes(who: str, vertices, triangles) -> Tuple[int, int]:
    """(V, T) of (V, 3) vertices and (T, 3) triangles, or ValueError"""
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{who} takes (V, 3) vertices, got {tuple(vertices.shape)}")
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{who} takes (T, 3) triangles, got {tuple(triangles.shape)}")
    V, T = vertices.shape[0], triangles.shape[0]
    if V >= 2 ** 31 or T >= 2 ** 31:
        raise ValueError(f"{who}: V = {V}, T = {T}: both must lie in [0, 2^31)")
    return V, T


def fragment_size(who: str, max_size: int, pix_to_face, bary, normals) -> int:
    """R of the fragment buffers rasterize_mesh returns - (R, R) pix_to_face, (R, R, 3) bary and normals - or ValueError"""
    shape = tuple(pix_to_face.shape)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError(f"{who} takes (R, R) pix_to_face, got {shape}")
    R = shape[0]
    if not 1 <= R <= max_size:
        raise ValueError(f"{who}: render size {R} outside [1, {max_size}]")
    for name, t in (("bary", bary), ("normals", normals)):
        if tuple(t.shape) != (R, R, 3):
            raise ValueError(f"{who} takes ({R}, {R}, 3) {name}, got {tuple(t.shape)}")
    return R


def texture_kind(who: str, name: str, texture) -> Tuple[int, bool]:
    """(A, the texture is fp32) of a uint8 (A, A, 4) or an fp32 (A, A, 3) texture, or ValueError"""
    import torch
    if not isinstance(texture, torch.Tensor):
        raise ValueError(f"{who} takes tensors; {name} is {type(texture).__name__}")
    if texture.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{who} takes a uint8 (A, A, 4) or an fp32 (A, A, 3) {name}, got {texture.dtype}")
    is_f32 = texture.dtype == torch.float32
    ts = tuple(texture.shape)
    if len(ts) != 3 or ts[0] != ts[1] or ts[2] != (3 if is_f32 else 4):
        raise ValueError(f"{who} takes a uint8 (A, A, 4) or an fp32 (A, A, 3) {name}, got {texture.dtype} {ts}")
    return ts[0], is_f32
