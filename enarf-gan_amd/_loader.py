"""What the ctypes bindings of the HIP libraries share (`_lib` and the `_<stem>_lib` modules, one per row of
build.ALL_LIBRARIES): loading a library and checking its ABI, turning a return code into an exception, and the checks every
op makes on its device arguments.

There is no CPU fallback anywhere: a missing library, a CPU tensor or a failed call raises EnarfHipError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

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
