"""ctypes binding of libenarf_geom.so (the C ABI declared in include/enarf_geom.h): depth, point and normal maps and a
shape image from the disparity and mask a march returns, and the running inverse-depth error of an evaluation set, on
the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Tuple

from ._loader import Library, device_of, rgb, stream_of

ABI_VERSION = 1

MAX_SIZE = 4096        # H, W
MAX_COUNT = 2 ** 31    # B H W
STATE_WORDS = 8
MAX_RECORDS = 1024
SHADES = {"normal": 0, "lit": 1, "depth": 2}
OUTPUTS = ("depth", "points", "normals", "flags", "image")

_p = C.c_void_p


class BuffersArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("KB", C.c_int32),
                ("normalise", C.c_int32), ("shade", C.c_int32),
                ("x0", C.c_float), ("y0", C.c_float), ("step", C.c_float),
                ("depth_scale", C.c_float), ("mask_threshold", C.c_float), ("edge", C.c_float),
                ("near_depth", C.c_float), ("far_depth", C.c_float),
                ("background", C.c_float * 3), ("reserved", C.c_int32),
                ("disparity", _p), ("mask", _p), ("inv_intrinsics", _p),
                ("depth", _p), ("points", _p), ("normals", _p), ("flags", _p), ("image", _p)]


# every symbol include/enarf_geom.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_geom_abi_version": (C.c_int, []),
    "enarf_geom_last_error": (C.c_char_p, []),
    "enarf_geom_buffers": (C.c_int, [C.POINTER(BuffersArgs), _p]),
    "enarf_geom_err_records": (C.c_int64, [C.c_int64]),
    "enarf_geom_err_update": (C.c_int, [_p, _p, _p, C.c_int64, C.c_float, _p, C.c_int64, _p, _p]),
}

GeometryBuffers = namedtuple("GeometryBuffers", OUTPUTS)

_library = Library("geom", ABI_VERSION, SIGNATURES, "The geometry kernels have no CPU fallback.")
load, check = _library.load, _library.check


def _number(value, name: str) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"geometry_buffers takes a number as {name}, got {value!r}") from None


def check_buffers_args(disparity, mask, inv_intrinsics, size, origin, step, shade, near, far, want) -> Tuple[int, int, int, int]:
    """(B, H, W, KB) of a geometry_buffers call, or ValueError; shapes, dtypes and values only, touches no device"""
    import torch
    for name, t in dict(disparity=disparity, mask=mask, inv_intrinsics=inv_intrinsics).items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"geometry_buffers takes tensors; {name} is {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"geometry_buffers takes torch.float32 {name}, got {t.dtype}")
    shape = tuple(disparity.shape)
    if size is None:
        if len(shape) != 3:
            raise ValueError(f"geometry_buffers takes (B, H, W) disparity, or (B, n) with size=(H, W); got {shape}")
        B, H, W = shape
    else:
        try:
            H, W = (int(s) for s in size)
        except (TypeError, ValueError):
            raise ValueError(f"geometry_buffers takes size=(H, W), got {size!r}") from None
        if len(shape) < 2 or shape not in ((shape[0], H * W), (shape[0], H, W)):
            raise ValueError(f"geometry_buffers: disparity {shape} is neither (B, {H * W}) nor (B, {H}, {W})")
        B = shape[0]
    if tuple(mask.shape) != shape:
        raise ValueError(f"geometry_buffers takes a mask of disparity's shape {shape}, got {tuple(mask.shape)}")
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f"geometry_buffers: image size {H} x {W} outside [1, {MAX_SIZE}]")
    if B < 1 or B * H * W >= MAX_COUNT:
        raise ValueError(f"geometry_buffers: B = {B} with {H} x {W} pixels: B H W must lie in [1, 2^31)")
    k = tuple(inv_intrinsics.shape)
    if k == (3, 3):
        KB = 1
    elif len(k) == 3 and k[1:] == (3, 3) and k[0] in (1, B):
        KB = k[0]
    else:
        raise ValueError(f"geometry_buffers takes (3, 3), (1, 3, 3) or ({B}, 3, 3) inv_intrinsics, got {k}")
    try:
        ok = len(origin) == 2
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"geometry_buffers takes origin=(x0, y0), got {origin!r}")
    if shade not in SHADES:
        raise ValueError(f"geometry_buffers: shade {shade!r} is none of {tuple(SHADES)}")
    want = tuple(want)
    if not want or any(w not in OUTPUTS for w in want):
        raise ValueError(f"geometry_buffers: want {want!r} must name at least one of {OUTPUTS} and nothing else")
    if shade == "depth" and "image" in want:
        if near is None or far is None:
            raise ValueError("geometry_buffers: shade='depth' takes near and far")
        n, f = _number(near, "near"), _number(far, "far")
        if not (n > 0 and f > 0 and n != f):
            raise ValueError(f"geometry_buffers: shade='depth' takes near > 0, far > 0, near != far, got {n} and {f}")
    return B, H, W, KB


def geometry_buffers(disparity, mask, inv_intrinsics, size=None, origin=(0, 0), step=1.0, depth_scale=1.0,
                     mask_threshold=0.5, edge=0.05, normalise=True, shade="normal", near=None, far=None, background=1.0,
                     want=OUTPUTS, out=None) -> GeometryBuffers:
    """GeometryBuffers(depth, points, normals, flags, image) on the inputs' device and its current stream, one launch, no
    synchronisation; a field not in `want` is None. `out` (a dict name -> contiguous tensor) writes into given tensors.
    The contract is in include/enarf_geom.h."""
    import torch
    B, H, W, KB = check_buffers_args(disparity, mask, inv_intrinsics, size, origin, step, shade, near, far, want)
    want = tuple(want)
    bg = rgb(background, "geometry_buffers", "background")
    scalars = {n: _number(v, n) for n, v in dict(x0=origin[0], y0=origin[1], step=step, depth_scale=depth_scale,
                                                 mask_threshold=mask_threshold, edge=edge).items()}
    shapes = dict(depth=((B, H, W), torch.float32), points=((B, H, W, 3), torch.float32),
                  normals=((B, H, W, 3), torch.float32), flags=((B, H, W), torch.uint8), image=((B, H, W, 3), torch.uint8))
    out = dict(out or {})
    for name, t in out.items():
        if name not in want:
            raise ValueError(f"geometry_buffers: out names {name!r}, which is not in want {want}")
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[name][0] or t.dtype != shapes[name][1] or not t.is_contiguous():
            raise ValueError(f"geometry_buffers: out[{name!r}] must be a contiguous {shapes[name][1]} tensor of shape {shapes[name][0]}")
    dev = device_of("geometry_buffers", (torch.float32,), disparity=disparity, mask=mask, inv_intrinsics=inv_intrinsics)
    for name, t in out.items():
        if t.device != dev:
            raise ValueError(f"geometry_buffers: out[{name!r}] is on {t.device}, the inputs on {dev}")
    lib = load()
    keep = [t.contiguous() for t in (disparity, mask, inv_intrinsics)]
    with torch.cuda.device(dev):
        res = {n: out[n] if n in out else torch.empty(shapes[n][0], dtype=shapes[n][1], device=dev) for n in want}
        a = BuffersArgs()
        a.B, a.H, a.W, a.KB = B, H, W, KB
        a.normalise, a.shade = int(bool(normalise)), SHADES[shade]
        a.x0, a.y0, a.step = scalars["x0"], scalars["y0"], scalars["step"]
        a.depth_scale, a.mask_threshold, a.edge = scalars["depth_scale"], scalars["mask_threshold"], scalars["edge"]
        a.near_depth, a.far_depth = (float(near), float(far)) if shade == "depth" and "image" in want else (0.0, 0.0)
        a.background[:] = bg
        a.disparity, a.mask, a.inv_intrinsics = (t.data_ptr() for t in keep)
        for n in OUTPUTS:
            setattr(a, n, res[n].data_ptr() if n in res else None)
        check(lib.enarf_geom_buffers(C.byref(a), stream_of(dev)), "enarf_geom_buffers")
    del keep
    return GeometryBuffers(*(res.get(n) for n in OUTPUTS))


def err_records(n: int) -> int:
    """workgroups (records of 64 bytes) an update of n pixels uses; plain arithmetic, the library's own rule"""
    return 0 if not 1 <= n < MAX_COUNT else min(MAX_RECORDS, (n + 2047) // 2048)


def check_err_args(disparity, target, mask) -> int:
    """pixels of a DepthError.update call, or ValueError; shapes and dtypes only"""
    import torch
    named = dict(disparity=disparity, target=target)
    if mask is not None:
        named["mask"] = mask
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"DepthError.update takes tensors; {name} is {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"DepthError.update takes torch.float32 {name}, got {t.dtype}")
        if tuple(t.shape) != tuple(disparity.shape):
            raise ValueError(f"DepthError.update: {name} {tuple(t.shape)} differs from disparity {tuple(disparity.shape)}")
    n = disparity.numel()
    if not 1 <= n < MAX_COUNT:
        raise ValueError(f"DepthError.update: {n} pixels outside [1, 2^31)")
    return n


class DepthError:
    """The running inverse-depth error of an evaluation set, kept on the device: update() is two launches with no
    synchronisation, result() the one host read. Sums are fp64 and bit-identical from run to run. The workspace and the
    state are the object's own and every update reads and rewrites them, so one DepthError belongs to one stream: the
    stream of its first update is kept, and an update issued on another raises ValueError (reset() keeps the stream)."""

    def __init__(self, mask_threshold: float = 0.5):
        self.mask_threshold = _number(mask_threshold, "mask_threshold")
        self._state = None
        self._workspace = None
        self._stream = None

    def update(self, disparity, target, mask=None) -> "DepthError":
        import torch
        n = check_err_args(disparity, target, mask)
        dev = device_of("DepthError.update", (torch.float32,), disparity=disparity, target=target, mask=mask)
        if self._state is not None and self._state.device != dev:
            raise ValueError(f"DepthError.update: inputs on {dev}, the running state on {self._state.device}")
        stream = stream_of(dev)
        handle = stream.value or 0                     # the null stream's handle reads back as None
        if self._stream is not None and handle != self._stream:
            raise ValueError("DepthError.update: issued on another stream than the first update; one DepthError belongs to "
                             "one stream")
        lib = load()
        records = err_records(n)
        keep = [None if t is None else t.contiguous() for t in (disparity, mask, target)]
        with torch.cuda.device(dev):
            if self._state is None:
                self._state = torch.zeros(STATE_WORDS, dtype=torch.int64, device=dev)
            if self._workspace is None or self._workspace.shape[0] < records:
                self._workspace = torch.empty((records, STATE_WORDS), dtype=torch.int64, device=dev)
            q, m, g = (None if t is None else t.data_ptr() for t in keep)
            check(lib.enarf_geom_err_update(q, m, g, n, self.mask_threshold, self._workspace.data_ptr(),
                                            self._workspace.shape[0], self._state.data_ptr(), stream),
                  "enarf_geom_err_update")
            self._stream = handle
        del keep
        return self

    def reset(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def state(self):
        """the (8,) int64 device tensor of include/enarf_geom.h (words 1 and 3 hold fp64 bits), or None before an update"""
        return self._state

    def result(self) -> dict:
        """one host read: n, sse_all, n_fg, sse_fg, inter, union, updates, and inv_depth_mse = sse_all / n,
        inv_depth_mse_fg = sse_fg / n_fg, iou = inter / union (NaN where the denominator is 0)"""
        import numpy as np
        if self._state is None:
            words = np.zeros(STATE_WORDS, np.int64)
        else:
            words = self._state.cpu().numpy()
        real = words.view(np.float64)
        r = dict(n=int(words[0]), sse_all=float(real[1]), n_fg=int(words[2]), sse_fg=float(real[3]), inter=int(words[4]),
                 union=int(words[5]), updates=int(words[6]))
        ratio = lambda a, b: a / b if b else float("nan")
        r["inv_depth_mse"] = ratio(r["sse_all"], r["n"])
        r["inv_depth_mse_fg"] = ratio(r["sse_fg"], r["n_fg"])
        r["iou"] = ratio(r["inter"], r["union"])
        return r

