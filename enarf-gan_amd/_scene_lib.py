"""ctypes binding of libenarf_scene.so (the C ABI declared in include/enarf_scene.h): K avatars marched on the same rays,
composed into one colour, mask and disparity per ray, with the share of the mask each avatar carries and the avatar that
owns each pixel, on the device.

Loading, return codes and the device-argument checks are `_loader`'s.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Tuple

from ._loader import Library, device_of, stream_of

ABI_VERSION = 1

MAX_AVATARS = 8        # K
MAX_SAMPLES = 128      # Nf
MAX_MERGED = 512       # K Nf
MAX_RAYS = 2 ** 31     # F n
OUTPUTS = ("color", "mask", "disparity", "instance_mass", "instance", "skipped", "t", "source", "weight")
DEFAULT_WANT = ("color", "mask", "disparity", "instance_mass", "instance", "skipped")

_p = C.c_void_p


class CompositeArgs(C.Structure):
    _fields_ = [("F", C.c_int32), ("K", C.c_int32), ("n", C.c_int32), ("Nf", C.c_int32),
                ("render_scale", C.c_float), ("threshold", C.c_float),
                ("depth", _p), ("density", _p), ("color", _p), ("valid", _p),
                ("out_color", _p), ("out_mask", _p), ("out_disparity", _p), ("out_instance_mass", _p),
                ("out_instance", _p), ("out_skipped", _p), ("out_t", _p), ("out_source", _p), ("out_weight", _p)]


# every symbol include/enarf_scene.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_scene_abi_version": (C.c_int, []),
    "enarf_scene_last_error": (C.c_char_p, []),
    "enarf_scene_composite": (C.c_int, [C.POINTER(CompositeArgs), _p]),
}

SceneComposite = namedtuple("SceneComposite", OUTPUTS)

_library = Library("scene", ABI_VERSION, SIGNATURES, "The scene compositing kernel has no CPU fallback.")
load, check = _library.load, _library.check


def _number(value, name: str) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"scene_composite takes a number as {name}, got {value!r}") from None


def check_composite_args(depth, density, color, valid, want) -> Tuple[int, int, int, int, bool]:
    """(F, K, n, Nf, framed) of a scene_composite call; ValueError for shapes, dtypes and `want`, NotImplementedError for
    the limits and for inputs that require a gradient. Touches no device and no library."""
    import torch
    for name, t in dict(depth=depth, density=density, color=color).items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"scene_composite takes tensors; {name} is {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"scene_composite takes torch.float32 {name}, got {t.dtype}")
    shape = tuple(depth.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"scene_composite takes depth (F, K, n, Nf), or (K, n, Nf) for one frame; got {shape}")
    framed = len(shape) == 4
    F, K, n, Nf = shape if framed else (1,) + shape
    lead = (F,) if framed else ()
    if tuple(density.shape) != shape:
        raise ValueError(f"scene_composite takes a density of depth's shape {shape}, got {tuple(density.shape)}")
    if tuple(color.shape) != lead + (K, 3, n, Nf):
        raise ValueError(f"scene_composite takes color {lead + (K, 3, n, Nf)} with depth {shape}, got {tuple(color.shape)}")
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise ValueError(f"scene_composite takes a tensor or None as valid, got {type(valid).__name__}")
        if valid.dtype != torch.uint8:
            raise ValueError(f"scene_composite takes torch.uint8 valid, got {valid.dtype}")
        if tuple(valid.shape) != lead + (K, n):
            raise ValueError(f"scene_composite takes valid {lead + (K, n)} with depth {shape}, got {tuple(valid.shape)}")
    try:
        want = tuple(want)
    except TypeError:
        raise ValueError(f"scene_composite: want {want!r} is not a sequence of names") from None
    if not want or any(w not in OUTPUTS for w in want):
        raise ValueError(f"scene_composite: want {want!r} must name at least one of {OUTPUTS} and nothing else")
    if F * n >= MAX_RAYS:
        raise ValueError(f"scene_composite: {F} frames of {n} rays: F n must stay below 2^31")
    if not 1 <= K <= MAX_AVATARS:
        raise NotImplementedError(f"scene_composite: {K} avatars outside [1, {MAX_AVATARS}]")
    if not 2 <= Nf <= MAX_SAMPLES:
        raise NotImplementedError(f"scene_composite: {Nf} samples a ray outside [2, {MAX_SAMPLES}]")
    if K * Nf > MAX_MERGED:
        raise NotImplementedError(f"scene_composite: {K} avatars of {Nf} samples are {K * Nf} breakpoints a ray, more than "
                                  f"{MAX_MERGED}")
    if any(t.requires_grad for t in (depth, density, color)):
        raise NotImplementedError("scene_composite carries no gradient (the taps it reads are not differentiable): detach "
                                  "the inputs or call it under torch.no_grad() on tensors that do not require one")
    return F, K, n, Nf, framed


def scene_composite(depth, density, color, valid=None, render_scale=1.0, threshold=0.5, want=DEFAULT_WANT,
                    out=None) -> SceneComposite:
    """SceneComposite(color, mask, disparity, instance_mass, instance, skipped, t, source, weight) on the inputs' device
    and its current stream, one launch, no synchronisation; a field not in `want` is None. `out` (a dict name ->
    contiguous tensor) writes into given tensors. The contract is in include/enarf_scene.h."""
    import torch
    F, K, n, Nf, framed = check_composite_args(depth, density, color, valid, want)
    want = tuple(want)
    scale, level = _number(render_scale, "render_scale"), _number(threshold, "threshold")
    lead = (F,) if framed else ()
    f32, i32 = torch.float32, torch.int32
    shapes = dict(color=(lead + (3, n), f32), mask=(lead + (n,), f32), disparity=(lead + (n,), f32),
                  instance_mass=(lead + (K, n), f32), instance=(lead + (n,), i32), skipped=(lead + (n,), i32),
                  t=(lead + (n, K * Nf), f32), source=(lead + (n, K * Nf), i32), weight=(lead + (n, K * Nf), f32))
    out = dict(out or {})
    for name, t in out.items():
        if name not in want:
            raise ValueError(f"scene_composite: out names {name!r}, which is not in want {want}")
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[name][0] or t.dtype != shapes[name][1] or not t.is_contiguous():
            raise ValueError(f"scene_composite: out[{name!r}] must be a contiguous {shapes[name][1]} tensor of shape {shapes[name][0]}")
    dev = device_of("scene_composite", (f32,), depth=depth, density=density, color=color)
    if valid is not None and device_of("scene_composite", (torch.uint8,), valid=valid) != dev:
        raise ValueError(f"scene_composite: valid is on {valid.device}, the samples on {dev}")
    for name, t in out.items():
        if t.device != dev:
            raise ValueError(f"scene_composite: out[{name!r}] is on {t.device}, the inputs on {dev}")
    lib = load()
    keep = [None if t is None else t.contiguous() for t in (depth, density, color, valid)]
    with torch.cuda.device(dev):
        res = {k: out[k] if k in out else torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
        if F * n > 0:
            a = CompositeArgs()
            a.F, a.K, a.n, a.Nf = F, K, n, Nf
            a.render_scale, a.threshold = scale, level
            a.depth, a.density, a.color = (t.data_ptr() for t in keep[:3])
            a.valid = None if keep[3] is None else keep[3].data_ptr()
            for k in OUTPUTS:
                setattr(a, "out_" + k, res[k].data_ptr() if k in res else None)
            check(lib.enarf_scene_composite(C.byref(a), stream_of(dev)), "enarf_scene_composite")
    del keep
    return SceneComposite(*(res.get(k) for k in OUTPUTS))
