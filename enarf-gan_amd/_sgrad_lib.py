"""ctypes binding of libenarf_sgrad.so (the C ABI declared in include/enarf_sgrad.h): the gradient of the multi-avatar
composite (libenarf_scene.so) with respect to the K avatars' densities and colours, on the device, and the
torch.autograd.Function that joins the two libraries into a differentiable composite.

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
UPSTREAM = ("g_color", "g_mask", "g_disparity", "g_instance_mass")
OUTPUTS = ("density", "color")

_p = C.c_void_p


class CompositeBwdArgs(C.Structure):
    _fields_ = [("F", C.c_int32), ("K", C.c_int32), ("n", C.c_int32), ("Nf", C.c_int32), ("render_scale", C.c_float),
                ("depth", _p), ("density", _p), ("color", _p), ("valid", _p),
                ("g_color", _p), ("g_mask", _p), ("g_disparity", _p), ("g_instance_mass", _p),
                ("g_density", _p), ("g_sample_color", _p)]


# every symbol include/enarf_sgrad.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_sgrad_abi_version": (C.c_int, []),
    "enarf_sgrad_last_error": (C.c_char_p, []),
    "enarf_sgrad_composite_bwd": (C.c_int, [C.POINTER(CompositeBwdArgs), _p]),
}

SceneGradients = namedtuple("SceneGradients", OUTPUTS)

_library = Library("sgrad", ABI_VERSION, SIGNATURES, "The scene composite's backward kernel has no CPU fallback.")
load, check = _library.load, _library.check


def check_composite_bwd_args(depth, density, color, valid, g_color, g_mask, g_disparity, g_instance_mass,
                             want) -> Tuple[int, int, int, int, bool]:
    """(F, K, n, Nf, framed) of a scene_composite_bwd call; ValueError for shapes, dtypes, `want` and a call without any
    upstream gradient, NotImplementedError for the limits. Touches no device and no library."""
    import torch
    who = "scene_composite_bwd"
    for name, t in dict(depth=depth, density=density, color=color).items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who} takes tensors; {name} is {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{who} takes torch.float32 {name}, got {t.dtype}")
    shape = tuple(depth.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"{who} takes depth (F, K, n, Nf), or (K, n, Nf) for one frame; got {shape}")
    framed = len(shape) == 4
    F, K, n, Nf = shape if framed else (1,) + shape
    lead = (F,) if framed else ()
    if tuple(density.shape) != shape:
        raise ValueError(f"{who} takes a density of depth's shape {shape}, got {tuple(density.shape)}")
    if tuple(color.shape) != lead + (K, 3, n, Nf):
        raise ValueError(f"{who} takes color {lead + (K, 3, n, Nf)} with depth {shape}, got {tuple(color.shape)}")
    if valid is not None:
        if not isinstance(valid, torch.Tensor):
            raise ValueError(f"{who} takes a tensor or None as valid, got {type(valid).__name__}")
        if valid.dtype != torch.uint8:
            raise ValueError(f"{who} takes torch.uint8 valid, got {valid.dtype}")
        if tuple(valid.shape) != lead + (K, n):
            raise ValueError(f"{who} takes valid {lead + (K, n)} with depth {shape}, got {tuple(valid.shape)}")
    upstream = dict(g_color=(g_color, lead + (3, n)), g_mask=(g_mask, lead + (n,)), g_disparity=(g_disparity, lead + (n,)),
                    g_instance_mass=(g_instance_mass, lead + (K, n)))
    if all(t is None for t, _ in upstream.values()):
        raise ValueError(f"{who}: no upstream gradient given; at least one of {UPSTREAM} is required")
    for name, (t, want_shape) in upstream.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who} takes a tensor or None as {name}, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{who} takes torch.float32 {name}, got {t.dtype}")
        if tuple(t.shape) != want_shape:
            raise ValueError(f"{who} takes {name} {want_shape} with depth {shape}, got {tuple(t.shape)}")
    try:
        want = tuple(want)
    except TypeError:
        raise ValueError(f"{who}: want {want!r} is not a sequence of names") from None
    if not want or any(w not in OUTPUTS for w in want):
        raise ValueError(f"{who}: want {want!r} must name at least one of {OUTPUTS} and nothing else")
    if F * n >= MAX_RAYS:
        raise ValueError(f"{who}: {F} frames of {n} rays: F n must stay below 2^31")
    if not 1 <= K <= MAX_AVATARS:
        raise NotImplementedError(f"{who}: {K} avatars outside [1, {MAX_AVATARS}]")
    if not 2 <= Nf <= MAX_SAMPLES:
        raise NotImplementedError(f"{who}: {Nf} samples a ray outside [2, {MAX_SAMPLES}]")
    if K * Nf > MAX_MERGED:
        raise NotImplementedError(f"{who}: {K} avatars of {Nf} samples are {K * Nf} breakpoints a ray, more than {MAX_MERGED}")
    return F, K, n, Nf, framed


def _number(value, name: str) -> float:
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"scene_composite_bwd takes a number as {name}, got {value!r}") from None


def scene_composite_bwd(depth, density, color, valid=None, render_scale=1.0, g_color=None, g_mask=None, g_disparity=None,
                        g_instance_mass=None, want=OUTPUTS, out=None) -> SceneGradients:
    """SceneGradients(density, color) on the inputs' device and its current stream, one launch, no synchronisation; a
    field not in `want` is None. `out` (a dict name -> contiguous tensor) writes into given tensors, every entry of
    which is overwritten. The contract is in include/enarf_sgrad.h."""
    import torch
    who = "scene_composite_bwd"
    F, K, n, Nf, framed = check_composite_bwd_args(depth, density, color, valid, g_color, g_mask, g_disparity,
                                                   g_instance_mass, want)
    want = tuple(want)
    scale = _number(render_scale, "render_scale")
    lead = (F,) if framed else ()
    f32 = torch.float32
    shapes = dict(density=lead + (K, n, Nf), color=lead + (K, 3, n, Nf))
    out = dict(out or {})
    for name, t in out.items():
        if name not in want:
            raise ValueError(f"{who}: out names {name!r}, which is not in want {want}")
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shapes[name] or t.dtype != f32 or not t.is_contiguous():
            raise ValueError(f"{who}: out[{name!r}] must be a contiguous {f32} tensor of shape {shapes[name]}")
    dev = device_of(who, (f32,), depth=depth, density=density, color=color, g_color=g_color, g_mask=g_mask,
                    g_disparity=g_disparity, g_instance_mass=g_instance_mass)
    if valid is not None and device_of(who, (torch.uint8,), valid=valid) != dev:
        raise ValueError(f"{who}: valid is on {valid.device}, the samples on {dev}")
    for name, t in out.items():
        if t.device != dev:
            raise ValueError(f"{who}: out[{name!r}] is on {t.device}, the inputs on {dev}")
    lib = load()
    keep = [None if t is None else t.detach().contiguous()
            for t in (depth, density, color, valid, g_color, g_mask, g_disparity, g_instance_mass)]
    with torch.cuda.device(dev):
        res = {k: out[k] if k in out else torch.empty(shapes[k], dtype=f32, device=dev) for k in want}
        if F * n > 0:
            a = CompositeBwdArgs()
            a.F, a.K, a.n, a.Nf = F, K, n, Nf
            a.render_scale = scale
            a.depth, a.density, a.color = (t.data_ptr() for t in keep[:3])
            for name, t in zip(("valid",) + UPSTREAM, keep[3:]):
                setattr(a, name, None if t is None else t.data_ptr())
            a.g_density = res["density"].data_ptr() if "density" in res else None
            a.g_sample_color = res["color"].data_ptr() if "color" in res else None
            check(lib.enarf_sgrad_composite_bwd(C.byref(a), stream_of(dev)), "enarf_sgrad_composite_bwd")
    del keep
    return SceneGradients(*(res.get(k) for k in OUTPUTS))


_FORWARD = ("color", "mask", "disparity", "instance_mass")


def _composite_function():
    """the autograd.Function, made on first use (this module imports no torch at import time)"""
    global _CompositeFunction
    if _CompositeFunction is not None:
        return _CompositeFunction
    import torch
    from . import _scene_lib

    class SceneCompositeFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, depth, density, color, valid, render_scale):
            res = _scene_lib.scene_composite(depth.detach(), density.detach(), color.detach(), valid, render_scale, 0.5,
                                             _FORWARD, None)
            ctx.save_for_backward(depth, density, color)
            ctx.set_materialize_grads(False)                  # an output the loss does not use arrives as None: zeros
            ctx.valid, ctx.render_scale = valid, render_scale
            return res.color, res.mask, res.disparity, res.instance_mass

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, g_color, g_mask, g_disparity, g_instance_mass):
            depth, density, color = ctx.saved_tensors
            want = tuple(name for name, needed in zip(OUTPUTS, ctx.needs_input_grad[1:3]) if needed)
            if not want:
                return None, None, None, None, None
            got = scene_composite_bwd(depth, density, color, ctx.valid, ctx.render_scale, g_color, g_mask, g_disparity,
                                      g_instance_mass, want, None)
            return None, got.density, got.color, None, None

    _CompositeFunction = SceneCompositeFunction
    return _CompositeFunction


_CompositeFunction = None


def scene_composite_posable(depth, density, color, valid=None, render_scale=1.0):
    """(color, mask, disparity, instance_mass) of scene_composite, differentiable with respect to density and color: the
    forward is scene_composite on the detached inputs, the backward one launch of libenarf_sgrad.so. A depth that
    requires a gradient raises NotImplementedError (depths are constants of the contract)."""
    import torch
    if isinstance(depth, torch.Tensor) and depth.requires_grad:
        raise NotImplementedError("scene_composite_posable carries no gradient to the depths (the sample positions are "
                                  "constants): detach depth")
    return _composite_function().apply(depth, density, color, valid, _number(render_scale, "render_scale"))
