"""ctypes binding of libenarf_photo.so (the C ABI declared in include/enarf_photo.h): the photometric loss of the
single-scene path (forward and backward) and the per-image validation metrics (SSIM, MSE, PSNR) on the device.

Loading, return codes and the device-argument checks are `_loader`'s. Shapes, loss types and rectangles are checked
before anything touches the device (ValueError), so those checks run without one.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

from ._loader import EnarfHipError, Library, device_of, stream_of

ABI_VERSION = 1

LOSS_TYPES = {"mse": 0, "mae": 1}
MAE_THRESHOLD = 0.01
LOSS_PARTIALS = 2 * 1024           # ENARF_PHOTO_LOSS_PARTIALS
WINDOW, TILE, MAX_SIDE = 7, 16, 16384

_p = C.c_void_p
_i64 = C.c_int64

# every symbol include/enarf_photo.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_photo_abi_version": (C.c_int, []),
    "enarf_photo_last_error": (C.c_char_p, []),
    "enarf_photo_loss_fwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, C.c_int, C.c_double, C.c_double, _p, _p, _p]),
    "enarf_photo_loss_bwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, C.c_int, C.c_double, C.c_double, _p, _p,
                                       _p, _p, _p]),
    "enarf_photo_metrics": (C.c_int, [_p, _p, _p, _p, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_int), _p, _i64, _p, _p]),
}

_library = Library("photo", ABI_VERSION, SIGNATURES, "The photometric loss and the image metrics have no CPU fallback.")
load, check = _library.load, _library.check


def metric_partials(h: int, w: int) -> int:
    """ENARF_PHOTO_METRIC_PARTIALS(h, w): doubles of scratch one image's rectangle needs"""
    return 3 * ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)


def check_loss_shapes(grid, sparse_color, sparse_mask, color, mask, loss_type: str) -> Tuple[int, int, int]:
    """(B, npix, N) of a loss call, or ValueError; needs no device. `grid` None stands for targets that are already
    gathered (color (B, 3, N), mask (B, N))."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"nerf_loss_type must be one of {sorted(LOSS_TYPES)}, got {loss_type!r}")
    if sparse_color.dim() != 3 or sparse_color.shape[1] != 3:
        raise ValueError(f"sparse_color must be (B, 3, N), got {tuple(sparse_color.shape)}")
    B, _, N = sparse_color.shape
    if tuple(sparse_mask.shape) != (B, N):
        raise ValueError(f"sparse_mask must be ({B}, {N}), got {tuple(sparse_mask.shape)}")
    if grid is None:
        if tuple(color.shape) != (B, 3, N):
            raise ValueError(f"gathered color must be ({B}, 3, {N}), got {tuple(color.shape)}")
        npix = N
    else:
        if color.dim() != 4 or color.shape[0] != B or color.shape[1] != 3 or color.shape[2] != color.shape[3]:
            raise ValueError(f"color must be ({B}, 3, S, S), got {tuple(color.shape)}")
        npix = color.shape[2] * color.shape[3]
        if tuple(grid.shape) != (B, N):
            raise ValueError(f"grid must be ({B}, {N}), got {tuple(grid.shape)}")
    want = (B, N) if grid is None else (B,) + tuple(color.shape[2:])
    if mask is not None and tuple(mask.shape) != want:
        raise ValueError(f"mask must be {want}, got {tuple(mask.shape)}")
    return B, npix, N


def _loss_args(grid, sparse_color, sparse_mask, color, mask, loss_type, who, check_ids):
    import torch
    B, npix, N = check_loss_shapes(grid, sparse_color, sparse_mask, color, mask, loss_type)
    dev = device_of(who, (torch.float32,), sparse_color=sparse_color, sparse_mask=sparse_mask, color=color, mask=mask)
    if grid is not None:
        if not isinstance(grid, torch.Tensor) or grid.device != dev or grid.dtype != torch.int64:
            raise EnarfHipError(f"{who} takes an int64 grid on {dev}")
        if check_ids and grid.numel() and not (0 <= int(grid.min()) and int(grid.max()) < npix):   # synchronises
            raise ValueError(f"{who}: grid ids outside [0, {npix})")
        grid = grid.contiguous()
    return (B, npix, N, dev, grid, sparse_color.contiguous(), sparse_mask.contiguous(), color.contiguous(),
            None if mask is None else mask.contiguous())


def loss_fwd(grid, sparse_color, sparse_mask, color, mask, loss_type: str, color_coef: float, mask_coef: float,
             check_ids: bool = False):
    """(2,) fp32 device tensor [loss_color, loss_mask] (loss_mask is 0 without a mask), on sparse_color's device and its
    current stream, no host synchronisation. The ids of `grid` must lie in [0, S * S), as torch.gather requires: the
    kernel clamps nothing; `check_ids=True` checks them on the host first (a debugging aid: it synchronises)."""
    import torch
    B, npix, N, dev, grid, sc, sm, color, mask = _loss_args(grid, sparse_color, sparse_mask, color, mask, loss_type,
                                                            "photometric_loss", check_ids)
    lib = load()
    with torch.cuda.device(dev):
        partials = torch.empty(LOSS_PARTIALS, dtype=torch.float64, device=dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        stream = stream_of(dev)
        check(lib.enarf_photo_loss_fwd(color.data_ptr(), None if mask is None else mask.data_ptr(),
                                       None if grid is None else grid.data_ptr(), sc.data_ptr(), sm.data_ptr(), B, npix,
                                       N, LOSS_TYPES[loss_type], float(color_coef), float(mask_coef),
                                       partials.data_ptr(), loss.data_ptr(), stream), "enarf_photo_loss_fwd")
    return loss


def loss_bwd(grid, sparse_color, sparse_mask, color, mask, loss_type: str, color_coef: float, mask_coef: float,
             g_color, g_mask):
    """(d sparse_color, d sparse_mask or None without a mask) from the upstream gradients of the two losses: 0-dim
    fp32 device tensors (None is a zero gradient), read on the device."""
    import torch
    B, npix, N, dev, grid, sc, sm, color, mask = _loss_args(grid, sparse_color, sparse_mask, color, mask, loss_type,
                                                            "photometric_loss backward", False)
    device_of("photometric_loss backward", (torch.float32,), g_color=g_color, g_mask=g_mask, sparse_color=sc)
    lib = load()
    with torch.cuda.device(dev):
        d_color = torch.empty_like(sc)
        d_mask = None if mask is None else torch.empty_like(sm)
        stream = stream_of(dev)
        check(lib.enarf_photo_loss_bwd(color.data_ptr(), None if mask is None else mask.data_ptr(),
                                       None if grid is None else grid.data_ptr(), sc.data_ptr(), sm.data_ptr(), B, npix,
                                       N, LOSS_TYPES[loss_type], float(color_coef), float(mask_coef),
                                       None if g_color is None else g_color.data_ptr(),
                                       None if g_mask is None else g_mask.data_ptr(), d_color.data_ptr(),
                                       None if d_mask is None else d_mask.data_ptr(), stream), "enarf_photo_loss_bwd")
    return d_color, d_mask


def check_metric_shapes(img, gen, mask, gen_mask, bbox) -> Tuple[int, int, int, int, int, bool, Optional[list]]:
    """(B, H, W, gen_h, gen_w, gen_cropped, boxes) of a metrics call, or ValueError; needs no device. `bbox` is None
    (the whole frame), one (x0, y0, x1, y1) for every image or a sequence of B of them, of host integers."""
    if img.dim() != 4 or img.shape[1] != 3 or gen.dim() != 4 or gen.shape[:2] != img.shape[:2]:
        raise ValueError(f"img and gen must be (B, 3, H, W) with one B, got {tuple(img.shape)} and {tuple(gen.shape)}")
    B, _, H, W = img.shape
    gh, gw = gen.shape[2:]
    if (mask is None) != (gen_mask is None):
        raise ValueError("mask and gen_mask come together or not at all")
    if mask is not None and (tuple(mask.shape) != (B, H, W) or tuple(gen_mask.shape) != (B, gh, gw)):
        raise ValueError(f"mask must be ({B}, {H}, {W}) and gen_mask ({B}, {gh}, {gw}), got {tuple(mask.shape)} and "
                         f"{tuple(gen_mask.shape)}")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"frame {H} x {W} outside [1, {MAX_SIDE}]")
    boxes = None
    if bbox is not None:
        rows = [bbox] * B if len(bbox) == 4 and not hasattr(bbox[0], "__len__") else list(bbox)
        if len(rows) != B or any(len(r) != 4 for r in rows):
            raise ValueError(f"bbox must be (x0, y0, x1, y1) or {B} of them")
        boxes = [[int(v) for v in r] for r in rows]
    cropped = (gh, gw) != (H, W)
    for x0, y0, x1, y1 in (boxes if boxes is not None else [[0, 0, W, H]]):
        if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
            raise ValueError(f"rectangle ({x0}, {y0}, {x1}, {y1}) outside the {H} x {W} frame")
        if x1 - x0 < WINDOW or y1 - y0 < WINDOW:
            raise ValueError(f"rectangle {y1 - y0} x {x1 - x0} has a side shorter than the {WINDOW} x {WINDOW} window "
                             "(win_size exceeds image extent)")
        if cropped and (gh, gw) != (y1 - y0, x1 - x0):
            raise ValueError(f"gen is {gh} x {gw}: neither the {H} x {W} frame nor its {y1 - y0} x {x1 - x0} rectangle")
    return B, H, W, gh, gw, cropped, boxes


def metrics(img, gen, mask=None, gen_mask=None, bbox: Optional[Sequence] = None):
    """(B, 4) fp32 device tensor [ssim, mse_color, psnr, mse_mask] per image (include/enarf_photo.h), on img's device
    and its current stream, no host synchronisation and no cropped copy. `gen` / `gen_mask` are frames like img / mask
    or already cropped to the rectangle (what render_entire_img(bbox=...) returns)."""
    import torch
    B, H, W, gh, gw, cropped, boxes = check_metric_shapes(img, gen, mask, gen_mask, bbox)
    dev = device_of("image_metrics", (torch.float32,), img=img, gen=gen, mask=mask, gen_mask=gen_mask)
    lib = load()
    sizes = [(y1 - y0, x1 - x0) for x0, y0, x1, y1 in boxes] if boxes is not None else [(H, W)]
    n_partials = B * max(metric_partials(h, w) for h, w in sizes)
    box_arr = None if boxes is None else (C.c_int * (4 * B))(*[v for r in boxes for v in r])
    with torch.cuda.device(dev):
        img, gen = img.contiguous(), gen.contiguous()
        mask, gen_mask = (None, None) if mask is None else (mask.contiguous(), gen_mask.contiguous())
        partials = torch.empty(max(n_partials, 1), dtype=torch.float64, device=dev)
        out = torch.empty(B, 4, dtype=torch.float32, device=dev)
        stream = stream_of(dev)
        check(lib.enarf_photo_metrics(img.data_ptr(), gen.data_ptr(), None if mask is None else mask.data_ptr(),
                                      None if gen_mask is None else gen_mask.data_ptr(), B, H, W, gh, gw, int(cropped),
                                      box_arr, partials.data_ptr(), n_partials, out.data_ptr(), stream),
              "enarf_photo_metrics")
    return out
