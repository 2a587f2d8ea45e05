"""Tensor-level wrappers of the C ABI: torch supplies device memory and the current HIP stream,
nothing else. Every function here requires CUDA(=HIP) tensors and raises otherwise.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import FEAT_DIM, MARCH, MLP_MODE, ORIGIN

PLANE_CH = 3 * FEAT_DIM   # 96 feature channels precede the part-probability planes (models/narf.py:239,255)


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _first_cuda_tensor(args, kwargs) -> Optional[torch.Tensor]:
    for v in list(args) + list(kwargs.values()):
        if isinstance(v, torch.Tensor) and v.is_cuda:
            return v
        if isinstance(v, dict):
            for w in v.values():
                if isinstance(w, torch.Tensor) and w.is_cuda:
                    return w
    return None


def _on_tensor_device(fn):
    """The library launches on the stream it is handed, and a HIP stream belongs to one device: make the device of the
    call's first device tensor current for the duration of the call (a process that drives several GPUs may have another
    one current)."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        t = _first_cuda_tensor(args, kwargs)
        if t is None or t.device.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(t.device):
            return fn(*args, **kwargs)
    return wrapped


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _dev_f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.EnarfHipError(f"{what} must be a CUDA/HIP tensor (enarf_gan_amd has no CPU path)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def mlp_pack_bytes() -> int:
    return int(_lib.load().enarf_mlp_pack_bytes())


def num_parts(num_joints: int, origin_location: str) -> int:
    return num_joints if origin_location == "center+head" else num_joints - 1


# ---------------------------------------------------------------------------------------- a1 operator
@_on_tensor_device
def triplane_sample_fwd(inp: torch.Tensor, grid: torch.Tensor, mode: int = 0, padding_mode: int = 0,
                        align_corners: bool = False, use_workspace: bool = True) -> torch.Tensor:
    """input (B,3C,H,W), grid (B,h,w,3) -> (B,C,h,w); cuda_extension/TriplaneSampler.cpp:15-24."""
    lib = _lib.load()
    inp = _dev_f32(inp, "input")
    grid = _dev_f32(grid, "grid")
    B, C3, H, W = inp.shape
    if C3 % 3 != 0 or grid.shape[0] != B or grid.shape[-1] != 3 or grid.dim() != 4:
        raise ValueError(f"triplane_sampler: input {tuple(inp.shape)} / grid {tuple(grid.shape)} shapes do not match "
                         "(B,3C,H,W) / (B,h,w,3)")
    h, w = grid.shape[1], grid.shape[2]
    Cc = C3 // 3
    out = torch.empty(B, Cc, h, w, dtype=torch.float32, device=inp.device)
    ws = None
    if use_workspace:
        nbytes = lib.enarf_triplane_sample_workspace_bytes(B, Cc, H, W)
        if nbytes:
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=inp.device)
    rc = lib.enarf_triplane_sample_fwd(_p(inp), _p(grid), _p(out), B, Cc, H, W, h * w, mode, padding_mode,
                                       int(bool(align_corners)), _p(ws), _stream(inp.device))
    _lib.check(rc, "enarf_triplane_sample_fwd")
    return out


@_on_tensor_device
def triplane_sample_bwd(grad_out: torch.Tensor, inp: torch.Tensor, grid: torch.Tensor, mode: int, padding_mode: int,
                        align_corners: bool, need_input: bool, need_grid: bool, use_workspace: bool = True
                        ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """cuda_extension/TriplaneSampler.cpp:26-52; returns (grad_input, grad_grid), None where not needed."""
    lib = _lib.load()
    grad_out = _dev_f32(grad_out, "grad_output")
    inp = _dev_f32(inp, "input")
    grid = _dev_f32(grid, "grid")
    B, C3, H, W = inp.shape
    h, w = grid.shape[1], grid.shape[2]
    gi = torch.zeros_like(inp) if need_input else None
    gg = torch.empty_like(grid) if need_grid else None
    ws = None
    if use_workspace:
        nbytes = lib.enarf_triplane_sample_bwd_workspace_bytes(B, C3 // 3, H, W)
        if nbytes:
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=inp.device)
    rc = lib.enarf_triplane_sample_bwd(_p(grad_out), _p(inp), _p(grid), _p(gi), _p(gg), B, C3 // 3, H, W, h * w,
                                       mode, padding_mode, int(bool(align_corners)), _p(ws), _stream(inp.device))
    _lib.check(rc, "enarf_triplane_sample_bwd")
    return gi, gg


@_on_tensor_device
def triplane_sample_ex_fwd(inp: torch.Tensor, grid: torch.Tensor, separate: bool = False,
                           point_image: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Generalised gather (bilinear, zeros, align_corners False): input (Bimg, 3C, H, W), grid (B, n, 3) -> (B, C, n), or
    (B, 3, C, n) with `separate` (the planes' samples side by side). point_image (n,) int32 with B == 1: point i samples
    image point_image[i]."""
    lib = _lib.load()
    inp, grid = _dev_f32(inp, "input"), _dev_f32(grid, "grid")
    Bi, C3, H, W = inp.shape
    B, n, _ = grid.shape
    Cc = C3 // 3
    pi = None if point_image is None else point_image.to(device=inp.device, dtype=torch.int32).contiguous()
    out = torch.empty((B, 3, Cc, n) if separate else (B, Cc, n), dtype=torch.float32, device=inp.device)
    _lib.check(lib.enarf_triplane_sample_ex_fwd(_p(inp), _p(grid), _p(out), B, Cc, H, W, n, 0, 0, 0, int(separate), _p(pi), Bi,
                                                _stream(inp.device)), "enarf_triplane_sample_ex_fwd")
    return out


@_on_tensor_device
def triplane_sample_ex_bwd(grad_out: torch.Tensor, inp: torch.Tensor, grid: torch.Tensor, separate: bool,
                           point_image: Optional[torch.Tensor], need_input: bool, need_grid: bool):
    lib = _lib.load()
    go, inp, grid = _dev_f32(grad_out, "grad_output"), _dev_f32(inp, "input"), _dev_f32(grid, "grid")
    Bi, C3, H, W = inp.shape
    B, n, _ = grid.shape
    pi = None if point_image is None else point_image.to(device=inp.device, dtype=torch.int32).contiguous()
    gi = torch.zeros_like(inp) if need_input else None
    gg = torch.empty_like(grid) if need_grid else None
    _lib.check(lib.enarf_triplane_sample_ex_bwd(_p(go), _p(inp), _p(grid), _p(gi), _p(gg), B, C3 // 3, H, W, n, 0, 0, 0,
                                                int(separate), _p(pi), Bi, _stream(inp.device)), "enarf_triplane_sample_ex_bwd")
    return gi, gg


# ---------------------------------------------------------------------------------------- a16 ray sampler
@_on_tensor_device
def mask_dilate_topk(mask: torch.Tensor, noise: torch.Tensor, k: int, radius: int = 64) -> torch.Tensor:
    """mask (B, h, w), noise (B, h*w) -> (B, k) int64 flat pixel ids of the k largest dilate(mask) + noise per image
    (libraries/NeRF/ray_sampler.py:23-30), unordered."""
    lib = _lib.load()
    m = _dev_f32(mask, "mask")
    nz = _dev_f32(noise, "noise")
    B, h, w = m.shape
    if nz.shape != (B, h * w):
        raise ValueError(f"noise {tuple(nz.shape)} must be (B, h*w) = {(B, h * w)}")
    out = torch.empty(B, k, dtype=torch.int64, device=m.device)
    ws = torch.empty(int(lib.enarf_mask_topk_workspace_bytes(B, h, w)) // 4, dtype=torch.float32, device=m.device)
    _lib.check(lib.enarf_mask_dilate_topk(_p(m), _p(nz), _p(out), B, h, w, int(k), int(radius), _p(ws), _stream(m.device)),
               "enarf_mask_dilate_topk")
    return out


# ---------------------------------------------------------------------------------------- re-layout
@_on_tensor_device
def triplane_pack(tri_nchw: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, 96+3P, H, W) NCHW -> feature planes channel-last (B, 3, H, W, 32)."""
    lib = _lib.load()
    tri = _dev_f32(tri_nchw, "tri_plane")
    B, Ct, H, W = tri.shape
    if out is None:
        out = torch.empty(B, 3, H, W, FEAT_DIM, dtype=torch.float32, device=tri.device)
    rc = lib.enarf_triplane_pack(_p(tri), _p(out), B, Ct, H, W, _stream(tri.device))
    _lib.check(rc, "enarf_triplane_pack")
    return out


@_on_tensor_device
def triplane_unpack_add(grad_feat_cl: torch.Tensor, grad_tri_nchw: torch.Tensor) -> torch.Tensor:
    """grad_tri[:, :96] += channel-last gradient (B, 3, H, W, 32) (the inverse re-layout)."""
    lib = _lib.load()
    g = _dev_f32(grad_feat_cl, "grad_feat_cl")
    B, Ct, H, W = grad_tri_nchw.shape
    _lib.check(lib.enarf_triplane_unpack_add(_p(g), _p(grad_tri_nchw), B, Ct, H, W, _stream(g.device)),
               "enarf_triplane_unpack_add")
    return grad_tri_nchw


@_on_tensor_device
def triplane_warp_fwd(src_cl: torch.Tensor, flow: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Deformation-field producer: src_cl (1|-,3,H,W,32) channel-last constant planes, flow (B,6,H,W) -> (B,3,H,W,32)."""
    lib = _lib.load()
    src = _dev_f32(src_cl, "src_cl").reshape(3, *src_cl.shape[-3:])
    fl = _dev_f32(flow, "flow")
    B, six, H, W = fl.shape
    if six != 6 or tuple(src.shape) != (3, H, W, FEAT_DIM):
        raise ValueError(f"flow {tuple(fl.shape)} / src_cl {tuple(src_cl.shape)}: expected (B,6,H,W) and (3,H,W,{FEAT_DIM})")
    if out is None:
        out = torch.empty(B, 3, H, W, FEAT_DIM, dtype=torch.float32, device=fl.device)
    _lib.check(lib.enarf_triplane_warp_fwd(_p(src), _p(fl), _p(out), B, H, W, _stream(fl.device)), "enarf_triplane_warp_fwd")
    return out


@_on_tensor_device
def triplane_warp_bwd(g_out_cl: torch.Tensor, src_cl: torch.Tensor, flow: torch.Tensor, need_src: bool = True,
                      need_flow: bool = True):
    """-> (g_src_cl (3,H,W,32) or None, g_flow (B,6,H,W) or None)."""
    lib = _lib.load()
    g = _dev_f32(g_out_cl, "g_out_cl")
    src = _dev_f32(src_cl, "src_cl").reshape(3, *src_cl.shape[-3:])
    fl = _dev_f32(flow, "flow")
    B, _, H, W = fl.shape
    gs = torch.zeros_like(src) if need_src else None
    gf = torch.empty_like(fl) if need_flow else None
    _lib.check(lib.enarf_triplane_warp_bwd(_p(g), _p(src), _p(fl), _p(gs), _p(gf), B, H, W, _stream(fl.device)),
               "enarf_triplane_warp_bwd")
    return gs, gf


# ---------------------------------------------------------------------------------------- prepare
def _prepare_args(pose_to_camera, bone_length, canonical_bone_length, z_rend, mlp, parents, origin_location,
                  coordinate_scale, parts_out, pack_out):
    """Validated enarf_prepare_args + the tensors its pointers borrow (kept alive by the caller)."""
    pose = _dev_f32(pose_to_camera, "pose_to_camera")
    B, J = pose.shape[0], pose.shape[1]
    P = num_parts(J, origin_location)
    bl = _dev_f32(bone_length, "bone_length").reshape(B, J - 1)
    cbl = _dev_f32(canonical_bone_length, "canonical_bone_length")
    z = _dev_f32(z_rend, "z_rend")
    if cbl.numel() != P:
        raise ValueError(f"canonical_bone_length has {cbl.numel()} entries, expected {P}")
    a = _lib.PrepareArgs()
    a.B, a.num_joints, a.origin_location, a.style_dim = B, J, ORIGIN[origin_location], z.shape[1]
    a.coordinate_scale = float(coordinate_scale)
    par = np.asarray(parents, dtype=np.int64)
    for j in range(J):
        a.parents[j] = int(par[j])
    a.pose_to_camera, a.bone_length, a.canonical_bone_length, a.z_rend = _p(pose), _p(bl), _p(cbl), _p(z)
    keep = []
    dims = [(FEAT_DIM, 64), (64, 64), (64, 4)]
    for i, (cin, cout) in enumerate(dims):
        cw = _dev_f32(mlp[f"layers.{i}.conv.weight"], "conv.weight")
        mw = _dev_f32(mlp[f"layers.{i}.conv.modulation.weight"], "modulation.weight")
        mb = _dev_f32(mlp[f"layers.{i}.conv.modulation.bias"], "modulation.bias")
        bs = _dev_f32(mlp[f"layers.{i}.bias"], "bias")
        if cw.numel() != cin * cout or mw.shape != (cin, z.shape[1]) or mb.numel() != cin or bs.numel() != cout:
            raise ValueError(f"StyledMLP layer {i}: unexpected parameter shapes "
                             f"{tuple(cw.shape)} {tuple(mw.shape)} {tuple(mb.shape)} {tuple(bs.shape)}")
        keep += [cw, mw, mb, bs]
        a.conv_weight[i], a.mod_weight[i], a.mod_bias[i], a.bias[i] = _p(cw), _p(mw), _p(mb), _p(bs)
    if parts_out is None:
        parts_out = torch.empty(B, P, 16, dtype=torch.float32, device=pose.device)
    if pack_out is None:
        pack_out = torch.empty(B, mlp_pack_bytes(), dtype=torch.uint8, device=pose.device)
    a.parts, a.mlp_pack = _p(parts_out), _p(pack_out)
    keep += [pose, bl, cbl, z]
    return a, keep, parts_out, pack_out


@_on_tensor_device
def prepare(pose_to_camera: torch.Tensor, bone_length: torch.Tensor, canonical_bone_length: torch.Tensor,
            z_rend: torch.Tensor, mlp: Dict[str, torch.Tensor], parents: Sequence[int], origin_location: str,
            coordinate_scale: float, parts_out: Optional[torch.Tensor] = None,
            pack_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """24 joints -> part frames (B,P,16) and the per-image MLP pack (B, pack_bytes) uint8."""
    lib = _lib.load()
    a, _keep, parts_out, pack_out = _prepare_args(pose_to_camera, bone_length, canonical_bone_length, z_rend, mlp,
                                                  parents, origin_location, coordinate_scale, parts_out, pack_out)
    rc = lib.enarf_prepare(C.byref(a), _stream(parts_out.device))
    _lib.check(rc, "enarf_prepare")
    return parts_out, pack_out


@_on_tensor_device
def prepare_mlp(z_rend: torch.Tensor, mlp: Dict[str, torch.Tensor], pack_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """enarf_prepare with parts == NULL: only the per-image modulated, demodulated MLP pack (B, pack_bytes) uint8."""
    lib = _lib.load()
    z = _dev_f32(z_rend.detach(), "z_rend")
    B = z.shape[0]
    a = _lib.PrepareArgs()
    a.B, a.num_joints, a.origin_location, a.style_dim = B, 2, ORIGIN["center_fixed"], z.shape[1]   # joints unused without parts
    a.coordinate_scale = 1.0
    a.parents[0], a.parents[1] = -1, 0
    a.z_rend = _p(z)
    keep = [z]
    dims = [(FEAT_DIM, 64), (64, 64), (64, 4)]
    for i, (cin, cout) in enumerate(dims):
        ts = [_dev_f32(mlp[f"layers.{i}.{leaf}"].detach(), leaf) for leaf in
              ("conv.weight", "conv.modulation.weight", "conv.modulation.bias", "bias")]
        if ts[0].numel() != cin * cout or ts[1].shape != (cin, z.shape[1]) or ts[2].numel() != cin or ts[3].numel() != cout:
            raise ValueError(f"StyledMLP layer {i}: unexpected parameter shapes {[tuple(t.shape) for t in ts]}")
        keep += ts
        a.conv_weight[i], a.mod_weight[i], a.mod_bias[i], a.bias[i] = [_p(t) for t in ts]
    if pack_out is None:
        pack_out = torch.empty(B, mlp_pack_bytes(), dtype=torch.uint8, device=z.device)
    a.parts, a.mlp_pack = None, _p(pack_out)
    _lib.check(lib.enarf_prepare(C.byref(a), _stream(z.device)), "enarf_prepare")
    return pack_out


@_on_tensor_device
def mlp_unpack(pack_one_image: torch.Tensor):
    """Dense (W1 (64,32), W2 (64,64), W3 (4,64), b1, b2, b3) from one image's pack (tests / interop)."""
    lib = _lib.load()
    dense = torch.empty(64 * 32 + 64 * 64 + 4 * 64 + 132, dtype=torch.float32, device=pack_one_image.device)
    _lib.check(lib.enarf_mlp_unpack(_p(pack_one_image), _p(dense), _stream(dense.device)), "enarf_mlp_unpack")
    o = 0
    outs = []
    for shp in ((64, 32), (64, 64), (4, 64), (64,), (64,), (4,)):
        n = int(np.prod(shp))
        outs.append(dense[o:o + n].reshape(shp))
        o += n
    return outs


def _plane_strides(tri_nchw: torch.Tensor, feat_cl: torch.Tensor, B: int):
    """Batch strides (in floats) of the mask planes inside tri_nchw and of feat_cl; 0 = shared tri-plane."""
    Ct, H, W = tri_nchw.shape[1:]
    mask_stride = 0 if tri_nchw.shape[0] == 1 else Ct * H * W
    feat_stride = 0 if feat_cl.shape[0] == 1 else 3 * H * W * FEAT_DIM
    if tri_nchw.shape[0] not in (1, B) or feat_cl.shape[0] not in (1, B):
        raise ValueError("tri-plane batch must be 1 (shared) or B")
    return mask_stride, feat_stride


# ---------------------------------------------------------------------------------------- a9 query
@_on_tensor_device
def query_fwd(points: Optional[torch.Tensor], parts: torch.Tensor, canonical_pose: torch.Tensor, tri_nchw: torch.Tensor,
              feat_cl: torch.Tensor, mlp_pack: torch.Tensor, mlp_mode: str = "f32",
              multiply_density_with_weight: bool = False, need_color: bool = True, need_valid: bool = False,
              debug: bool = False, grid: Optional[Tuple[int, Sequence[float], float]] = None, clamp_mask: bool = False,
              uniform_part_weight: bool = False):
    """points (B,3,N) -> density (B,1,N), color (B,3,N) [, valid_bits (B,N) int32 [, canonical, weight]].

    grid = (D, centre (3,), scale) with points = None: the D^3 lattice of create_mesh, generated in the kernel."""
    lib = _lib.load()
    P = parts.shape[1]
    if grid is not None:
        if points is not None:
            raise ValueError("pass either points or grid")
        B, N = parts.shape[0], int(grid[0]) ** 3
        pts = parts                       # device / dtype carrier only
    else:
        pts = _dev_f32(points, "points")
        B, _, N = pts.shape
    tri = _dev_f32(tri_nchw, "tri_plane")
    H, W = tri.shape[2], tri.shape[3]
    mstride, fstride = _plane_strides(tri, feat_cl, B)
    dev = pts.device
    if N == 0:   # nothing to launch (an empty tensor has no device pointer)
        def z(*shape, dt=torch.float32):
            return torch.empty(*shape, dtype=dt, device=dev)
        out = (z(B, 1, 0), z(B, 3, 0) if need_color else None)
        if need_valid or debug:
            out = out + (z(B, 0, dt=torch.int32),)
        if debug:
            out = out + (z(B, P, 3, 0), z(B, P, 0))
        return out
    den = torch.empty(B, 1, N, dtype=torch.float32, device=dev)
    col = torch.empty(B, 3, N, dtype=torch.float32, device=dev) if need_color else None
    vb = torch.empty(B, N, dtype=torch.int32, device=dev) if (need_valid or debug) else None
    dc = torch.zeros(B, P, 3, N, dtype=torch.float32, device=dev) if debug else None
    dw = torch.zeros(B, P, N, dtype=torch.float32, device=dev) if debug else None
    a = _lib.QueryArgs()
    a.B, a.N, a.P, a.H, a.W = B, N, P, H, W
    a.mlp_mode, a.multiply_density_with_weight = MLP_MODE[mlp_mode], int(multiply_density_with_weight)
    a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
    a.points, a.parts, a.canonical_pose = (None if grid is not None else _p(pts)), _p(parts), _p(_dev_f32(canonical_pose, "canonical_pose"))
    if grid is not None:
        a.grid_D, a.grid_scale = int(grid[0]), float(grid[2])
        for j in range(3):
            a.grid_center[j] = float(grid[1][j])
    a.feat_cl, a.feat_batch_stride = _p(feat_cl), fstride
    a.mask_planes, a.mask_batch_stride = tri.data_ptr() + PLANE_CH * H * W * 4, mstride
    a.mlp_pack, a.density, a.color, a.valid_bits = _p(mlp_pack), _p(den), _p(col), _p(vb)
    a.dbg_canonical, a.dbg_weight = _p(dc), _p(dw)
    _lib.check(lib.enarf_query_fwd(C.byref(a), _stream(dev)), "enarf_query_fwd")
    out = (den, col)
    if need_valid or debug:
        out = out + (vb,)
    if debug:
        out = out + (dc, dw)
    return out


# ---------------------------------------------------------------------------------------- a13 render
_render_ws = {}


_render_epoch = {}


def _ws_key(dev: torch.device):
    return (dev.index, torch.cuda.current_stream(dev).cuda_stream)


def _render_workspace(dev: torch.device, B: int, n: int) -> torch.Tensor:
    """Workspace of enarf_render_fwd, cached per (device, stream): launches on one stream are ordered, so they can
    share it; it only grows."""
    key = _ws_key(dev)
    need = int(_lib.load().enarf_render_workspace_bytes(B, n))
    ws = _render_ws.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=dev)
        _render_ws[key] = ws
        _render_epoch[key] = 0
    return ws


_render_shape = {}


class _Epoch:
    """ws_epoch bookkeeping of the cached workspace of the current stream (include/enarf_hip.h, enarf_render_args):
    `with _Epoch(dev, shape) as k:` hands out the epoch for one forward call and, when the call went through, advances the
    count; anything that raises - and every call that does not keep count, like the backward - falls back to epoch 0, and
    so does a call whose (B, n, group_frames, per-frame planes) differs from the previous one's: a batch marched in groups
    keeps one queue-header pair per group inside the workspace, at offsets that depend on those."""

    def __init__(self, dev: torch.device, shape=None, counted: bool = True):
        self.key, self.counted, self.shape = _ws_key(dev), counted, shape

    def __enter__(self) -> int:
        same = self.shape is not None and _render_shape.get(self.key) == self.shape
        self.k = _render_epoch.get(self.key, 0) if (self.counted and same) else 0
        _render_epoch[self.key] = 0
        _render_shape[self.key] = self.shape if self.counted else None
        return self.k

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            _render_epoch[self.key] = self.k + 1
        return False


def _shape_key(a) -> tuple:
    return (a.B, a.n, a.group_frames, a.feat_batch_stride != 0)


class RenderOutputs:
    __slots__ = ("color", "mask", "disparity", "fine_weights", "fine_depth", "taps", "counters")


@_on_tensor_device
def render_fwd(image_coord: torch.Tensor, inv_intrinsics: torch.Tensor, parts: torch.Tensor,
               canonical_pose: torch.Tensor, tri_nchw: torch.Tensor, feat_cl: torch.Tensor, mlp_pack: torch.Tensor,
               Nc: int, Nf: int, render_scale: float = 1.0, bins: Optional[torch.Tensor] = None, seed: int = 0,
               mlp_mode: str = "f32", multiply_density_with_weight: bool = False,
               drop_invalid_rays: Optional[bool] = None, want_fine: bool = True, debug: bool = False,
               count: bool = False, early_stop_eps: float = 0.0, return_bins: bool = False, clamp_mask: bool = False,
               uniform_part_weight: bool = False, march: str = "auto", group_frames: int = 0) -> RenderOutputs:
    """The fused ray march. image_coord (B,1,3,n) or (B,3,n); returns color (B,3,n), mask (B,n), disparity (B,n),
    fine_weights (B,1,n,Nf-1), fine_depth (B,1,n,Nf) and, with debug=True, the parity taps."""
    lib = _lib.load()
    a, o, _keep = _render_args(image_coord, inv_intrinsics, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, Nc, Nf,
                               render_scale, bins, seed, mlp_mode, multiply_density_with_weight, drop_invalid_rays,
                               want_fine, debug, count, early_stop_eps, return_bins, clamp_mask, uniform_part_weight, march)
    a.group_frames = int(group_frames)
    with _Epoch(o.color.device, _shape_key(a)) as k:
        a.ws_epoch = k
        _lib.check(lib.enarf_render_fwd(C.byref(a), _stream(o.color.device)), "enarf_render_fwd")
    return o


def _render_args(image_coord, inv_intrinsics, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, Nc, Nf, render_scale,
                 bins, seed, mlp_mode, multiply_density_with_weight, drop_invalid_rays, want_fine, debug, count,
                 early_stop_eps, return_bins, clamp_mask=False, uniform_part_weight=False, march="auto"):
    """enarf_render_args with freshly allocated outputs + the tensors its pointers borrow."""
    coord = _dev_f32(image_coord, "image_coord")
    B, n = coord.shape[0], coord.shape[-1]
    coord = coord.reshape(B, 3, n)
    Ki = _dev_f32(inv_intrinsics, "inv_intrinsics")
    if Ki.dim() == 2:
        Ki = Ki[None].expand(B, -1, -1).contiguous()
    P = parts.shape[1]
    tri = _dev_f32(tri_nchw, "tri_plane")
    H, W = tri.shape[2], tri.shape[3]
    mstride, fstride = _plane_strides(tri, feat_cl, B)
    dev = coord.device
    o = RenderOutputs()
    o.color = torch.empty(B, 3, n, dtype=torch.float32, device=dev)
    o.mask = torch.empty(B, n, dtype=torch.float32, device=dev)
    o.disparity = torch.empty(B, n, dtype=torch.float32, device=dev)
    o.fine_weights = torch.empty(B, 1, n, Nf - 1, dtype=torch.float32, device=dev) if want_fine else None
    o.fine_depth = torch.empty(B, 1, n, Nf, dtype=torch.float32, device=dev) if want_fine else None
    o.taps, o.counters = None, None
    a = _lib.RenderArgs()
    a.B, a.n, a.P, a.Nc, a.Nf, a.H, a.W = B, n, P, Nc, Nf, H, W
    a.mlp_mode, a.multiply_density_with_weight = MLP_MODE[mlp_mode], int(multiply_density_with_weight)
    a.drop_invalid_rays = int(B == 1 if drop_invalid_rays is None else drop_invalid_rays)
    a.render_scale, a.early_stop_eps = float(render_scale), float(early_stop_eps)
    a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
    a.march = MARCH[march]
    a.image_coord, a.inv_intrinsics, a.parts = _p(coord), _p(Ki), _p(parts)
    cpose = _dev_f32(canonical_pose, "canonical_pose")
    a.canonical_pose = _p(cpose)
    a.feat_cl, a.feat_batch_stride = _p(feat_cl), fstride
    a.mask_planes, a.mask_batch_stride = tri.data_ptr() + PLANE_CH * H * W * 4, mstride
    a.mlp_pack = _p(mlp_pack)
    if bins is not None:
        bins = _dev_f32(bins, "bins").reshape(B, n, Nf)
    a.bins, a.seed = _p(bins), int(seed) & 0xFFFFFFFFFFFFFFFF
    a.color, a.mask, a.disparity = _p(o.color), _p(o.mask), _p(o.disparity)
    a.fine_weights, a.fine_depth = _p(o.fine_weights), _p(o.fine_depth)
    if debug:
        t = {
            "depth_min": torch.zeros(B, n, device=dev), "depth_max": torch.zeros(B, n, device=dev),
            "ray_validity": torch.zeros(B, n, dtype=torch.uint8, device=dev),
            "coarse_density": torch.zeros(B, n, Nc, device=dev), "fine_density": torch.zeros(B, n, Nf, device=dev),
            "fine_color": torch.zeros(B, 3, n, Nf, device=dev),
            "fine_valid": torch.zeros(B, n, Nf, dtype=torch.int32, device=dev),
            "bins": torch.zeros(B, n, Nf, device=dev),
        }
        a.dbg_depth_min, a.dbg_depth_max, a.dbg_ray_valid = _p(t["depth_min"]), _p(t["depth_max"]), _p(t["ray_validity"])
        a.dbg_coarse_density, a.dbg_fine_density = _p(t["coarse_density"]), _p(t["fine_density"])
        a.dbg_fine_color, a.dbg_fine_valid, a.dbg_bins = _p(t["fine_color"]), _p(t["fine_valid"]), _p(t["bins"])
        o.taps = t
    if return_bins and not debug:      # the importance samples actually used (needed to replay / differentiate)
        o.taps = {"bins": torch.zeros(B, n, Nf, dtype=torch.float32, device=dev)}     # rays that are dropped keep zeros
        a.dbg_bins = _p(o.taps["bins"])
    if count:
        o.counters = torch.zeros(8, dtype=torch.int64, device=dev)
        a.counters = _p(o.counters)
    ws = _render_workspace(dev, B, n)
    a.workspace = _p(ws)
    return a, o, [coord, Ki, cpose, tri, bins, ws]


STEP_PRE, STEP_MARCH, STEP_ALL = 1, 2, 3


class RenderStep:
    """One forward step bound to its arguments: `RenderStep(...).run()` = enarf_render_step_fwd (re-layout + prepare +
    ray set-up in ONE launch, then the march). `run(STEP_PRE)` / `run(STEP_MARCH)` issue the two launches separately
    (bench.py brackets the march with events that way)."""

    def __init__(self, pose_to_camera, bone_length, canonical_bone_length, z_rend, mlp, parents, origin_location,
                 coordinate_scale, image_coord, inv_intrinsics, canonical_pose, tri_nchw, feat_cl, Nc, Nf,
                 parts_out=None, pack_out=None, relayout=True, render_scale=1.0, bins=None, seed=0, mlp_mode="f32",
                 multiply_density_with_weight=False, drop_invalid_rays=None, want_fine=True, debug=False, count=False,
                 early_stop_eps=0.0, return_bins=False, clamp_mask=False, uniform_part_weight=False, march="auto",
                 group_frames=0):
        self.lib = _lib.load()
        self.pa, k1, self.parts, self.pack = _prepare_args(pose_to_camera, bone_length, canonical_bone_length, z_rend,
                                                           mlp, parents, origin_location, coordinate_scale, parts_out,
                                                           pack_out)
        self.ra, self.out, k2 = _render_args(image_coord, inv_intrinsics, self.parts, canonical_pose, tri_nchw, feat_cl,
                                             self.pack, Nc, Nf, render_scale, bins, seed, mlp_mode,
                                             multiply_density_with_weight, drop_invalid_rays, want_fine, debug, count,
                                             early_stop_eps, return_bins, clamp_mask, uniform_part_weight, march)
        self.ra.group_frames = int(group_frames)
        self.tri = _dev_f32(tri_nchw, "tri_plane")
        self.feat_cl, self.relayout = feat_cl, relayout
        if feat_cl.shape[0] != self.tri.shape[0]:
            raise ValueError("feat_cl and tri_plane must have the same batch")
        self._keep = k1 + k2

    def run(self, phases: int = STEP_ALL) -> RenderOutputs:
        if self.tri.device.index != torch.cuda.current_device():
            with torch.cuda.device(self.tri.device):
                return self._run(phases)
        return self._run(phases)

    def _run(self, phases: int) -> RenderOutputs:
        t = self.tri

        def call():
            rc = self.lib.enarf_render_step_fwd(C.byref(self.pa), _p(t) if self.relayout else None, _p(self.feat_cl),
                                                t.shape[0], t.shape[1], C.byref(self.ra), phases, _stream(t.device))
            _lib.check(rc, "enarf_render_step_fwd")

        if phases & STEP_PRE:          # a new epoch starts with the pre-march phase; a march-only call stays in it
            with _Epoch(t.device, _shape_key(self.ra)) as k:
                self.ra.ws_epoch = k
                call()
        else:
            call()
        return self.out


def render_step_fwd(*args, **kw) -> RenderOutputs:
    """prepare + tri-plane re-layout + render in two launches; arguments as RenderStep. Returns RenderOutputs
    (plus .parts / .pack of the prepare stage as attributes of the RenderStep it ran: use RenderStep to keep them)."""
    return RenderStep(*args, **kw).run()


# ---------------------------------------------------------------------------------------- backward
@_on_tensor_device
def render_bwd(image_coord, inv_intrinsics, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, Nf, bins,
               g_color, g_mask, g_disparity=None, render_scale: float = 1.0, drop_invalid_rays: Optional[bool] = None,
               feat_grad_channel_last: bool = False, clamp_mask: bool = False, uniform_part_weight: bool = False,
               multiply_density_with_weight: bool = False, counters: Optional[torch.Tensor] = None, group_frames: int = 0):
    """Backward of render_fwd w.r.t. the tri-plane and the per-image demodulated MLP weights / biases.

    Returns (grad_tri (same batch as tri_nchw: 1 for a shared tri-plane), dW [3 x (B,out,in)], db [3 x (out,)]).
    feat_grad_channel_last: the feature-plane gradient stays channel-last (same shape as feat_cl) and is returned as a
    fourth value instead of being folded into grad_tri[:, :96] (for producers that emit channel-last planes).
    The weight gradients are formed by enarf_weight_grad from the kernel's compact per-tile rows (features in, dL/dz3 out:
    it re-runs the MLP forward and backward on them; no library GEMM, no host sync).
    counters: optional zeroed int64 tensor [8] on the device (enarf_render_bwd_args.counters: pairs, tiles, rays, 128-B
    feature-gradient lines added, part-probability adds, gather rounds)."""
    lib = _lib.load()
    coord = _dev_f32(image_coord, "image_coord")
    B, n = coord.shape[0], coord.shape[-1]
    coord = coord.reshape(B, 3, n)
    Ki = _dev_f32(inv_intrinsics, "inv_intrinsics")
    if Ki.dim() == 2:
        Ki = Ki[None].expand(B, -1, -1).contiguous()
    P = parts.shape[1]
    tri = _dev_f32(tri_nchw, "tri_plane")
    Ct, H, W = tri.shape[1:]
    mstride, fstride = _plane_strides(tri, feat_cl, B)
    dev = coord.device
    rows = int(lib.enarf_render_bwd_rows_per_image(n, Nf))
    bufs, blocks = _row_buffers(B, rows, dev)
    grad_tri, gfeat = _zeros_pair(tri, feat_cl)
    a = _lib.RenderBwdArgs()
    a.B, a.n, a.P, a.Nf, a.H, a.W = B, n, P, Nf, H, W
    a.drop_invalid_rays = int(B == 1 if drop_invalid_rays is None else drop_invalid_rays)
    a.render_scale = float(render_scale)
    a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
    a.multiply_density_with_weight = int(bool(multiply_density_with_weight))
    a.image_coord, a.inv_intrinsics, a.parts = _p(coord), _p(Ki), _p(parts)
    a.canonical_pose = _p(_dev_f32(canonical_pose, "canonical_pose"))
    a.feat_cl, a.feat_batch_stride = _p(feat_cl), fstride
    a.mask_planes, a.mask_batch_stride = tri.data_ptr() + PLANE_CH * H * W * 4, mstride
    a.mlp_pack = _p(mlp_pack)
    bins = _dev_f32(bins, "bins").reshape(B, n, Nf)
    a.bins = _p(bins)
    gc = None if g_color is None else _dev_f32(g_color, "g_color").reshape(B, 3, n)
    gm = None if g_mask is None else _dev_f32(g_mask, "g_mask").reshape(B, n)
    gd = None if g_disparity is None else _dev_f32(g_disparity, "g_disparity").reshape(B, n)
    a.g_color, a.g_mask, a.g_disparity = _p(gc), _p(gm), _p(gd)
    a.grad_feat_cl, a.grad_feat_batch_stride = _p(gfeat), fstride
    a.grad_mask_planes, a.grad_mask_batch_stride = grad_tri.data_ptr() + PLANE_CH * H * W * 4, mstride
    a.rows_x, a.rows_dz3 = _p(bufs["x"]), _p(bufs["dz3"])
    a.rows_per_image, a.row_blocks = rows, _p(blocks)
    a.workspace = _p(_render_workspace(dev, B, n))
    a.group_frames = int(group_frames)
    if counters is not None:
        if counters.dtype != torch.int64 or counters.numel() < 8 or counters.device != dev:
            raise ValueError("counters: an int64 tensor of 8 elements on the inputs' device")
        a.counters = _p(counters)
    with _Epoch(dev, counted=False):      # the backward's set-up clears the headers itself and uses header 0 (of every group)
        _lib.check(lib.enarf_render_bwd(C.byref(a), _stream(dev)), "enarf_render_bwd")
    if not feat_grad_channel_last:
        _lib.check(lib.enarf_triplane_unpack_add(_p(gfeat), _p(grad_tri), grad_tri.shape[0], Ct, H, W, _stream(dev)),
                   "enarf_triplane_unpack_add")
    dW, db = _weight_grad(bufs, blocks, mlp_pack, B, rows, dev)
    if feat_grad_channel_last:
        return grad_tri, dW, db, gfeat
    return grad_tri, dW, db


def _zeros_pair(a: torch.Tensor, b: torch.Tensor):
    """zero-filled tensors shaped like a and b from ONE allocation and one fill launch (the gradient planes of a backward)"""
    na = (a.numel() + 63) // 64 * 64                      # keeps the second tensor 256-byte aligned
    buf = torch.zeros(na + b.numel(), dtype=torch.float32, device=a.device)
    return buf[:a.numel()].view(a.shape), buf[na:].view(b.shape)


def _sum_images(t: torch.Tensor) -> torch.Tensor:
    """per-image gradients of a shared parameter -> the parameter's gradient; one image: a view, not a launch (the 13 such
    sums of a C1 backward were 57 us of 4 us reduction kernels: profiles/r03_bwd_final_kernel_stats.csv)"""
    return t[0] if t.shape[0] == 1 else t.sum(dim=0)


def _row_buffers(B: int, rows: int, dev: torch.device):
    bufs = {k: torch.empty(B, rows, w, dtype=torch.float32, device=dev) for k, w in (("x", 32), ("dz3", 4))}
    return bufs, torch.zeros(B, dtype=torch.int32, device=dev)


def _weight_grad(bufs, blocks, mlp_pack, B: int, rows: int, dev: torch.device):
    """dW'_l = dZ_l^T H_{l-1} per image and db_l = column sums of dZ_l, from the compact rows (x, dz3) a backward kernel
    exported: enarf_weight_grad re-runs the MLP forward and backward on them."""
    lib = _lib.load()
    dW = [torch.empty(B, 64, 32, device=dev), torch.empty(B, 64, 64, device=dev), torch.empty(B, 4, 64, device=dev)]
    dbb = [torch.empty(B, 64, device=dev), torch.empty(B, 64, device=dev), torch.empty(B, 4, device=dev)]
    w = _lib.WeightGradArgs()
    w.B, w.rows_per_image, w.row_blocks = B, rows, _p(blocks)
    w.rows_x, w.rows_dz3, w.mlp_pack = _p(bufs["x"]), _p(bufs["dz3"]), _p(mlp_pack)
    w.dW1, w.dW2, w.dW3 = _p(dW[0]), _p(dW[1]), _p(dW[2])
    w.db1, w.db2, w.db3 = _p(dbb[0]), _p(dbb[1]), _p(dbb[2])
    wws = torch.empty(int(lib.enarf_weight_grad_workspace_bytes(B, rows)) // 4, dtype=torch.float32, device=dev)
    w.workspace = _p(wws)
    _lib.check(lib.enarf_weight_grad(C.byref(w), _stream(dev)), "enarf_weight_grad")
    return dW, [_sum_images(t) for t in dbb]


@_on_tensor_device
def query_bwd(points, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, g_density, g_color, clamp_mask: bool = False,
              uniform_part_weight: bool = False, multiply_density_with_weight: bool = False):
    """Backward of query_fwd w.r.t. the tri-plane and the per-image demodulated MLP weights / biases.

    points (B,3,N); g_density (B,1,N) or None; g_color (B,3,N) or None. Returns (grad_tri, dW [3 x (B,out,in)], db)."""
    lib = _lib.load()
    pts = _dev_f32(points, "points")
    B, _, N = pts.shape
    P = parts.shape[1]
    tri = _dev_f32(tri_nchw, "tri_plane")
    Ct, H, W = tri.shape[1:]
    mstride, fstride = _plane_strides(tri, feat_cl, B)
    dev = pts.device
    rows = max(int(lib.enarf_query_bwd_rows_per_image(N)), 16)
    bufs, blocks = _row_buffers(B, rows, dev)
    grad_tri, gfeat = _zeros_pair(tri, feat_cl)
    a = _lib.QueryBwdArgs()
    a.B, a.P, a.H, a.W, a.N = B, P, H, W, N
    a.clamp_mask, a.uniform_part_weight = int(bool(clamp_mask)), int(bool(uniform_part_weight))
    a.multiply_density_with_weight = int(bool(multiply_density_with_weight))
    a.points, a.parts = _p(pts) if N else _p(torch.zeros(1, device=dev)), _p(parts)
    a.canonical_pose = _p(_dev_f32(canonical_pose, "canonical_pose"))
    a.feat_cl, a.feat_batch_stride = _p(feat_cl), fstride
    a.mask_planes, a.mask_batch_stride = tri.data_ptr() + PLANE_CH * H * W * 4, mstride
    a.mlp_pack = _p(mlp_pack)
    gd = None if g_density is None else _dev_f32(g_density, "g_density").reshape(B, N)
    gc = None if g_color is None else _dev_f32(g_color, "g_color").reshape(B, 3, N)
    a.g_density, a.g_color = (_p(gd) if N else None), (_p(gc) if N else None)
    a.grad_feat_cl, a.grad_feat_batch_stride = _p(gfeat), fstride
    a.grad_mask_planes, a.grad_mask_batch_stride = grad_tri.data_ptr() + PLANE_CH * H * W * 4, mstride
    a.rows_x, a.rows_dz3 = _p(bufs["x"]), _p(bufs["dz3"])
    a.rows_per_image, a.row_blocks = rows, _p(blocks)
    _lib.check(lib.enarf_query_bwd(C.byref(a), _stream(dev)), "enarf_query_bwd")
    _lib.check(lib.enarf_triplane_unpack_add(_p(gfeat), _p(grad_tri), grad_tri.shape[0], Ct, H, W, _stream(dev)),
               "enarf_triplane_unpack_add")
    dW, db = _weight_grad(bufs, blocks, mlp_pack, B, rows, dev)
    return grad_tri, dW, db


@_on_tensor_device
def prepare_bwd(z_rend: torch.Tensor, mlp: Dict[str, torch.Tensor], dW):
    """dW' (3 x (B,out,in)) -> gradients of conv.weight, modulation.weight, modulation.bias (summed over the batch,
    in the parameters' own shapes) and of z_rend (B, style_dim)."""
    lib = _lib.load()
    z = _dev_f32(z_rend, "z_rend")
    B, D = z.shape
    dev = z.device
    a = _lib.PrepareBwdArgs()
    a.B, a.style_dim, a.z_rend = B, D, _p(z)
    keep, outs = [], []
    dims = [(FEAT_DIM, 64), (64, 64), (64, 4)]
    for i, (cin, cout) in enumerate(dims):
        cw = _dev_f32(mlp[f"layers.{i}.conv.weight"].detach(), "conv.weight")
        mw = _dev_f32(mlp[f"layers.{i}.conv.modulation.weight"].detach(), "modulation.weight")
        mb = _dev_f32(mlp[f"layers.{i}.conv.modulation.bias"].detach(), "modulation.bias")
        d = _dev_f32(dW[i], "dW")
        o = (torch.empty(B, cout, cin, device=dev), torch.empty(B, cin, D, device=dev), torch.empty(B, cin, device=dev))
        keep += [cw, mw, mb, d]
        outs.append(o)
        a.conv_weight[i], a.mod_weight[i], a.mod_bias[i], a.dW[i] = _p(cw), _p(mw), _p(mb), _p(d)
        a.d_conv_weight[i], a.d_mod_weight[i], a.d_mod_bias[i] = _p(o[0]), _p(o[1]), _p(o[2])
    dz = torch.empty(B, 3, D, device=dev)
    a.d_z_rend = _p(dz)
    _lib.check(lib.enarf_prepare_bwd(C.byref(a), _stream(dev)), "enarf_prepare_bwd")
    grads = {}
    for i, (cin, cout) in enumerate(dims):
        grads[f"layers.{i}.conv.weight"] = _sum_images(outs[i][0]).reshape(1, cout, cin, 1)
        grads[f"layers.{i}.conv.modulation.weight"] = _sum_images(outs[i][1])
        grads[f"layers.{i}.conv.modulation.bias"] = _sum_images(outs[i][2])
    return grads, dz.sum(1)


# ------------------------------------------------------------------------------------------------- DSO supervision
class _PhotometricLoss(torch.autograd.Function):
    """libenarf_photo.so's loss: two launches forward, one backward; the targets (color, mask) get no gradient."""

    @staticmethod
    def forward(ctx, sparse_color, sparse_mask, grid, color, mask, loss_type, color_coef, mask_coef, check_ids):
        from . import _photo_lib
        loss = _photo_lib.loss_fwd(grid, sparse_color, sparse_mask, color, mask, loss_type, color_coef, mask_coef, check_ids)
        ctx.save_for_backward(sparse_color, sparse_mask, grid, color, mask)
        ctx.cfg = (loss_type, color_coef, mask_coef)
        return loss[0], loss[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_color, g_mask):
        from . import _photo_lib
        sparse_color, sparse_mask, grid, color, mask = ctx.saved_tensors
        d_color, d_mask = _photo_lib.loss_bwd(grid, sparse_color, sparse_mask, color, mask, *ctx.cfg,
                                              None if g_color is None else g_color.contiguous(),
                                              None if g_mask is None else g_mask.contiguous())
        return d_color, d_mask, None, None, None, None, None, None, None


def photometric_loss(grid: Optional[torch.Tensor], sparse_color: torch.Tensor, sparse_mask: torch.Tensor,
                     color: torch.Tensor, mask: Optional[torch.Tensor] = None, loss_type: str = "mse",
                     color_coef: float = 1.0, mask_coef: float = 1.0, check_ids: bool = False):
    """(loss_color, loss_mask) of the reference's PhotometricLoss (libraries/NeRF/loss.py:17-48) as 0-dim fp32 device
    tensors, differentiable in sparse_color (B, 3, N) and sparse_mask (B, N); loss_mask is the integer 0 without a
    mask, as in the reference. color (B, 3, S, S) and mask (B, S, S) are the real frame, grid (B, N) int64 flat pixel
    ids in [0, S * S) (unchecked unless `check_ids`, which synchronises); grid None takes color (B, 3, N) and mask
    (B, N) as already gathered. loss_type "mse" or "mae" (the truncated MAE, threshold 0.01)."""
    if color.requires_grad or (mask is not None and mask.requires_grad):
        raise NotImplementedError("photometric_loss: the real image and mask are targets and get no gradient; detach them")
    loss_color, loss_mask = _PhotometricLoss.apply(sparse_color, sparse_mask, grid, color, mask, loss_type,
                                                   float(color_coef), float(mask_coef), bool(check_ids))
    return loss_color, (0 if mask is None else loss_mask)


def image_metrics(img: torch.Tensor, gen: torch.Tensor, mask: Optional[torch.Tensor] = None,
                  gen_mask: Optional[torch.Tensor] = None, bbox=None) -> torch.Tensor:
    """(B, 4) fp32 device tensor [ssim, mse_color, psnr, mse_mask] per image over the rectangle bbox = (x0, y0, x1, y1)
    (exclusive upper bounds; one for all images or one per image; None = the whole frame), read in place, with no host
    synchronisation. SSIM is scikit-image's structural_similarity(x * 0.5 + 0.5, data_range=1, 7 x 7 uniform window)
    averaged over the channels; psnr = 20 log10(2) - 10 log10(mse_color); mse_mask is NaN without masks. `gen` and
    `gen_mask` may already be cropped to the rectangle. A rectangle side shorter than 7 raises ValueError."""
    from . import _photo_lib
    return _photo_lib.metrics(img, gen, mask, gen_mask, bbox)


# ------------------------------------------------------------------------------------------------- GAN supervision
class _MaskGuidanceLoss(torch.autograd.Function):
    """libenarf_guide.so's loss: a memset and six launches forward (two without the push term), one backward; the bone
    mask gets no gradient. The selection is carried to the backward as the forward's state, not as an index tensor."""

    @staticmethod
    def forward(ctx, fake_mask, bone_mask, background_ratio, coef):
        from . import _guide_lib
        out, state = _guide_lib.loss_fwd(fake_mask, bone_mask, background_ratio, coef)
        ctx.save_for_backward(fake_mask, bone_mask, state)
        ctx.cfg = (background_ratio, coef)
        loss, push, bone = out[0], out[1], out[2]
        ctx.mark_non_differentiable(push, bone)
        return loss, push, bone

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, up, _push, _bone):
        from . import _guide_lib
        fake_mask, bone_mask, state = ctx.saved_tensors
        return _guide_lib.loss_bwd(fake_mask, bone_mask, *ctx.cfg, state, up), None, None, None


def mask_guidance_loss(fake_mask: torch.Tensor, bone_mask: torch.Tensor, background_ratio: float = 0.3,
                       coef: float = 10, return_terms: bool = False):
    """`nerf_patch_loss` of the reference's models/loss.py:5-30 as a 0-dim fp32 device tensor, differentiable in
    fake_mask: (push + bone) * coef with push = the mean square of the k = int(N * background_ratio) smallest mask
    values (left out when background_ratio <= 0) and bone = the mean of (1 - m)^2 over the pixels under the bone mask
    (max-pooled down to the mask's resolution, > 0.5). fake_mask is (..., s, s); bone_mask has the same shape or, for
    3-D masks, (B, S, S) with S // s >= 1. Of several values equal to the k-th smallest the ones with the lowest flat
    index are selected (include/enarf_guide.h), so the gradient is a function of the input. An empty bone mask gives a
    NaN loss and NaN gradients, as in the reference. `return_terms` adds the two unscaled terms (push, bone), detached.
    Nothing here synchronises."""
    if bone_mask.requires_grad:
        raise NotImplementedError("mask_guidance_loss: the bone mask is a target and gets no gradient; detach it")
    loss, push, bone = _MaskGuidanceLoss.apply(fake_mask, bone_mask, float(background_ratio), float(coef))
    return (loss, push, bone) if return_terms else loss


# ------------------------------------------------------------------------------------------------- animation
def interpolate_pose(pose_3d: torch.Tensor, parents: Sequence[int], num: int = 100, loop: bool = True,
                     orbit: Optional[torch.Tensor] = None, return_f32: bool = False, return_bone_length: bool = False):
    """The reference's interpolate_pose (libraries/NARF/pose_utils.py:48-115) in one launch of libenarf_anim.so: key
    poses (K, J, 4, 4) on the device, fp64 or fp32 -> (num, J, 4, 4) in the same dtype (computed in fp64 either way;
    the fp32 result is that rounded once). `orbit`, a (num,) device tensor of angles, turns frame i about the y axis
    through its mean joint translation (rotate_pose_by_angle). `return_f32` adds the fp32 copy the renderer takes,
    `return_bone_length` the (num, J - 1, 1) fp32 bone lengths of the frames. Rotations run on t = i K / num (loop) or
    i (K - 1) / (num - 1), translations on the reference's concatenated linspace blocks of num // K or num // (K - 1)
    frames: without loop the two clocks differ slightly, as in the reference. ValueError where the reference raises
    (num not a multiple of the segments) or cannot run; nothing here synchronises."""
    from . import _anim_lib
    poses, poses32, bone = _anim_lib.interpolate_pose(pose_3d, parents, num, loop, orbit,
                                                      want_f32=return_f32 or pose_3d.dtype == torch.float32,
                                                      want_bone_length=return_bone_length)
    out = (poses32 if pose_3d.dtype == torch.float32 else poses,)
    if return_f32:
        out += (poses32,)
    if return_bone_length:
        out += (bone,)
    return out if len(out) > 1 else out[0]


def compose_frames(color: torch.Tensor, mask: torch.Tensor, background=-1.0, return_masks: bool = True, out=None):
    """Rendered frames to 8-bit images in one launch of libenarf_anim.so, the demo's conversion (ENARF_GAN_demo.py:70-79)
    without the host: color (F, 3, n) or (F, 3, S, S) and mask (F, n) or (F, S, S) fp32 on the device, background a
    number, one (1, 3, S, S) image or (F, 3, S, S) images -> frames (F, S, S, 3) uint8 = trunc(clamp((c + (1 - m) bg)
    127.5 + 127.5, 0, 255)) and, with `return_masks`, masks (F, S, S) uint8 = trunc(clamp(255 m, 0, 255)); a NaN gives
    0. `out` = (frames, masks or None) writes into given contiguous tensors. Nothing here synchronises."""
    from . import _anim_lib
    frames, masks = _anim_lib.compose_frames(color, mask, background, want_masks=return_masks, out=out)
    return (frames, masks) if return_masks else frames


# ------------------------------------------------------------------------------------------------- part segmentation
def part_labels(points: torch.Tensor, parts: torch.Tensor, canonical_pose: torch.Tensor, tri_nchw: torch.Tensor, *,
                clamp_mask: bool = False, uniform_part_weight: bool = False, points_last: bool = False,
                return_valid_bits: bool = False):
    """The part that owns each point, in one launch of libenarf_seg.so: (label (B, M) int32, top (B, M), second (B, M)
    [, valid_bits (B, M) int32]). A point is owned by the part of the largest tri-plane part probability among the parts
    whose cube contains it (the lowest index among equals); label is -1 and top 0 where no cube does; second is the
    runner-up's weight, -1 without one; valid_bits are the bits query_fwd(need_valid=True) returns. points (B, 3, M) in
    the scaled camera space, or with `points_last` (M, 3) (B = 1) / (B, M, 3), read in place through their strides;
    parts (B, P, 16) from prepare, tri_nchw the (1 or B, 96 + 3P, H, W) tri-plane. No feature gather and no MLP run,
    nothing synchronises; M = 0 returns empty tensors without a launch."""
    from . import _seg_lib
    return _seg_lib.part_labels(points, parts, canonical_pose, tri_nchw, clamp_mask, uniform_part_weight, points_last,
                                return_valid_bits)


def part_labels_on_rays(image_coord: torch.Tensor, inv_intrinsics: torch.Tensor, depth_min: torch.Tensor,
                        depth_max: torch.Tensor, bins: torch.Tensor, parts: torch.Tensor, canonical_pose: torch.Tensor,
                        tri_nchw: torch.Tensor, *, clamp_mask: bool = False, uniform_part_weight: bool = False,
                        return_valid_bits: bool = False):
    """part_labels on the fine samples of a march, as (B, n, Nf) tensors: the points are formed in the kernel from the
    march's taps (render_fwd(debug=True).taps: depth_min, depth_max (B, n), bins (B, n, Nf)) with the march's own
    arithmetic, so the validity bits are the march's."""
    from . import _seg_lib
    return _seg_lib.part_labels_on_rays(image_coord, inv_intrinsics, depth_min, depth_max, bins, parts, canonical_pose,
                                        tri_nchw, clamp_mask, uniform_part_weight, return_valid_bits)


def semantic_composite(labels: torch.Tensor, fine_weights: torch.Tensor, palette: torch.Tensor):
    """Labels along each ray to the semantic map, in one launch of libenarf_seg.so: labels (B, n, Nf) int32, fine_weights
    (B, 1, n, Nf - 1) as the march returns them, palette (P, 3) -> (color (B, 3, n) = sum of w_i palette[label_i] over the
    labelled samples, part_map (B, n) int32 = the part of the largest summed weight along the ray (the lowest index among
    equals, -1 when no labelled sample has weight), part_mass (B, n) = that sum). Bit-identical from run to run."""
    from . import _seg_lib
    return _seg_lib.semantic_composite(labels, fine_weights, palette)


# ------------------------------------------------------------------------------------------------- coloured meshes
def shade_fragments(pix_to_face: torch.Tensor, bary: torch.Tensor, normals: torch.Tensor, vertices: torch.Tensor,
                    triangles: torch.Tensor, *, vertex_colors: Optional[torch.Tensor] = None,
                    vertex_labels: Optional[torch.Tensor] = None, palette: Optional[torch.Tensor] = None, lit: bool = True,
                    background=1.0, neutral=0.5):
    """The fragment buffers of rasterize_mesh to a coloured image, in one launch of libenarf_paint.so: the namedtuple
    (image (R, R, 3) uint8, albedo (R, R, 3) fp32, shaded (R, R, 3) fp32). pix_to_face (R, R) int64, bary and normals
    (R, R, 3) fp32 as rasterize_mesh returns them, vertices (V, 3) fp32, triangles (T, 3) int64 and exactly one of
    vertex_colors (V, 3) fp32 in [0, 1] or vertex_labels (V,) int32 with palette (P, 3) fp32 in [0, 1]. The texel (albedo)
    is the barycentric mix of the three vertex colours, or the palette colour of the corner with the largest barycentric
    (`neutral` for a label outside [0, P)); `lit` applies the rasteriser's hard-Phong terms to it, shaded = texel
    (0.5 + 0.3 max(c, 0)) + 0.2 specular, else shaded = texel; a pixel without a face takes `background`; image =
    floor(255 clamp(shaded, 0, 1)). background and neutral are a number or three. Computed in fp64 from the fp32 inputs;
    bit-identical from run to run, nothing synchronises. ValueError for shapes or dtypes it does not take."""
    from . import _paint_lib
    return _paint_lib.shade_fragments(pix_to_face, bary, normals, vertices, triangles, vertex_colors, vertex_labels, palette,
                                      lit, background, neutral)


# ------------------------------------------------------------------------------------------------- textured meshes
def bake_layout(T: int, size: int):
    """The texture atlas of T triangles in `size` x `size` texels: BakeLayout(cell, cells_per_row, capacity). Triangles are
    packed in pairs into square cells of `cell` texels a side, the largest integer >= 6 with 2 (size // cell)^2 >= T (the
    layout is a function of T and size alone, include/enarf_bake.h). ValueError for 6 <= size <= 8192 or 0 <= T < 2^31
    violated, NotImplementedError when size is too small for T (the message says how large it must be). Pure host
    arithmetic: no device, no library."""
    from . import _bake_lib
    return _bake_lib.bake_layout(T, size)


def bake_points(vertices: torch.Tensor, triangles: torch.Tensor, size: int, rows=None):
    """The surface point of every texel of a mesh's atlas, in one launch of libenarf_bake.so: the namedtuple (points
    (3, rows size) fp32 - three planes, the layout query_fwd takes -, texel_face (rows, size) int32 - the triangle that
    owns the texel, -1 for an empty one, whose point is (0, 0, 0)). vertices (V, 3) fp32, triangles (T, 3) int64; `rows` =
    (first, stop) restricts the call to a band of atlas rows (all rows by default), so that a large atlas is baked band
    by band. A triangle naming a vertex outside [0, V) owns nothing. Computed in fp64 from the fp32 inputs and rounded
    once; bit-identical from run to run, nothing synchronises. ValueError for shapes, dtypes or devices it does not take,
    NotImplementedError for an atlas too small for the mesh."""
    from . import _bake_lib
    return _bake_lib.bake_points(vertices, triangles, size, rows)


def bake_resolve(texel_face: torch.Tensor, *, color: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                 palette: Optional[torch.Tensor] = None, fill=0.0, neutral=0.5, want_float: bool = False,
                 unit: bool = False, out=None):
    """The colours or labels found at bake_points' points to the texture, in one launch of libenarf_bake.so: the
    namedtuple (texture (rows, size, 4) uint8, texture_f32 (rows, size, 3) fp32 or None). texel_face (rows, size) int32
    and exactly one of color (3, rows size) fp32 as query_fwd returns it, in [-1, 1] and mapped by (x + 1) / 2 (`unit`:
    already in [0, 1]), or labels (rows size) int32 with palette (P, 3) fp32 in [0, 1] (`neutral` for a label outside
    [0, P)). rgb = floor(255 clamp(v, 0, 1)), a NaN giving 0, alpha 255; an empty texel takes `fill` and alpha 0.
    `want_float` adds the unquantised fp32 texture; `out` = (texture, texture_f32 or None) writes into given tensors."""
    from . import _bake_lib
    return _bake_lib.bake_resolve(texel_face, color, labels, palette, fill, neutral, want_float, unit, out)


def shade_textured(pix_to_face: torch.Tensor, bary: torch.Tensor, normals: torch.Tensor, vertices: torch.Tensor,
                   triangles: torch.Tensor, texture: torch.Tensor, *, lit: bool = True, background=1.0):
    """shade_fragments with the albedo read from a baked texture, in one launch of libenarf_bake.so: the namedtuple (image
    (R, R, 3) uint8, albedo (R, R, 3) fp32, shaded (R, R, 3) fp32). The fragment buffers as rasterize_mesh returns them,
    the mesh they were rasterised from, and its texture: (A, A, 4) uint8 (alpha ignored) or (A, A, 3) fp32. The uv of a
    pixel is the barycentric mix of its face's corner positions in the atlas (from the layout, nothing stored), the
    albedo one bilinear tap there, clamped to the edge; the lighting is shade_fragments'. Bit-identical from run to run,
    nothing synchronises."""
    from . import _bake_lib
    return _bake_lib.shade_textured(pix_to_face, bary, normals, vertices, triangles, texture, lit, background)


# ------------------------------------------------------------------------------------------------- normal-mapped meshes
from ._nmap_lib import NormalMappedFragments, NormalMapTexture  # noqa: E402,F401  (the results of the two ops below)


def encode_normal_map(texel_face: torch.Tensor, vectors: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor,
                      negate: bool = True, min_length: float = 0.0, want_float: bool = False, out=None):
    """The vectors found at bake_points' points to a tangent-space normal map, in one launch of libenarf_nmap.so: the
    namedtuple (texture (rows, A, 4) uint8, texture_f32 (rows, A, 3) fp32 or None). texel_face (rows, A) int32 as
    bake_points returns it, vectors (3, rows A) fp32 as three planes (what field_gradient returns per image), the mesh the
    atlas belongs to. The normal of a texel is -vector with `negate` (a density gradient), else vector, expressed in the
    frame (t^, b^, n^) of the texel's triangle (include/enarf_nmap.h) and stored as round(255 (c + 1) / 2); a texel whose
    vector is no longer than min_length or not finite, or whose triangle has no frame, is the flat (128, 128, 255); an
    empty texel the same with alpha 0. `out` as in bake_resolve. ValueError for shapes, dtypes and devices before a device
    is touched; no CPU fallback."""
    from . import _nmap_lib
    return _nmap_lib.encode_normal_map(texel_face, vectors, vertices, triangles, negate, min_length, want_float, out)


def shade_normal_mapped(pix_to_face: torch.Tensor, bary: torch.Tensor, normals: torch.Tensor, vertices: torch.Tensor,
                        triangles: torch.Tensor, normal_texture: torch.Tensor, texture: Optional[torch.Tensor] = None,
                        base_color=1.0, lit: bool = True, background=1.0):
    """shade_textured with the shading normal read from a tangent-space normal map, in one launch of libenarf_nmap.so: the
    namedtuple (image (R, R, 3) uint8, albedo, normal, shaded (R, R, 3) fp32). normal_texture (A, A, 4) uint8 or (A, A, 3)
    fp32 as encode_normal_map wrote it; the albedo is one tap of `texture` (either kind of shade_textured, the same A) or
    the constant base_color. The frame is rebuilt per pixel from the vertices given here, so a posed mesh (skin_mesh)
    carries its map along. Bit-identical from run to run, nothing synchronises, no CPU fallback."""
    from . import _nmap_lib
    return _nmap_lib.shade_normal_mapped(pix_to_face, bary, normals, vertices, triangles, normal_texture, texture, base_color,
                                         lit, background)


# ------------------------------------------------------------------------------------------------- simplified meshes
def simplify_mesh(vertices: torch.Tensor, triangles: torch.Tensor, cell: float, origin=None, placement: str = "quadric",
                  reg: float = 1e-3):
    """A mesh simplified by uniform-grid vertex clustering (libenarf_simp.so; the contract is in include/enarf_simp.h): the
    named tuple (vertices (C, 3) fp32, triangles (T', 3) int64, vertex_cluster (V,) int32, cluster_size (C,) int32) on the
    mesh's device. vertices (V, 3) fp32 and triangles (T, 3) int64 device tensors; `cell` the cell size h > 0, taken as
    fp32; `origin` three fp32 at or below the vertices' minimum (the default: the minimum itself). Every vertex falls into
    the cell floor((v - origin) / h); every non-empty cell becomes one vertex (numbered by ascending cx, cy, cz), placed at
      placement="mean"     the mean of the cell's vertices;
      placement="quadric"  the point nearest the planes of the fine triangles that touch the cell, each weighed by its
                           squared area, regularised toward the mean with `reg` x trace and clamped to the cell's box;
    triangles with two corners in a cell are dropped, the others renamed, one copy of each distinct oriented triple kept,
    in lexicographic order with the smallest index first in each. All fp64 from the stored fp32, every sum in a fixed
    order, no atomics: two calls give the same bits. The output sizes depend on the data, so the call synchronises with
    the host (for the vertices' bounds, the cluster count and the compaction of the triples). ValueError /
    NotImplementedError before any launch for wrong shapes or dtypes, a cell that is not finite and > 0, non-finite
    vertices, an origin above the minimum, 2^21 cells or more on an axis, V or 3 T >= 2^31 and an unknown placement; an
    empty mesh gives empty outputs and launches nothing. Clustering does not preserve topology: thin gaps can close and
    edges can become non-manifold. There is no CPU fallback."""
    from . import _simp_lib
    return _simp_lib.simplify_mesh(vertices, triangles, cell, origin, placement, reg)


# ------------------------------------------------------------------------------------------------- rigged meshes
def skin_weights(vertices: torch.Tensor, parts_rest: torch.Tensor, canonical_pose: torch.Tensor, tri_plane: torch.Tensor, *,
                 max_influences: int = 4, clamp_mask: bool = False, uniform_part_weight: bool = False,
                 coordinate_scale: float = 1.0, return_valid_bits: bool = False):
    """The skin weights of mesh vertices, in one launch of libenarf_skin.so: (joints (V, K) int32, weights (V, K) fp32,
    kept_mass (V,) fp32[, valid_bits (V,) int32]), K = max_influences (4 or 8). A vertex is bound to the K parts of the
    largest tri-plane part probability among the parts whose cube contains it in the rest pose (part_labels' validity and
    weights; the lower index first among equals), by descending weight, the weights normalised to sum 1; unused slots
    hold joint -1 and weight 0. kept_mass is the share of the whole probability mass the kept parts carry (1 when at most
    K parts contain the vertex). A vertex no cube contains follows the part whose cube is nearest (joint slot 0, weight 1,
    kept_mass 0). vertices (V, 3) fp32 in camera units (a (3, V).t() view is read in place), multiplied by
    coordinate_scale in the kernel; parts_rest (1, P, 16) from prepare, tri_plane the (1, 96 + 3P, H, W) tri-plane.
    Nothing synchronises; V = 0 returns empty tensors without a launch."""
    from . import _skin_lib
    return _skin_lib.skin_weights(vertices, parts_rest, canonical_pose, tri_plane, max_influences, clamp_mask,
                                  uniform_part_weight, coordinate_scale, return_valid_bits)


def skin_pose(vertices: torch.Tensor, joints: torch.Tensor, weights: torch.Tensor, parts_rest: torch.Tensor,
              parts: torch.Tensor, *, coordinate_scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mesh in F poses, in one launch of libenarf_skin.so: (F, V, 3) fp32, frame f = sum_j weights[:, j] M_j^f v with
    M_k^f = rho_k R_k^f R_k^rest^T (v - t_k^rest) + t_k^f and rho_k the bone-length ratio of frame f over the rest pose:
    linear-blend skinning with one uniform scale a bone. vertices (V, 3) fp32 in camera units, joints and weights (V, 4 or
    8) from skin_weights, parts_rest (1, P, 16) and parts (F, P, 16) from prepare (their translations are divided by
    coordinate_scale). `out` writes into a given (F, V, 3) tensor or slice whose frames are contiguous. Computed in fp64
    from the fp32 inputs and rounded once, bit-identical from run to run, nothing synchronises."""
    from . import _skin_lib
    return _skin_lib.skin_pose(vertices, joints, weights, parts_rest, parts, coordinate_scale, out)


# ------------------------------------------------------------------------------------------------- differentiable pose
def query_pose_bwd(points: torch.Tensor, parts: torch.Tensor, canonical_pose: torch.Tensor, tri_nchw: torch.Tensor,
                   feat_cl: torch.Tensor, mlp_pack: torch.Tensor, g_density: Optional[torch.Tensor],
                   g_color: Optional[torch.Tensor], clamp_mask: bool = False, uniform_part_weight: bool = False,
                   multiply_density_with_weight: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Backward of query_fwd (mode f32) w.r.t. the sample points and the part records, the two inputs query_bwd leaves out,
    in two launches of libenarf_pgrad.so: (g_points (B, 3, N), g_parts (B, P, 16)) fp32. Arguments as query_fwd / query_bwd
    take them: points (B, 3, N), parts (B, P, 16) and mlp_pack from prepare, tri_nchw the (1 or B, 96 + 3P, H, W) tri-plane,
    feat_cl its channel-last feature planes from triplane_pack; g_density (B, N) or (B, 1, N) and g_color (B, 3, N), either
    of which may be None. g_parts is laid out as the record: dL/dR row-major in 0..8, dL/dt (the scaled translation) in
    9..11, dL/ds in 12, zeros in 13..15. The gradient is what the reference's autograd returns for its query, the density
    activation's own backward rule included; validity and the bilinear cells are constants. A point in no cube gets
    zeros. No atomics: bit-identical from run to run; nothing synchronises. ValueError for shapes it does not take."""
    from . import _pgrad_lib
    return _pgrad_lib.query_pose_bwd(points, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, g_density, g_color,
                                     clamp_mask, uniform_part_weight, multiply_density_with_weight)


# ------------------------------------------------------------------------------------------------- geometry buffers
from ._geom_lib import DepthError, GeometryBuffers  # noqa: E402,F401  (the running depth error; geometry_buffers' result)


def geometry_buffers(disparity: torch.Tensor, mask: torch.Tensor, inv_intrinsics: torch.Tensor, *, size=None, origin=(0, 0),
                     step=1.0, depth_scale=1.0, mask_threshold=0.5, edge=0.05, normalise=True, shade="normal", near=None,
                     far=None, background=1.0, want=("depth", "points", "normals", "flags", "image"), out=None):
    """The disparity and mask of a march to geometry, in one launch of libenarf_geom.so: the namedtuple GeometryBuffers
    (depth (B, H, W) fp32, points (B, H, W, 3) fp32 in camera space, normals (B, H, W, 3) fp32, flags (B, H, W) uint8 with
    bit 0 = valid and bit 1 = normal valid, image (B, H, W, 3) uint8); a field not named in `want` is None and is not
    written. disparity and mask are (B, H, W), or (B, n) with size=(H, W); inv_intrinsics (3, 3), (1, 3, 3) or (B, 3, 3).
    Pixel (r, c) sits at x = origin[0] + (c + 0.5) step, y = origin[1] + (r + 0.5) step. A pixel is valid when its mask is
    at least mask_threshold and its disparity positive; depth = depth_scale mask / disparity (the march's disparity is not
    divided by the mask), or depth_scale / disparity with normalise=False; point = depth K^-1 (x, y, 1). Normals come from
    the differences of the 4-neighbours whose depth lies within `edge` (relative; negative = no test) of the pixel's, and
    face the camera. shade: "normal" (0.5 + 0.5 (Nx, -Ny, -Nz)), "lit" (the rasteriser's hard-Phong terms on white) or
    "depth" ((1 / z - 1 / far) / (1 / near - 1 / far)); pixels without what the mode needs take `background`, a number or
    three. `out` maps names of `want` to contiguous tensors to write into. Computed in fp64 from the fp32 inputs,
    bit-identical from run to run, nothing synchronises. ValueError for shapes, dtypes or values it does not take."""
    from . import _geom_lib
    return _geom_lib.geometry_buffers(disparity, mask, inv_intrinsics, size, origin, step, depth_scale, mask_threshold, edge,
                                      normalise, shade, near, far, background, want, out)


# ------------------------------------------------------------------------------------------------- field normals
from ._nrm_lib import RayNormals  # noqa: E402,F401  (ray_normals' result)


def field_gradient(points: torch.Tensor, parts: torch.Tensor, canonical_pose: torch.Tensor, tri_nchw: torch.Tensor,
                   feat_cl: torch.Tensor, mlp_pack: torch.Tensor, clamp_mask: bool = False, uniform_part_weight: bool = False,
                   multiply_density_with_weight: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The density of query_fwd (mode f32) and its spatial gradient, in one launch of libenarf_nrm.so: (density (B, N),
    gradient (B, 3, N)) fp32, the gradient in the space the points are given in (the scaled camera space). Arguments as
    query_pose_bwd takes them, without upstream gradients. The gradient is query_pose_bwd's g_points for g_density = 1 and
    g_color = None - what the reference's autograd returns for sum(density): zero where the density head is off, validity
    and the bilinear cells constants - without the colour head, the record gradients and the second launch. A point in no
    cube gets density 0 and an exact zero gradient. The surface normal is -gradient / |gradient|. No atomics:
    bit-identical from run to run; nothing synchronises; N = 0 launches nothing. ValueError for shapes it does not take."""
    from . import _nrm_lib
    return _nrm_lib.field_gradient(points, parts, canonical_pose, tri_nchw, feat_cl, mlp_pack, clamp_mask, uniform_part_weight,
                                   multiply_density_with_weight)


def ray_normals(gradient: torch.Tensor, weights: torch.Tensor, mask: torch.Tensor, *, fallback: Optional[torch.Tensor] = None,
                flags: Optional[torch.Tensor] = None, points: Optional[torch.Tensor] = None, shade: Optional[str] = None,
                mask_threshold=0.5, min_gradient=0.0, background=1.0, want_magnitude: bool = False) -> RayNormals:
    """The field normal of every ray of a march, in one launch of libenarf_nrm.so: the namedtuple RayNormals (normals
    (B, n, 3) fp32, flags (B, n) uint8, magnitude (B, n) fp32 or None, image (B, n, 3) uint8 or None). gradient (B, 3, n Nf)
    from field_gradient at the march's fine points (ray-major, sample-minor), weights the march's fine_weights (B, n,
    Nf - 1) or (B, 1, n, Nf - 1) - weight i belongs to sample i, as in composite_fine -, mask (B, n), or (B, H, W) for
    outputs of that shape. G = sum_i w_i g_i over the first Nf - 1 samples in ascending order, m = |G|; a ray has a field
    normal -G / m when mask >= mask_threshold and m > min_gradient; otherwise it takes `fallback` (B, n, 3) where bit 1 of
    `flags` (B, n) uint8 is set - the normals and flags geometry_buffers returns - or zeros. The flags returned keep the
    given bits and set bit 2 on a field normal. `shade` = "normal" or "lit" adds the 8-bit image in geometry_buffers'
    formulas over `background` ("lit" takes `points` (B, n, 3)); `want_magnitude` adds m. Computed in fp64 from the fp32
    inputs, bit-identical from run to run, nothing synchronises. NotImplementedError for Nf outside [2, 128] or B above
    65535, ValueError for shapes, dtypes or values it does not take."""
    from . import _nrm_lib
    return _nrm_lib.ray_normals(gradient, weights, mask, fallback, flags, points, shade, mask_threshold, min_gradient,
                                background, want_magnitude)


# ------------------------------------------------------------------------------------------------- multi-avatar scenes
from ._scene_lib import SceneComposite  # noqa: E402,F401  (scene_composite's result)


def scene_composite(depth: torch.Tensor, density: torch.Tensor, color: torch.Tensor, valid: Optional[torch.Tensor] = None, *,
                    render_scale=1.0, threshold=0.5,
                    want=("color", "mask", "disparity", "instance_mass", "instance", "skipped"), out=None):
    """K avatars marched on the same n rays to one image, in one launch of libenarf_scene.so: the namedtuple SceneComposite
    (color (F, 3, n), mask (F, n), disparity (F, n), instance_mass (F, K, n) fp32, instance (F, n) and skipped (F, n) int32,
    and the merged samples t, source, weight (F, n, K Nf)); a field not named in `want` is None and is not written. depth
    and density are (F, K, n, Nf), color (F, K, 3, n, Nf), valid (F, K, n) uint8 or None - the fine_depth, fine_density and
    fine_color taps and the ray_validity of render_fwd(debug=True) on a batch of F K images, read in place; without the
    frame axis (K, n, Nf) is one frame and the outputs lose it too. Every avatar is the medium of the march's own
    quadrature on the running maximum of its depths; the scene is the sum of the media, integrated over the merged
    breakpoints (include/enarf_scene.h): mask = 1 - exp(-sum tau), instance_mass sums to the mask over the avatars,
    instance is the avatar of the largest share where mask >= threshold, else -1. An avatar takes no part on a ray where
    its validity byte is 0, or - bit k of `skipped` is then set - where a value is not finite, a depth <= 0 or a density
    < 0. `out` maps names of `want` to contiguous tensors to write into. Computed in fp64 from the fp32 inputs,
    bit-identical from run to run, nothing synchronises, F n = 0 launches nothing. No gradient: inputs that require one
    raise NotImplementedError, as do K outside [1, 8], Nf outside [2, 128] and K Nf > 512; ValueError for shapes or dtypes
    it does not take."""
    from . import _scene_lib
    return _scene_lib.scene_composite(depth, density, color, valid, render_scale, threshold, want, out)


# ------------------------------------------------------------------------------------------------- differentiable scenes
from ._sgrad_lib import SceneGradients  # noqa: E402,F401  (scene_composite_bwd's result)


def scene_composite_bwd(depth: torch.Tensor, density: torch.Tensor, color: torch.Tensor, valid: Optional[torch.Tensor] = None,
                        render_scale=1.0, g_color: Optional[torch.Tensor] = None, g_mask: Optional[torch.Tensor] = None,
                        g_disparity: Optional[torch.Tensor] = None, g_instance_mass: Optional[torch.Tensor] = None,
                        want=("density", "color"), out=None):
    """Backward of scene_composite with respect to the avatars' densities and colours, in one launch of libenarf_sgrad.so:
    the namedtuple SceneGradients (density (F, K, n, Nf), color (F, K, 3, n, Nf) fp32); a field not named in `want` is None
    and is not written. depth, density, color, valid and render_scale as scene_composite takes them (without the frame
    axis (K, n, Nf) is one frame and the outputs lose it too); the upstream gradients g_color (F, 3, n), g_mask and
    g_disparity (F, n), g_instance_mass (F, K, n) fp32, each of which may be None (zeros), at least one given. The
    gradient is that of g_color . colour + g_mask mask + g_disparity disparity + sum_k g_instance_mass[k]
    instance_mass[k] at fixed depths (include/enarf_sgrad.h has the formulas); at a density of exactly 0 it is the
    derivative from inside s >= 0. Every entry is written: an avatar's last sample, an avatar that takes no part on a ray
    and a ray nobody takes part on get exact zeros. `out` maps names of `want` to contiguous tensors to write into.
    Computed in fp64 from the fp32 inputs without atomics, bit-identical from run to run, nothing synchronises, F n = 0
    launches nothing. NotImplementedError for K outside [1, 8], Nf outside [2, 128] and K Nf > 512; ValueError for
    shapes or dtypes it does not take, an empty `want` and a call without any upstream gradient."""
    from . import _sgrad_lib
    return _sgrad_lib.scene_composite_bwd(depth, density, color, valid, render_scale, g_color, g_mask, g_disparity,
                                          g_instance_mass, want, out)


def scene_composite_posable(depth: torch.Tensor, density: torch.Tensor, color: torch.Tensor,
                            valid: Optional[torch.Tensor] = None, render_scale=1.0):
    """scene_composite for densities and colours that require gradients: (color (F, 3, n), mask (F, n), disparity (F, n),
    instance_mass (F, K, n)) through a torch.autograd.Function whose forward is scene_composite on the detached inputs,
    bit for bit, and whose backward is scene_composite_bwd. The depths are constants: a depth that requires a gradient
    raises NotImplementedError. scene_composite itself keeps refusing inputs that require gradients."""
    from . import _sgrad_lib
    return _sgrad_lib.scene_composite_posable(depth, density, color, valid, render_scale)
