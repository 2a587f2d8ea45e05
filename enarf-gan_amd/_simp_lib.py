"""ctypes binding of libenarf_simp.so (the C ABI declared in include/enarf_simp.h): simplification of a triangle mesh by
uniform-grid vertex clustering with quadric placement, on the device.

Loading, return codes and the device-argument checks are `_loader`'s. The library holds the three kernels (cell keys,
cluster triples and incidence slots, placement); the stable sorts, the segment offsets and the compaction between them are
torch calls here. `check_simplify_args` makes every host check and needs neither the library nor a device.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from typing import Optional, Tuple

from ._loader import Library, stream_of

ABI_VERSION = 1

AXIS_BITS = 21
NO_CLUSTER = 0x7FFFFFFF
PLACEMENTS = ("mean", "quadric")

_p = C.c_void_p


class KeysArgs(C.Structure):
    _fields_ = [("V", C.c_int64), ("origin", C.c_float * 3), ("cell", C.c_float), ("vertices", _p), ("keys", _p)]


class CornersArgs(C.Structure):
    _fields_ = [("V", C.c_int64), ("T", C.c_int64), ("C", C.c_int32), ("reserved", C.c_int32),
                ("triangles", _p), ("vertex_cluster", _p), ("triples", _p), ("incidence", _p)]


class PlaceArgs(C.Structure):
    _fields_ = [("V", C.c_int64), ("T", C.c_int64), ("C", C.c_int32), ("quadric", C.c_int32),
                ("origin", C.c_float * 3), ("cell", C.c_float), ("reg", C.c_double),
                ("vertices", _p), ("triangles", _p), ("keys", _p), ("vertex_order", _p), ("vertex_start", _p),
                ("slot_order", _p), ("slot_start", _p), ("out", _p)]


# every symbol include/enarf_simp.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "enarf_simp_abi_version": (C.c_int, []),
    "enarf_simp_last_error": (C.c_char_p, []),
    "enarf_simp_keys": (C.c_int, [C.POINTER(KeysArgs), _p]),
    "enarf_simp_corners": (C.c_int, [C.POINTER(CornersArgs), _p]),
    "enarf_simp_place": (C.c_int, [C.POINTER(PlaceArgs), _p]),
}

SimplifiedMesh = namedtuple("SimplifiedMesh", ["vertices", "triangles", "vertex_cluster", "cluster_size"])

_library = Library("simp", ABI_VERSION, SIGNATURES, "Mesh simplification has no CPU fallback.")
load, check = _library.load, _library.check


def _f32(x: float) -> float:
    """x rounded to fp32, as a Python float (inf when it overflows)"""
    try:
        return C.c_float(float(x)).value
    except OverflowError:
        return math.inf if x > 0 else -math.inf


def check_simplify_args(vertices, triangles, cell, origin=None, placement: str = "quadric", reg: float = 1e-3,
                        bounds=None) -> Tuple[int, int, float, Optional[Tuple[float, float, float]]]:
    """(V, T, the cell size as fp32, the origin as three fp32 or None for an empty mesh) of a simplify_mesh call, or
    ValueError / NotImplementedError. `bounds` = (minimum, maximum) of the vertices per axis, three numbers each; when it is
    None it is taken from `vertices` (a host synchronisation for a device tensor). Touches no device otherwise."""
    import torch
    who = "simplify_mesh"
    for name, t, dtype in (("vertices", vertices, torch.float32), ("triangles", triangles, torch.int64)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who} takes tensors; {name} is {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"{who} takes {dtype} {name}, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who} takes ({name[0].upper()}, 3) {name}, got {tuple(t.shape)}")
    V, T = vertices.shape[0], triangles.shape[0]
    if V >= 2 ** 31 or 3 * T >= 2 ** 31:
        raise ValueError(f"{who}: V = {V}, T = {T}: V and 3 T must lie in [0, 2^31)")
    try:
        h = _f32(cell)
    except (TypeError, ValueError):
        raise ValueError(f"{who} takes a number as cell, got {cell!r}") from None
    if not math.isfinite(h) or h <= 0:
        raise ValueError(f"{who}: the cell size must be finite and > 0 as fp32, got {cell!r}")
    if placement not in PLACEMENTS:
        raise ValueError(f"{who}: placement is 'quadric' or 'mean', got {placement!r}")
    try:
        r = float(reg)
    except (TypeError, ValueError):
        raise ValueError(f"{who} takes a number as reg, got {reg!r}") from None
    if not math.isfinite(r) or r <= 0:
        raise ValueError(f"{who}: reg must be finite and > 0, got {reg!r}")
    o = None
    if origin is not None:
        try:
            o = tuple(_f32(x) for x in (origin.reshape(-1).tolist() if isinstance(origin, torch.Tensor) else origin))
        except (TypeError, ValueError):
            raise ValueError(f"{who} takes three numbers as origin, got {origin!r}") from None
        if len(o) != 3 or not all(math.isfinite(x) for x in o):
            raise ValueError(f"{who} takes three finite numbers as origin, got {origin!r}")
    if V == 0:
        return V, T, h, o
    if bounds is None:
        bounds = vertex_bounds(vertices)
    try:
        lo, hi = (tuple(float(x) for x in b) for b in bounds)
    except (TypeError, ValueError):
        raise ValueError(f"{who} takes bounds as (minimum, maximum) of three numbers each, got {bounds!r}") from None
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"{who} takes bounds as (minimum, maximum) of three numbers each, got {bounds!r}")
    if not all(math.isfinite(x) for x in lo + hi):
        raise ValueError(f"{who}: the vertices are not all finite (bounds {lo} to {hi})")
    if o is None:
        o = lo
    for k in range(3):
        if o[k] > lo[k]:
            raise ValueError(f"{who}: origin[{k}] = {o[k]} lies above the vertices' minimum {lo[k]}")
        cells = math.floor((hi[k] - o[k]) / h)          # the arithmetic of the key kernel: doubles of the fp32 values
        if cells >= 2 ** AXIS_BITS:
            raise NotImplementedError(f"{who}: axis {k} spans {cells + 1} cells of {h}; a key holds 2^{AXIS_BITS} an axis")
    return V, T, h, o


def vertex_bounds(vertices):
    """((min x, min y, min z), (max x, max y, max z)) of (V, 3) vertices, V >= 1, as Python floats; a NaN or an infinity
    among the vertices shows in them (torch's amin / amax propagate a NaN). For a device tensor this is a device -> host
    synchronisation."""
    import torch
    both = torch.stack([vertices.amin(0), vertices.amax(0)]).double().cpu()
    return tuple(both[0].tolist()), tuple(both[1].tolist())


def _empty(dev) -> SimplifiedMesh:
    import torch
    return SimplifiedMesh(torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int64, device=dev),
                          torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))


def _starts(counts):
    """(C + 1) int64 segment starts of (C) counts"""
    import torch
    out = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=out[1:])
    return out


def vertex_keys(vertices, h: float, origin, V: int):
    """Stage 1, simp_key_kernel: (V) int64 cell keys, no synchronisation"""
    import torch
    dev = vertices.device
    lib = load()
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    a = KeysArgs()
    a.V, a.cell = V, h
    a.origin[:] = origin
    a.vertices, a.keys = vertices.data_ptr(), keys.data_ptr()
    check(lib.enarf_simp_keys(C.byref(a), stream_of(dev)), "enarf_simp_keys")
    return keys


def cluster_vertices(keys):
    """The clusters of simp_key_kernel's keys, by torch's stable sort: (keys (C) int64 ascending, vertex_cluster (V) int32,
    cluster_size (C) int64, vertex_order (V) int64, vertex_start (C + 1) int64). unique_consecutive sizes its outputs from
    the data: the second host synchronisation of a simplify_mesh call."""
    import torch
    sorted_keys, order = torch.sort(keys, stable=True)
    cluster_keys, inverse, counts = torch.unique_consecutive(sorted_keys, return_inverse=True, return_counts=True)
    vertex_cluster = torch.empty(keys.numel(), dtype=torch.int32, device=keys.device)
    vertex_cluster[order] = inverse.to(torch.int32)
    return cluster_keys, vertex_cluster, counts, order, _starts(counts)


def cluster_corners(triangles, vertex_cluster, V: int, T: int, n_clusters: int):
    """Stage 2, simp_corner_kernel: (triples (T, 3) int32, incidence (T, 3) int32), no synchronisation"""
    import torch
    dev = triangles.device
    lib = load()
    triples = torch.empty(T, 3, dtype=torch.int32, device=dev)
    incidence = torch.empty(T, 3, dtype=torch.int32, device=dev)
    a = CornersArgs()
    a.V, a.T, a.C = V, T, n_clusters
    a.triangles, a.vertex_cluster = (t.data_ptr() if t.numel() else None for t in (triangles, vertex_cluster))
    a.triples, a.incidence = (t.data_ptr() if t.numel() else None for t in (triples, incidence))
    check(lib.enarf_simp_corners(C.byref(a), stream_of(dev)), "enarf_simp_corners")
    return triples, incidence


def incidence_segments(incidence, n_clusters: int):
    """(slot_order (3 T) int64, slot_start (C + 1) int64): the incidence slots sorted by cluster (stable: by triangle, then
    by corner, inside a cluster), the NO_CLUSTER slots last and outside every segment"""
    import torch
    flat = incidence.reshape(-1)
    sorted_inc, order = torch.sort(flat, stable=True)
    edges = torch.arange(n_clusters + 1, dtype=torch.int32, device=flat.device)
    return order, torch.searchsorted(sorted_inc, edges).to(torch.int64)


def place_clusters(vertices, triangles, cluster_keys, vertex_order, vertex_start, slot_order, slot_start, h: float, origin,
                   reg: float, quadric: bool, V: int, T: int):
    """Stage 3, simp_place_kernel<quadric or mean>: (C, 3) fp32 vertices, no synchronisation"""
    import torch
    dev = vertices.device
    lib = load()
    n = cluster_keys.numel()
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    a = PlaceArgs()
    a.V, a.T, a.C, a.quadric, a.cell, a.reg = V, T, n, int(quadric), h, reg
    a.origin[:] = origin
    ptr = lambda t: None if t is None or not t.numel() else t.data_ptr()
    a.vertices, a.triangles, a.keys = ptr(vertices), ptr(triangles), ptr(cluster_keys)
    a.vertex_order, a.vertex_start, a.slot_order, a.slot_start = ptr(vertex_order), ptr(vertex_start), ptr(slot_order), ptr(slot_start)
    a.out = ptr(out)
    check(lib.enarf_simp_place(C.byref(a), stream_of(dev)), "enarf_simp_place")
    return out


def compact_triples(triples):
    """The kept triples of simp_corner_kernel, one copy of each, in lexicographic order, as (T', 3) int64: two stable sorts
    (by the last two columns in one 64-bit key, then by the first) and unique_consecutive. Two data-dependent sizes (the kept triples, the
    distinct ones): two host synchronisations"""
    import torch
    kept = triples[triples[:, 0] >= 0].to(torch.int64)
    if kept.shape[0] == 0:
        return kept
    kept = kept[torch.sort((kept[:, 1] << 32) | kept[:, 2], stable=True)[1]]
    kept = kept[torch.sort(kept[:, 0], stable=True)[1]]
    return torch.unique_consecutive(kept, dim=0)


def simplify_mesh(vertices, triangles, cell, origin=None, placement: str = "quadric", reg: float = 1e-3) -> SimplifiedMesh:
    """SimplifiedMesh(vertices (C, 3) fp32, triangles (T', 3) int64, vertex_cluster (V) int32, cluster_size (C) int32) on the
    mesh's device and its current stream; the contract is in include/enarf_simp.h. Three launches and torch's sorts between
    them. The sizes C and T' depend on the data, so the call synchronises with the host, as marching_cubes does: once for
    the vertices' bounds (the host checks need them, check_simplify_args), once where unique_consecutive counts the clusters
    (cluster_vertices), and twice in compact_triples (the kept triples, the distinct ones). An empty mesh launches
    nothing."""
    import torch
    V, T, h, o = check_simplify_args(vertices, triangles, cell, origin, placement, reg)
    dev = vertices.device
    if dev.type != "cuda" or triangles.device != dev:
        raise ValueError(f"simplify_mesh takes device tensors on one device (there is no CPU fallback); vertices are on "
                         f"{dev}, triangles on {triangles.device}")
    if V == 0:
        return _empty(dev)
    vertices, triangles = vertices.contiguous(), triangles.contiguous()
    quadric = placement == "quadric"
    with torch.cuda.device(dev):
        keys, vertex_cluster, counts, vertex_order, vertex_start = cluster_vertices(vertex_keys(vertices, h, o, V))
        triples, incidence = cluster_corners(triangles, vertex_cluster, V, T, keys.numel())
        slot_order, slot_start = incidence_segments(incidence, keys.numel()) if quadric else (None, None)
        out = place_clusters(vertices, triangles, keys, vertex_order, vertex_start, slot_order, slot_start, h, o, float(reg),
                             quadric, V, T)
        new_triangles = compact_triples(triples)
    return SimplifiedMesh(out, new_triangles, vertex_cluster, counts.to(torch.int32))
