"""Float64 numpy restatement of the mesh simplification contract (include/enarf_simp.h): uniform-grid vertex
clustering with quadric placement. Written from the contract, not from the kernels: every sum is sequential in index order
(np.add.at), the 3 x 3 systems go through np.linalg.solve. Needs neither the library nor a device."""
import collections

import numpy as np

Simplified = collections.namedtuple("Simplified", ["vertices", "triangles", "vertex_cluster", "cluster_size", "info"])


def cells_of(vertices, h, origin):
    """(V, 3) int64: floor((double(v) - double(origin)) / double(h))"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    return np.floor((v - np.asarray(origin, np.float32).astype(np.float64)) / float(np.float32(h))).astype(np.int64)


def simplify(vertices, triangles, cell, origin=None, placement="quadric", reg=1e-3):
    """Simplified(vertices (C, 3) fp32, triangles (T', 3) int64, vertex_cluster (V,) int32, cluster_size (C,) int32, info).
    info: `unclamped` (C, 3) float64 the vertex before the clamp, `clamped` (C,) bool the clamp moved it, `cond` (C,) the
    condition number of A + lambda I (nan where the mean was taken), `trace` (C,)."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    V = len(v32)
    h = float(np.float32(cell))
    if V == 0:
        z = np.zeros(0, np.int32)
        return Simplified(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), z, z, {})
    o32 = v32.min(0) if origin is None else np.asarray(origin, np.float32).reshape(3)
    o = o32.astype(np.float64)
    v = v32.astype(np.float64)
    c = cells_of(v32, h, o32)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    keys, cluster = np.unique(key, return_inverse=True)
    cluster = cluster.reshape(-1)
    C = len(keys)
    size = np.bincount(cluster, minlength=C)
    cc = np.stack([keys >> 42, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF], -1)
    lo = o + cc.astype(np.float64) * h                                         # (C, 3)

    rel = v - lo[cluster]
    mean = np.zeros((C, 3))
    np.add.at(mean, cluster, rel)
    mean /= size[:, None]

    valid = ((tri >= 0) & (tri < V)).all(1)
    tv = tri[valid]
    x = mean.copy()
    cond = np.full(C, np.nan)
    trace = np.zeros(C)
    if placement == "quadric":
        A = np.zeros((C, 3, 3))
        b = np.zeros((C, 3))
        tc = cluster[tv]                                                       # (Tv, 3)
        slot, ids, t = [], [], []
        for k in range(3):
            first = np.ones(len(tv), bool)
            for j in range(k):
                first &= tc[:, j] != tc[:, k]                                  # a cluster named twice counts once
            slot.append(3 * np.nonzero(first)[0] + k)
            ids.append(tc[first, k])
            t.append(tv[first])
        order = np.argsort(np.concatenate(slot), kind="stable")               # by triangle, then by corner
        ids, t = np.concatenate(ids)[order], np.concatenate(t)[order]
        p = v[t] - lo[ids][:, None, :]                                         # corners relative to this cluster's corner
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        d = (n * p[:, 0]).sum(-1)
        np.add.at(A, ids, n[:, :, None] * n[:, None, :])
        np.add.at(b, ids, n * d[:, None])
        trace = np.trace(A, axis1=1, axis2=2)
        for i in np.nonzero(trace > 0)[0]:
            lam = reg * trace[i]
            M = A[i] + lam * np.eye(3)
            x[i] = np.linalg.solve(M, b[i] + lam * mean[i])
            cond[i] = np.linalg.cond(M)
    elif placement != "mean":
        raise ValueError(placement)
    clipped = np.clip(x, 0.0, h)
    out_v = (clipped + lo).astype(np.float32)

    t = cluster[tv].astype(np.int64)
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    if len(t):
        r = np.argmin(t, axis=1)
        t = np.stack([t[np.arange(len(t)), (r + k) % 3] for k in range(3)], -1)
        t = np.unique(t, axis=0)
    info = dict(unclamped=x + lo, clamped=(clipped != x).any(1), cond=cond, trace=trace, lo=lo, mean=mean + lo)
    return Simplified(out_v, t.reshape(-1, 3).astype(np.int64), cluster.astype(np.int32), size.astype(np.int32), info)


def one_step_of(got, want):
    """every entry of fp32 `got` equals `want` or is one fp32 step from it"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(((got == want) | (got == np.nextafter(want, np.float32(np.inf))) |
                 (got == np.nextafter(want, np.float32(-np.inf)))).all())
