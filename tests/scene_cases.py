"""Inputs of the scene-compositing tests (tests/test_scene_cpu.py, tests/test_gpu_scene.py): seeded sample lists of K
avatars on n rays with hand-planted rays. Everything is fp32 numpy in the library's layouts: depth, density (F, K, n, Nf),
color (F, K, 3, n, Nf), valid (F, K, n) uint8. The arrays are shared and read-only."""
import functools

import numpy as np

# (K, Nf, n, F): one segment; two avatars of one segment; M = 15; M = 65, one past a wavefront; a usual march; M = 512 with
# many avatars; M = 512 with long lists
SHAPES = ((1, 2, 1, 1), (2, 2, 67, 2), (3, 5, 67, 1), (5, 13, 67, 2), (4, 64, 67, 1), (8, 64, 67, 2), (4, 128, 1, 2))

# what is planted on ray r of a frame with n = 67 (frame 1 shifts the list by 5 rays); the other rays are interleaved
# ranges with random validity bytes
PLANTED = ("interleaved", "disjoint", "tied_lists", "repeated", "inversion", "zero_density", "opaque_start", "one_invalid",
           "all_invalid", "nan_depth", "negative_density", "zero_depth", "dropped")


def _lists(rs, K, Nf, lo, hi):
    """ascending depths of K avatars, avatar k inside [lo[k], hi[k]]"""
    u = np.sort(rs.uniform(0.0, 1.0, size=(K, Nf)), axis=-1)
    return (lo[:, None] + (hi - lo)[:, None] * u).astype(np.float32)


def planted_ray(kind, K, Nf, rs):
    """(depth (K, Nf), density (K, Nf), color (K, 3, Nf), valid (K,)) of one ray of the named kind"""
    near = rs.uniform(2.0, 2.5, size=K)
    d = _lists(rs, K, Nf, near, near + rs.uniform(0.5, 1.5, size=K))              # overlapping ranges: interleaved lists
    s = np.exp(rs.uniform(-3.0, 3.0, size=(K, Nf))).astype(np.float32)
    s[rs.uniform(size=(K, Nf)) < 0.2] = 0.0
    c = rs.uniform(-1.0, 1.0, size=(K, 3, Nf)).astype(np.float32)
    v = np.ones(K, np.uint8)
    if kind == "disjoint":
        lo = 2.0 + np.arange(K, dtype=np.float64)[rs.permutation(K)]
        d = _lists(rs, K, Nf, lo, lo + 0.8)
    elif kind == "tied_lists":                              # every breakpoint of avatar 0 tied with one of the last avatar
        d[K - 1] = d[0]
    elif kind == "repeated":
        for k in range(K):
            i = int(rs.randint(0, Nf - 1))
            d[k, i + 1:min(i + 3, Nf)] = d[k, i]
    elif kind == "inversion":                               # one step down: the running maximum closes an empty interval
        for k in range(K):
            i = int(rs.randint(0, Nf - 1))
            d[k, i + 1] = np.nextafter(d[k, i], np.float32(0))
    elif kind == "zero_density":
        s[:] = 0.0
    elif kind == "opaque_start":                            # tau of the first segment > 745: exp(-tau) is exactly 0
        k, first = int(np.argmin(d[:, 0])), np.sort(d.reshape(-1))[:2]
        d[k, 0] = first[0]
        if first[1] - first[0] < 1e-3:                      # keep the first segment long enough
            d[k, 0] = np.float32(first[1] - 1e-2)
        s[k, 0] = 1e7
    elif kind == "one_invalid":
        v[0] = 0
    elif kind in ("all_invalid", "dropped"):
        v[:] = 0
        if kind == "dropped":                               # what the march leaves on a ray it drops: zeros, and no bit set
            d[:], s[:], c[:] = 0.0, 0.0, 0.0
    elif kind == "nan_depth":
        d[K - 1, Nf // 2] = np.nan
    elif kind == "negative_density":
        s[0, Nf - 1] = -1e-3
    elif kind == "zero_depth":
        d[min(1, K - 1), 0] = 0.0
    return d, s, c, v


SKIPPED_BIT = {"nan_depth": lambda K: 1 << (K - 1), "negative_density": lambda K: 1, "zero_depth": lambda K: 1 << min(1, K - 1)}


def kind_of(r, f, n):
    """what is planted on ray r of frame f"""
    if n < len(PLANTED):
        return "interleaved"
    i = r - 5 * f
    return PLANTED[i] if 0 <= i < len(PLANTED) else "random_validity"


@functools.lru_cache(maxsize=None)
def case(K, Nf, n, F, seed=0):
    """(depth, density, color, valid) of a whole call, read-only"""
    rs = np.random.RandomState(1000 * K + 10 * Nf + n + F + seed)
    depth, density = np.zeros((F, K, n, Nf), np.float32), np.zeros((F, K, n, Nf), np.float32)
    color, valid = np.zeros((F, K, 3, n, Nf), np.float32), np.zeros((F, K, n), np.uint8)
    for f in range(F):
        for r in range(n):
            kind = kind_of(r, f, n)
            d, s, c, v = planted_ray(kind, K, Nf, rs)
            if kind == "random_validity":
                v = (rs.uniform(size=K) < 0.7).astype(np.uint8)
            depth[f, :, r], density[f, :, r], color[f, :, :, r], valid[f, :, r] = d, s, c, v
    for a in (depth, density, color, valid):
        a.setflags(write=False)
    return depth, density, color, valid


def two_apart(Nf=6, seed=3):
    """two avatars with disjoint depth ranges on one ray, avatar 1 in front: (depth, density, color) of (2, Nf), (2, 3, Nf)"""
    rs = np.random.RandomState(seed)
    d = _lists(rs, 2, Nf, np.array([4.0, 2.0]), np.array([5.0, 3.0]))
    s = np.exp(rs.uniform(-1.0, 2.0, size=(2, Nf))).astype(np.float32)
    c = rs.uniform(-1.0, 1.0, size=(2, 3, Nf)).astype(np.float32)
    return d, s, c
