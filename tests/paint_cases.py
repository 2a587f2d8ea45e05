"""Inputs the CPU and GPU tests of the deferred shading share (tests/test_paint_cpu.py, tests/test_gpu_paint.py): the
33^3 marching-cubes sphere, its cameras, and a hand-written 8 x 8 fragment buffer with every edge case of the contract."""
import functools

import numpy as np

import mc_reference as M

# R -> (img_size, fx, fy, cx, cy): fx != fy, an off-centre principal point, img_size != R (tests/test_gpu_raster.py's)
CAMERAS = {64: (96, 110.0, 90.0, 52.0, 41.0), 257: (128, 150.0, 130.0, 70.0, 58.0)}


def intrinsics(R):
    _, fx, fy, cx, cy = CAMERAS[R]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


@functools.lru_cache(maxsize=None)
def sphere():
    """(vertices (V, 3) fp32 in camera space, triangles (T, 3) int64): radius 14.3 in a 33^3 volume, about 7.7 k triangles"""
    n = 33
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    g = np.meshgrid(x, x, x, indexing="ij")
    v, t = M.marching_cubes((14.3 - np.sqrt(sum(a * a for a in g))).astype(np.float32), 0.0)
    v = (v.astype(np.float64) - (n - 1) / 2) * (0.8 / 14.3) + [0.05, -0.03, 3.0]
    v, t = v.astype(np.float32), t.astype(np.int64)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def sine_colors(vertices):
    """0.5 + 0.5 sin(k x) per channel, k = 7, 11, 13 on x, y, z: (V, 3) fp32 in [0, 1]"""
    v = np.asarray(vertices, np.float64)
    return (0.5 + 0.5 * np.sin(v * [7.0, 11.0, 13.0])).astype(np.float32)


def octant_labels(vertices, centre=(0.05, -0.03, 3.0)):
    """(V,) int32: the octant of the vertex about the centre, every 7th label -1"""
    d = np.asarray(vertices, np.float64) - centre
    lab = ((d[:, 0] > 0) * 1 + (d[:, 1] > 0) * 2 + (d[:, 2] > 0) * 4).astype(np.int32)
    lab[::7] = -1
    return lab


OCTANT_PALETTE = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [0.25, 0.5, 0.75], [0.9, 0.9, 0.9]],
                          np.float32)


def hand_buffer():
    """An 8 x 8 fragment buffer written by hand. V = 6, T = 5, P = 3. Triangle 3 names vertex V, triangle 4 vertex -1.
    Row 0: face ids -1, T, T + 5, a large id, then in range; row 1: the triangles with a vertex outside [0, V);
    row 2: exact barycentric ties; row 3: labels -1 and P at the winning corner; row 4: a zero normal, a normal facing
    away, a NaN barycentric; the rest: random fragments. Returns a dict of the kernel's inputs."""
    rng = np.random.default_rng(5)
    V, T, P, R = 6, 5, 3, 8
    verts = np.array([[-0.4, -0.3, 2.0], [0.5, -0.2, 2.2], [0.1, 0.6, 1.9], [-0.2, 0.1, 2.6], [0.3, 0.3, 3.0], [0.0, -0.5, 2.4]],
                     np.float32)
    tris = np.array([[0, 1, 2], [3, 4, 5], [2, 1, 4], [0, 1, V], [-1, 2, 3]], np.int64)
    labels = np.array([0, 1, 2, -1, P, 1], np.int32)
    palette = np.array([[0.9, 0.1, 0.2], [0.2, 0.8, 0.3], [0.1, 0.3, 1.0]], np.float32)
    colors = rng.uniform(0, 1, (V, 3)).astype(np.float32)
    f = rng.integers(0, 3, (R, R)).astype(np.int64)
    b = rng.uniform(0.05, 1, (R, R, 3))
    b = (b / b.sum(-1, keepdims=True)).astype(np.float32)
    n = rng.normal(0, 1, (R, R, 3))
    n[..., 2] = -np.abs(n[..., 2]) - 0.5                                    # mostly toward the camera at the origin
    n = n.astype(np.float32)
    f[0] = [-1, T, T + 5, 2 ** 40, 0, 1, 2, -7]
    f[1] = [3, 4, 3, 4, 0, 1, 2, 3]
    f[2] = [0, 1, 2, 0, 1, 2, 0, 1]
    ties = [(0.5, 0.5, 0.0), (0.25, 0.25, 0.5), (0.4, 0.4, 0.2), (0.2, 0.4, 0.4), (0.4, 0.2, 0.4), (1 / 3, 1 / 3, 1 / 3),
            (0.0, 0.5, 0.5), (0.5, 0.0, 0.5)]
    b[2] = np.array(ties, np.float32)
    f[3] = [1, 1, 1, 1, 2, 2, 0, 0]                                         # triangle 1 = vertices 3, 4, 5: labels -1, P, 1
    b[3] = np.array([(0.8, 0.1, 0.1), (0.1, 0.8, 0.1), (0.1, 0.1, 0.8), (0.45, 0.45, 0.1), (0.1, 0.1, 0.8), (0.1, 0.8, 0.1),
                     (0.6, 0.3, 0.1), (0.2, 0.2, 0.6)], np.float32)        # triangle 2 = vertices 2, 1, 4: label P at corner 2
    f[4, :3] = [0, 1, 2]
    n[4, 0] = 0.0
    n[4, 1] = [0.0, 0.0, 1.0]
    b[4, 2] = [np.nan, 0.3, 0.7]
    return dict(pix_to_face=f, bary=b, normals=n, vertices=verts, triangles=tris, vertex_colors=colors,
                vertex_labels=labels, palette=palette)
