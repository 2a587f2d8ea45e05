"""Inputs the CPU and GPU tests of the texture atlas share (tests/test_bake_cpu.py, tests/test_gpu_bake.py): the small
(T, A) shapes of the layout, their hand meshes, textures for the hand fragment buffer, and the colour functions."""
import functools

import numpy as np

import paint_cases as PC

# (T, A) -> the cell the layout must give; (9, 12) is unsupported
LAYOUTS = {(1, 6): 6, (5, 16): 8, (5, 21): 10, (8, 12): 6}
UNSUPPORTED = (9, 12)


@functools.lru_cache(maxsize=None)
def hand_mesh(T):
    """(vertices (6, 3) fp32, triangles (T, 3) int64). T = 5 is the mesh of paint_cases.hand_buffer(): triangle 3 names
    vertex V = 6, triangle 4 vertex -1; the others take random vertices in range."""
    h = PC.hand_buffer()
    if T == 5:
        v, t = h["vertices"].copy(), h["triangles"].copy()
    else:
        rng = np.random.default_rng(40 + T)
        v = (h["vertices"] + rng.normal(0, 0.05, h["vertices"].shape)).astype(np.float32)
        t = np.stack([rng.permutation(6)[:3] for _ in range(T)]).astype(np.int64).reshape(T, 3)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def hand_textures(A=16):
    """(RGBA8 (A, A, 4) uint8, fp32 (A, A, 3)) random textures for the 5 triangles of the hand buffer; the fp32 one has
    values outside [0, 1]"""
    rng = np.random.default_rng(9)
    u8 = rng.integers(0, 256, (A, A, 4)).astype(np.uint8)
    f32 = rng.uniform(-0.25, 1.25, (A, A, 3)).astype(np.float32)
    u8.setflags(write=False)
    f32.setflags(write=False)
    return u8, f32


def resolve_inputs(rows=5, A=13, P=3):
    """texel_face (rows, A) int32 with empty texels, colours (3, M) fp32 with NaN, +-inf and values outside [-1, 1], labels
    (M,) int32 with -1 and P, a palette (P, 3)"""
    rng = np.random.default_rng(21)
    M = rows * A
    face = rng.integers(-1, 4, (rows, A)).astype(np.int32)
    face[0, :3] = [-1, 0, -1]
    color = rng.uniform(-1.3, 1.3, (3, M)).astype(np.float32)
    color[:, 1] = [np.nan, np.inf, -np.inf]
    color[:, 4] = [1.0, -1.0, 0.0]
    color[:, 5] = [np.nextafter(np.float32(1), np.float32(0)), 1.5, -1.5]
    color[:, 0] = np.nan                                   # an empty texel: never read
    labels = rng.integers(0, P, M).astype(np.int32)
    labels[[1, 6, 7, 8]] = [-1, P, P + 40, -2 ** 31]
    palette = np.array([[0.9, 0.1, 0.2], [0.2, 0.8, 0.3], [0.1, 0.3, 1.0]], np.float32)[:P]
    return face, color, labels, palette


def face_colors(T):
    """(T, 3) float64: a colour per face on the 1/64 lattice (exact in fp32), any two faces at least 1/64 apart in some
    channel, for T <= 61^3"""
    t = np.arange(T)
    return np.stack([(t % 61) + 1, ((t // 61) % 61) + 1, ((t // 3721) % 61) + 1], -1) / 64.0


def affine_color(points):
    """an affine function of position with values in [0, 1] around the sphere of paint_cases: (M, 3) float64"""
    p = np.asarray(points, np.float64)
    G, o = affine_gradient()
    return p @ G.T + o


def affine_gradient():
    G = np.array([[0.30, -0.10, 0.05], [0.08, 0.25, -0.12], [-0.07, 0.11, 0.28]])
    o = np.array([0.5, 0.5, 0.5]) - G @ np.array([0.05, -0.03, 3.0])
    return G, o


# paint_cases.sine_colors(points * SINE_SCALE) has the wavelengths 2 pi / (7, 11, 13) / SINE_SCALE = 0.112, 0.071, 0.060:
# near the edge length of the 33^3 sphere, whose lattice step is 0.8 / 14.3 = 0.056
SINE_SCALE = 8.0


def fine_sine(points):
    """(M, 3) fp32 in [0, 1]"""
    return PC.sine_colors(np.asarray(points, np.float64) * SINE_SCALE)
