"""Inputs the CPU and GPU tests of the normal maps share (tests/test_nmap_cpu.py, tests/test_gpu_nmap.py,
tests/nmap_poison_cases.py): the meshes and atlas sizes of the encode cases (bake_cases' and paint_cases'), their seeded
vector fields, the normal textures of the hand fragment buffer, and the bounds of the GPU test."""
import functools

import numpy as np

import bake_cases as BC
import bake_reference as BR
import paint_cases as PC

ENCODE_CASES = [(1, 6), (5, 21), (8, 12), "sphere"]
SPHERE_SMALL = 380                 # tests/test_gpu_bake.py's: cell 6, 63 cells a row, a margin of two texels
MIN_LENGTH = 0.25

# the GPU test's bounds. The normal output: two fp32 steps of 1 per component (the referee is float64, the kernel rounds
# once; a unit vector's components are at most 1). The fp32 map: one fp32 step of 1.
NORMAL_BOUND = 2 * 2.0 ** -23
F32_BOUND = 2.0 ** -23


def mesh(case):
    return (PC.sphere(), SPHERE_SMALL) if case == "sphere" else (BC.hand_mesh(case[0]), case[1])


@functools.lru_cache(maxsize=None)
def texel_face(case):
    """(A, A) int32: bake_reference.points' owners (what bake_points writes: tests/test_gpu_bake.py holds it to that)"""
    (v, t), A = mesh(case)
    face = BR.points(v, t, A)["texel_face"]
    face.setflags(write=False)
    return face


@functools.lru_cache(maxsize=None)
def vectors(case):
    """(3, A A) fp32, seeded: unit-ish random vectors, every 11th shorter than MIN_LENGTH, and among the first owned texels
    a NaN, +inf, -inf, an exact zero, and lengths a step on either side of MIN_LENGTH"""
    (v, t), A = mesh(case)
    rng = np.random.default_rng(300 + A)
    g = rng.normal(0, 1, (A * A, 3))
    g[::11] *= 0.05
    own = np.flatnonzero(texel_face(case).reshape(-1) >= 0)
    special = [[np.nan, 0.3, 0.2], [np.inf, 0.1, 0.0], [0.2, -np.inf, 0.1], [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0],
               [MIN_LENGTH, 0.0, 0.0], [0.0, np.nextafter(np.float32(MIN_LENGTH), np.float32(1)), 0.0],
               [0.0, 0.0, np.nextafter(np.float32(MIN_LENGTH), np.float32(0))], [3e38, 3e38, 3e38], [1e-30, 2e-30, 1e-30]]
    for k, s in zip(own[1::2], special):          # every other owned texel: lower and upper halves alike
        g[k] = s
    out = np.ascontiguousarray(g.T.astype(np.float32))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hand_normal_textures(A=16):
    """(RGBA8 (A, A, 4) uint8, fp32 (A, A, 3)) normal textures for the 5 triangles of the hand buffer (cell 8): random; the
    fp32 one has the second cell all zero (a tap there is |q| = 0), a NaN and an inf texel in the first"""
    rng = np.random.default_rng(19)
    u8 = rng.integers(0, 256, (A, A, 4)).astype(np.uint8)
    f32 = rng.normal(0, 1, (A, A, 3)).astype(np.float32)
    f32[0:8, 8:16] = 0
    f32[3, 3, 1] = np.nan
    f32[2, 5, 0] = np.inf
    u8.setflags(write=False)
    f32.setflags(write=False)
    return u8, f32


def rigid_motion(seed=7):
    """(R (3, 3), tau (3,)) float64: a proper rotation by a seeded axis and angle, and a translation"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(0, 1, 3)
    axis /= np.linalg.norm(axis)
    angle = 0.9
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    return R, np.array([0.03, -0.02, 0.1])


CONSTANT_D = np.array([0.36, -0.48, -0.8])          # a unit vector, exact to fp64 rounding
