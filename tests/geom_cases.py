"""Inputs of the geometry-buffer and depth-error tests (tests/test_geom_cpu.py, tests/test_gpu_geom.py): analytic scenes
with their exact normals, hand-written buffers that plant one rule each, and random depth-error batches. numpy only;
every function returns fresh arrays computed in float64 and rounded to fp32 once."""
import numpy as np


def pinhole_inverse(f, H, W):
    """K^-1 of a pinhole of focal length f with the principal point at the image centre, (3, 3) fp32"""
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float64)
    return np.linalg.inv(K).astype(np.float32)


def _rays(K_inv, H, W, origin=(0.0, 0.0), step=1.0):
    """(H, W, 3) float64 rays K^-1 (x, y, 1) at the pixel centres, from the fp32 matrix the kernel reads"""
    K = np.asarray(K_inv, np.float32).astype(np.float64)
    x = origin[0] + (np.arange(W) + 0.5) * step
    y = origin[1] + (np.arange(H) + 0.5) * step
    pix = np.stack([np.broadcast_to(x[None], (H, W)), np.broadcast_to(y[:, None], (H, W)), np.ones((H, W))], -1)
    return pix @ K.T


def _plane(rays, normal, through):
    """depth along the camera axis of the plane's hit per ray"""
    return float(np.dot(normal, through)) / (rays @ normal)


PLANE_NORMAL = np.array([0.3, -0.2, -0.93]) / np.linalg.norm([0.3, -0.2, -0.93])
SPHERE_CENTRE, SPHERE_RADIUS = np.array([0.05, -0.03, 2.5]), 0.6


def _sphere(rays):
    """(hit (H, W) bool, depth (H, W), unit normal (H, W, 3)) of the sphere; depth 1 and normal 0 where the ray misses"""
    c, R = SPHERE_CENTRE, SPHERE_RADIUS
    dd, dc = (rays * rays).sum(-1), rays @ c
    disc = dc * dc - dd * (c @ c - R * R)
    hit = disc > 0
    t = np.where(hit, (dc - np.sqrt(np.where(hit, disc, 0.0))) / dd, 1.0)
    normal = np.where(hit[..., None], (t[..., None] * rays - c) / R, 0.0)
    return hit, t, normal


def scene(kind, H, W, f=None, origin=(0.0, 0.0), step=1.0):
    """dict of disparity, mask (H, W) fp32, inv_intrinsics (3, 3) fp32, normal (H, W, 3) float64 (the analytic unit
    normal facing the camera, 0 on background) and surface (H, W) bool. kind: "plane" (the tilted plane through
    (0, 0, 3)), "sphere", "sphere_on_plane" (the sphere in front of the plane z = 4) or "empty"."""
    f = f if f is not None else {"plane": 60.0, "sphere_on_plane": 80.0}.get(kind, 1.2 * max(H, W))
    K_inv = pinhole_inverse(f * step, H * step + 2 * origin[1], W * step + 2 * origin[0])
    rays = _rays(K_inv, H, W, origin, step)
    if kind == "plane":
        depth, surface = _plane(rays, PLANE_NORMAL, np.array([0.0, 0.0, 3.0])), np.ones((H, W), bool)
        normal = np.broadcast_to(PLANE_NORMAL, (H, W, 3)).copy()
    elif kind == "empty":
        depth, surface, normal = np.ones((H, W)), np.zeros((H, W), bool), np.zeros((H, W, 3))
    else:
        surface, depth, normal = _sphere(rays)
        if kind == "sphere_on_plane":
            depth = np.where(surface, depth, 4.0)
            normal = np.where(surface[..., None], normal, np.array([0.0, 0.0, -1.0]))
            surface = np.ones((H, W), bool)
    disparity = np.where(surface, 1.0 / depth, 0.0).astype(np.float32)
    return {"disparity": disparity, "mask": surface.astype(np.float32), "inv_intrinsics": K_inv, "normal": normal,
            "surface": surface}


def hand_buffer(n=5):
    """(disparity, mask, inv_intrinsics) of an n x n image, n >= 5: a gently tilted surface near depth 2 with, in its top
    left 5 x 5 pixels, a mask exactly at the threshold 0.5 at (1, 1) (valid, at half the depth: no neighbour within the
    edge), a mask one fp32 step below it at (1, 3), q = 0 at (3, 1), a negative q at (3, 3), a NaN q at (4, 0), an
    infinite q at (4, 4) and a NaN mask at (0, 4)."""
    r, c = np.mgrid[0:n, 0:n]
    q = (0.5 + 0.01 * c + 0.005 * r).astype(np.float32)
    m = np.ones((n, n), np.float32)
    m[1, 1] = 0.5
    m[1, 3] = np.nextafter(np.float32(0.5), np.float32(0))
    q[3, 1], q[3, 3], q[4, 0], q[4, 4] = 0.0, -0.5, np.nan, np.inf
    m[0, 4] = np.nan
    return q, m, pinhole_inverse(4.0, n, n)


HAND_INVALID = [(1, 3), (3, 1), (3, 3), (4, 0), (4, 4), (0, 4)]
# (pixel, which neighbours its differences use with edge = 0.05): lo/hi along c, lo/hi along r; "" = no difference
HAND_DIFFERENCES = {(2, 2): ("lh", "lh"), (0, 0): ("h", "h"), (0, 2): ("lh", "h"), (4, 2): ("lh", "l"), (2, 0): ("h", "lh"),
                    (2, 4): ("l", "lh"), (1, 1): ("", ""), (0, 1): ("lh", ""), (2, 1): ("lh", ""), (2, 3): ("lh", ""),
                    (3, 2): ("", "lh")}


def edge_equality():
    """(disparity, mask, inv_intrinsics, edge) of a 3 x 3 image at depth 1 whose centre has, with edge = 0.25, a left
    neighbour exactly at the limit (depth 0.75: usable) and a right neighbour one fp32 step beyond it (not usable)"""
    q = np.ones((3, 3), np.float32)
    m = np.ones((3, 3), np.float32)
    m[1, 0] = 0.75
    m[1, 2] = np.nextafter(np.float32(0.75), np.float32(0))
    return q, m, pinhole_inverse(3.0, 3, 3), 0.25


def error_batch(shape, seed):
    """(disparity, target, mask) fp32 of `shape`: a target with a background of exact zeros, a generated disparity with
    zeros and negatives of its own, and a soft mask"""
    rng = np.random.default_rng(seed)
    target = rng.uniform(0.1, 0.6, shape) * (rng.uniform(size=shape) < 0.4)
    disparity = (target + rng.normal(0, 0.05, shape)) * (rng.uniform(size=shape) < 0.8)
    mask = rng.uniform(size=shape)
    return disparity.astype(np.float32), target.astype(np.float32), mask.astype(np.float32)
