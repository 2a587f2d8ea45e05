"""Referees of libenarf_nrm.so (include/enarf_nrm.h). No GPU, nothing of the product.

ray_normals: a plain-numpy float64 restatement of enarf_nrm_ray_normals - the composite G = sum_i w_i g_i over the first
Nf - 1 samples in ascending order, the validity rule, the fallback and both shades (the formulas and constants of
tests/geom_reference.py's `buffers`). It takes the fp32 values the kernel takes, rounds the scalars to fp32 as the argument
structure does, and works from nothing else. `wrong` plants one of three bugs a kernel could have, for the referee's own
sensitivity test (tests/test_nrm_cpu.py).

gradient_referee: d sum(density) / d points from tests/pgrad_reference.py's Referee with gd = ones and gc = None - the
definition of enarf_nrm_field_gradient's output; no autograd code of its own.

ray_case: the seeded inputs the GPU test and the sensitivity test share."""
import numpy as np
import torch

import geom_reference as GR
import pgrad_reference as PR

FLAG_VALID, FLAG_NORMAL, FLAG_FIELD = 1, 2, 4
RAY_CASES = ((1, 2), (64, 3), (65, 33), (300, 64), (64, 128))      # (n, Nf), B = 2
WRONG = ("shifted_weights", "includes_last_sample", "no_minus_sign")


def ray_normals(gradient, weights, mask, fallback=None, flags=None, points=None, shade=None, mask_threshold=0.5,
                min_gradient=0.0, background=1.0, wrong=None):
    """dict of normals (B, n, 3) float64, flags (B, n) uint8, magnitude (B, n) float64 and image (B, n, 3) uint8 or None.
    gradient (B, 3, n Nf), weights (B, n, Nf - 1), mask (B, n), fallback (B, n, 3) with flags (B, n) uint8, points (B, n, 3)."""
    g32, w32, m32 = np.asarray(gradient, np.float32), np.asarray(weights, np.float32), np.asarray(mask, np.float32)
    B, n = m32.shape
    Nf = w32.shape[-1] + 1
    g = g32.astype(np.float64).reshape(B, 3, n, Nf)
    w = w32.astype(np.float64).reshape(B, n, Nf - 1)
    steps = range(Nf - 1)
    if wrong == "shifted_weights":                         # weight i taken for sample i + 1
        g = g[..., 1:]
    elif wrong == "includes_last_sample":                  # Nf weights read from rows of Nf - 1: the last is the next ray's first
        flat = np.concatenate([w.reshape(-1), [0.0]])
        w = np.stack([flat[np.arange(B * n) * (Nf - 1) + i] for i in range(Nf)], -1).reshape(B, n, Nf)
        steps = range(Nf)
    G = np.zeros((B, n, 3))
    with np.errstate(all="ignore"):
        for i in steps:                                    # ascending i, one rounding a product and a sum
            for k in range(3):
                G[..., k] = G[..., k] + w[..., i] * g[:, k, :, i]
        m = np.sqrt((G[..., 0] * G[..., 0] + G[..., 1] * G[..., 1]) + G[..., 2] * G[..., 2])
        field = (m32 >= np.float32(mask_threshold)) & (m > GR._f(min_gradient)) & (m < np.inf)
        sign = 1.0 if wrong == "no_minus_sign" else -1.0
        N = np.where(field[..., None], sign * G / np.where(field, m, 1.0)[..., None], 0.0)
        fin = np.zeros((B, n), np.uint8) if flags is None else np.asarray(flags, np.uint8).reshape(B, n)
        fall = ~field & ((fin & FLAG_NORMAL) > 0) & (fallback is not None)
        if fallback is not None:
            N = np.where(fall[..., None], np.asarray(fallback, np.float32).astype(np.float64).reshape(B, n, 3), N)
        out_flags = ((fin & ~np.uint8(FLAG_FIELD)) | (field.astype(np.uint8) * FLAG_FIELD)).astype(np.uint8)
        image = None
        if shade is not None:
            has = field | fall
            v = np.empty((B, n, 3))
            v[:] = np.broadcast_to(np.asarray(background, np.float32).astype(np.float64), (3,))
            if shade == "normal":
                rgb = np.stack([0.5 + 0.5 * N[..., 0], 0.5 + 0.5 * -N[..., 1], 0.5 + 0.5 * -N[..., 2]], -1)
                v = np.where(has[..., None], rgb, v)
            else:
                p = np.asarray(points, np.float32).astype(np.float64).reshape(B, n, 3)
                dp = np.maximum(np.sqrt(GR._dot(p, p)), 1e-6)
                c = -GR._dot(N, p) / dp
                spec = np.where(c > 0, np.maximum(2.0 * c * c - 1.0, 0.0), 0.0)
                for _ in range(6):
                    spec = spec * spec
                grey = (0.5 + 0.3 * np.where(c > 0, c, 0.0)) + 0.2 * spec
                v = np.where(has[..., None], grey[..., None], v)
            image = np.floor(255.0 * np.clip(np.nan_to_num(v, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)).astype(np.uint8)
    return {"normals": N, "flags": out_flags, "magnitude": m, "image": image}


def ray_case(n, Nf, B=2, seed=0):
    """Seeded inputs of one ray case as fp32 / uint8 numpy arrays. Ray r of image b is of kind (r + 2 b) % 5: 0 and 4 plain,
    1 all-zero weights, 2 a zero gradient, 3 a mask below the threshold 0.5 (0.1 against 0.9). A fallback with flags drawn
    from {0, 1, 3} (bit 1 set or clear) rides on every ray. Plain rays have |G| of order 1 and the others exactly 0, so
    with min_gradient = 0 no ray is borderline."""
    rng = np.random.default_rng(1000 * n + Nf + seed)
    kind = (np.arange(n)[None] + 2 * np.arange(B)[:, None]) % 5
    w = rng.uniform(0.01, 1.0, (B, n, Nf - 1)).astype(np.float32) / np.float32(Nf - 1)
    g = (rng.standard_normal((B, 3, n, Nf)) + np.array([0.5, -1.0, 2.0])[None, :, None, None]).astype(np.float32) * 5
    w[kind == 1] = 0
    g[np.broadcast_to((kind == 2)[:, None], (B, 3, n))] = 0
    mask = np.where(kind == 3, 0.1, 0.9).astype(np.float32)
    fb = rng.standard_normal((B, n, 3))
    fb = (fb / np.linalg.norm(fb, axis=-1, keepdims=True)).astype(np.float32)
    flags = rng.choice(np.array([0, 1, 3], np.uint8), (B, n))
    points = (rng.uniform(-1, 1, (B, n, 3)) + np.array([0, 0, 3.0])).astype(np.float32)
    return dict(gradient=g.reshape(B, 3, n * Nf), weights=w, mask=mask, fallback=fb, flags=flags, points=points, kind=kind)


def gradient_referee(sc, pts, mode):
    """(the pgrad Referee of the scene's points in `mode`, the all-ones upstream (B, N) whose g_points is the gradient):
    referee.grads(ones, None, n) is what PR.check holds enarf_nrm_field_gradient's output to on the first n points."""
    ref = PR.Referee(sc, pts, mode)
    return ref, torch.ones(pts.shape[0], pts.shape[2])
