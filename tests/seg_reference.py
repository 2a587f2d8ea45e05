"""Referee of libenarf_seg.so, built on the oracle's functions (oracle/enarf_oracle.py).

Validity and canonical coordinates come from O.to_local_and_canonical and O.validity in fp32: the bit-exact contract the
parity tests hold the query and march kernels to. The part weights come from O.part_prob in float64 at those fp32
coordinates; labels, top, second, the composite and the part map follow in float64 (numpy: argmax returns the first of
equal maxima, which is the lowest part index).

The ambiguity rule. The kernels evaluate the part weights in fp32 with the hardware exp2 and reciprocal; the project's
parity bound is 1e-4 of an output's scale, and part weights have scale <= 1. Two weights that differ by no more than
twice that bound (AMBIGUITY = 2e-4) can change order inside the bound, so
  * a sample is ambiguous when its two largest referee weights differ by at most AMBIGUITY;
  * a ray is ambiguous when its two largest part masses differ by at most AMBIGUITY plus the compositing weight its
    ambiguous samples carry (each such sample may move its whole weight from one part's mass to another's).
Labels and part maps are compared on the unambiguous samples and rays only, and the ambiguous ones are capped:
MAX_AMBIGUOUS_SAMPLES of the samples with two or more valid parts, MAX_AMBIGUOUS_RAYS of the labelled rays.
"""
import numpy as np
import torch

from oracle import enarf_oracle as O

PLANE_CH = 96
AMBIGUITY = 2e-4
MAX_AMBIGUOUS_SAMPLES = 0.01
MAX_AMBIGUOUS_RAYS = 0.05


def validity_and_weights(points, pose_scaled, scale, cpose, tri_plane, clamp_mask=False, uniform_part_weight=False):
    """points (B, 3, N) fp32 in the scaled camera space -> (valid (B, P, N) bool, weight (B, P, N) float64 numpy)"""
    points = points.to(torch.float32)
    B, P = pose_scaled.shape[:2]
    local, canonical = O.to_local_and_canonical(points, pose_scaled, scale, cpose)
    valid = O.validity(local, canonical)
    if uniform_part_weight:
        w = torch.full(valid.shape, 1.0 / P, dtype=torch.float64)
    else:
        planes = tri_plane[:, PLANE_CH:].double()
        if planes.shape[0] == 1 and B > 1:
            planes = planes.expand(B, -1, -1, -1)
        w = O.part_prob(planes, canonical.double(), valid, clamp_mask=clamp_mask)
    return valid, w.numpy()


def labels_from_weights(valid, weight):
    """valid (B, P, N) bool, weight (B, P, N) float64 -> dict of numpy arrays, each (B, N): label int32 (-1: no valid
    part; the lowest index among equal maxima), top and second float64 (0 / -1 as include/enarf_seg.h), n_valid, and
    ambiguous bool"""
    v = valid.numpy() if isinstance(valid, torch.Tensor) else np.asarray(valid)
    w = np.where(v, np.asarray(weight, dtype=np.float64), -np.inf)
    n_valid = v.sum(axis=1)
    label = np.argmax(w, axis=1)
    top = np.take_along_axis(w, label[:, None], axis=1)[:, 0]
    rest = w.copy()
    np.put_along_axis(rest, label[:, None], -np.inf, axis=1)
    second = rest.max(axis=1)
    gap = np.where(n_valid > 1, top, 1.0) - np.where(n_valid > 1, second, 0.0)
    return {"label": np.where(n_valid > 0, label, -1).astype(np.int32),
            "top": np.where(n_valid > 0, top, 0.0),
            "second": np.where(n_valid > 1, second, -1.0),
            "n_valid": n_valid,
            "ambiguous": (n_valid > 1) & (gap <= AMBIGUITY)}


def labels(points, pose_scaled, scale, cpose, tri_plane, clamp_mask=False, uniform_part_weight=False):
    """the referee's labels of points (B, 3, N): labels_from_weights' dict plus `valid` (B, P, N) bool (torch)"""
    valid, w = validity_and_weights(points, pose_scaled, scale, cpose, tri_plane, clamp_mask, uniform_part_weight)
    out = labels_from_weights(valid, w)
    out["valid"] = valid
    return out


def ray_points(image_coord, inv_intrinsics, depth_min, depth_max, bins):
    """the fine points of a march, (B, 3, n * Nf) fp32, formed as the oracle's render() forms them (O.ray_directions,
    O.coarse_points' start / end, O.fine_points)"""
    rd = O.ray_directions(image_coord.to(torch.float32), inv_intrinsics.to(torch.float32))
    start, end = depth_min[:, None] * rd, depth_max[:, None] * rd
    _, pts = O.fine_points(bins.to(torch.float32), depth_min, depth_max, start, end)
    return pts.reshape(pts.shape[0], 3, -1)


def composite(sample_labels, fine_weights, palette, ambiguous_samples=None):
    """labels (B, n, Nf) int, fine_weights (B, n, Nf - 1) or (B, 1, n, Nf - 1), palette (P, 3) -> dict of numpy arrays:
    color (B, 3, n), part_mass (B, n) float64, part_map (B, n) int32, labelled (B, n) bool (the ray has a labelled sample
    of positive weight) and ambiguous (B, n) bool. The last fine sample carries no weight. `ambiguous_samples` (B, n, Nf)
    bool marks the samples whose label is ambiguous."""
    lab = np.asarray(sample_labels)[..., :-1].astype(np.int64)
    B, n, m = lab.shape
    w = np.asarray(fine_weights, dtype=np.float64).reshape(B, n, m)
    pal = np.asarray(palette, dtype=np.float64)
    P = pal.shape[0]
    lab = np.where((lab >= 0) & (lab < P), lab, -1)
    mass = np.zeros((B, n, P))
    for k in range(P):
        mass[..., k] = np.where(lab == k, w, 0.0).sum(axis=-1)
    color = np.einsum("bnk,kc->bcn", mass, pal)
    best = mass.max(axis=-1)
    labelled = best > 0
    part_map = np.where(labelled, np.argmax(mass, axis=-1), -1).astype(np.int32)
    srt = np.sort(mass, axis=-1)
    runner = srt[..., -2] if P > 1 else np.zeros_like(best)
    slack = np.zeros_like(best)
    if ambiguous_samples is not None:
        slack = np.where(np.asarray(ambiguous_samples)[..., :-1] & (lab >= 0), np.abs(w), 0.0).sum(axis=-1)
    return {"color": color, "part_mass": np.where(labelled, best, 0.0), "part_map": part_map, "labelled": labelled,
            "ambiguous": labelled & (best - runner <= AMBIGUITY + slack)}


def bits(valid):
    """(B, P, N) bool -> (B, N) uint32 bit masks, bit k = part k"""
    from _helpers import bits_of
    return bits_of(valid)


def lowest_set_bit(b):
    """(…) uint32 bit masks -> the index of the lowest set bit, -1 for 0"""
    b = np.asarray(b).astype(np.uint32).astype(np.int64)
    low = b & -b
    return np.where(b != 0, np.log2(np.maximum(low, 1)).astype(np.int64), -1).astype(np.int32)
