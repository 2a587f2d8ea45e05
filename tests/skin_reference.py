"""Referee of libenarf_skin.so, built on tests/seg_reference.py and the oracle's functions (oracle/enarf_oracle.py).

Weights. Validity and the local and canonical coordinates come from the oracle in fp32 (seg_reference.validity_and_weights,
O.to_local_and_canonical): the bit-exact contract the parity tests hold the query and march kernels to. The raw part weights
come from O.part_prob in float64 at those fp32 coordinates. The K kept parts are the K largest raw weights among the valid
parts, by descending weight, the lower part index first among equals (a stable sort of the negated weights); the normalised
weights are the kept raw weights over their sum S, kept_mass is S over the sum of all valid raw weights (1 when at most K
parts are valid), unused slots hold joint -1 and weight 0. A vertex no part contains follows the part with the smallest
max |local| over the three axes of the oracle's fp32 local coordinates (the lowest index on a tie): joint slot 0, weight 1,
kept_mass 0; those coordinates are bit-exact, so this choice is exactly reproducible.

The ambiguity rule. The kernel evaluates the raw weights in fp32 with the hardware exp2 and reciprocal; the project's parity
bound is 1e-4 of an output's scale, and part weights have scale <= 1. A vertex is *ambiguous* when both of these hold:
  * more than K parts are valid;
  * its K-th and (K+1)-th largest referee raw weights differ by at most seg_reference.AMBIGUITY = 2e-4 (twice the bound).
Only there may the kept set differ from the referee's. Everywhere else the kept set is the referee's; the order among
near-equal kept weights may still differ, so (joints, weights) are compared after `dense` scatters them into a (V, P)
vector. Ambiguous vertices are capped at MAX_AMBIGUOUS of the vertices with more than K valid parts.

Posing. Float64 linear-blend skinning from the records and the stored weights as given (fp32 in the GPU tests), in the
operation order include/enarf_skin.h states: rho = sA / sB, L = rho (RB RA^T), t = tB / cs - L (tA / cs), and the blend
accumulated in slot order, slots with joint -1 skipped.
"""
import numpy as np
import torch

import seg_reference as SR
from oracle import enarf_oracle as O

AMBIGUITY = SR.AMBIGUITY
MAX_AMBIGUOUS = 0.01


def scene_points(sc, per=200, half=0.6, seed=5):
    """the points of the scene tests: `per` points a part, uniform in +-half around each scaled part translation:
    (1, 3, P per) fp32 in the scaled camera space"""
    g = torch.Generator().manual_seed(seed)
    centres = sc.pose_scaled[0, :, :3, 3]
    p = centres[:, None, :] + (torch.rand(sc.P, per, 3, generator=g) * 2 - 1) * half
    return p.reshape(-1, 3).t()[None].contiguous()


def weights(points, pose_scaled, scale, cpose, tri_plane, K, clamp_mask=False, uniform_part_weight=False):
    """points (1, 3, N) fp32 in the scaled camera space -> dict of numpy arrays: joints (N, K) int32, weights, raw (N, K)
    float64 (raw: the kept raw weights, 0 in unused slots), kept_sum, kept_mass (N,) float64, n_valid (N,), valid (P, N)
    bool, unowned (N,) bool, fallback (N,) int32 (the nearest part, meaningful where unowned), ambiguous (N,) bool"""
    points = points.to(torch.float32)
    valid_t, w = SR.validity_and_weights(points, pose_scaled, scale, cpose, tri_plane, clamp_mask, uniform_part_weight)
    assert valid_t.shape[0] == 1, "one identity"
    valid, w = valid_t[0].numpy(), np.asarray(w[0], np.float64)            # (P, N)
    P, N = valid.shape
    local, _ = O.to_local_and_canonical(points, pose_scaled, scale, cpose)
    reach = local[0].abs().amax(dim=1).numpy()                              # (P, N) fp32
    fallback = np.argmin(reach, axis=0).astype(np.int32)                    # the first of equal minima: the lowest index
    wv = np.where(valid, w, -np.inf)
    order = np.argsort(-wv, axis=0, kind="stable")                          # descending, the lower index first among equals
    srt = np.take_along_axis(wv, order, axis=0)
    n_valid = valid.sum(axis=0)
    Kp = min(K, P)
    joints = np.full((N, K), -1, np.int32)
    raw = np.zeros((N, K))
    used = np.arange(Kp)[None, :] < np.minimum(n_valid, Kp)[:, None]
    joints[:, :Kp] = np.where(used, order[:Kp].T, -1)
    raw[:, :Kp] = np.where(used, srt[:Kp].T, 0.0)
    kept_sum = raw.sum(axis=1)
    total = np.where(valid, w, 0.0).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = np.where(joints >= 0, raw / kept_sum[:, None], 0.0)
        mass = np.where(n_valid <= K, 1.0, kept_sum / total)
    unowned = n_valid == 0
    joints[unowned, 0] = fallback[unowned]
    norm[unowned, 0] = 1.0
    mass = np.where(unowned, 0.0, mass)
    ambiguous = np.zeros(N, bool)
    if P > K:
        with np.errstate(invalid="ignore"):                                 # -inf - -inf where fewer than K parts are valid
            ambiguous = (n_valid > K) & (srt[K - 1] - srt[K] <= AMBIGUITY)
    return {"joints": joints, "weights": norm, "raw": raw, "kept_sum": kept_sum, "kept_mass": mass, "n_valid": n_valid,
            "valid": valid, "unowned": unowned, "fallback": fallback, "ambiguous": ambiguous}


def dense(joints, weights, P):
    """(V, K) joints and weights -> (V, P) float64: the weight of every part, 0 where it is not kept"""
    joints, weights = np.asarray(joints), np.asarray(weights, np.float64)
    out = np.zeros((joints.shape[0], P))
    for j in range(joints.shape[1]):
        rows = np.nonzero(joints[:, j] >= 0)[0]
        np.add.at(out, (rows, joints[rows, j]), weights[rows, j])
    return out


def records(pose, bone_length, canonical_bone_length=None, coordinate_scale=1.0):
    """(B, P, 4, 4) part frames with unscaled translation and (B, P) or (B, P, 1) bone lengths -> (B, P, 16) records in the
    layout of ops.prepare, in the dtype of `pose` (numpy): R row-major, t cs, cbl / bl / cs"""
    pose = np.asarray(pose)
    B, P = pose.shape[:2]
    bl = np.asarray(bone_length, pose.dtype).reshape(-1, P)
    cbl = np.ones(P, pose.dtype) if canonical_bone_length is None else np.asarray(canonical_bone_length, pose.dtype).reshape(P)
    rec = np.zeros((B, P, 16), pose.dtype)
    rec[:, :, :9] = pose[:, :, :3, :3].reshape(B, P, 9)
    rec[:, :, 9:12] = pose[:, :, :3, 3] * pose.dtype.type(coordinate_scale)
    rec[:, :, 12] = cbl[None] / bl / pose.dtype.type(coordinate_scale)
    return rec


def transforms(parts_rest, parts, coordinate_scale=1.0):
    """rest (1, P, 16) and target (F, P, 16) records -> (L (F, P, 3, 3), t (F, P, 3)) float64, M v = L v + t"""
    A = np.asarray(parts_rest, np.float64).reshape(-1, 16)
    B = np.asarray(parts, np.float64)
    cs = float(coordinate_scale)
    rho = A[None, :, 12] / B[:, :, 12]
    RA, RB = A[:, :9].reshape(-1, 3, 3), B[:, :, :9].reshape(B.shape[0], -1, 3, 3)
    ta, tb = A[:, 9:12] / cs, B[:, :, 9:12] / cs
    L = np.empty(RB.shape)
    for r in range(3):
        for c in range(3):
            L[:, :, r, c] = rho * ((RB[:, :, r, 0] * RA[None, :, c, 0] + RB[:, :, r, 1] * RA[None, :, c, 1])
                                   + RB[:, :, r, 2] * RA[None, :, c, 2])
    t = tb - ((L[..., 0] * ta[None, :, None, 0] + L[..., 1] * ta[None, :, None, 1]) + L[..., 2] * ta[None, :, None, 2])
    return L, t


def pose(vertices, joints, weights, parts_rest, parts, coordinate_scale=1.0):
    """float64 linear-blend skinning: (F, V, 3)"""
    v = np.asarray(vertices, np.float64)
    joints, w = np.asarray(joints), np.asarray(weights, np.float64)
    L, t = transforms(parts_rest, parts, coordinate_scale)
    P = L.shape[1]
    out = np.zeros((L.shape[0],) + v.shape)
    for j in range(joints.shape[1]):
        k = joints[:, j]
        use = (k >= 0) & (k < P)
        kk = np.where(use, k, 0)
        Lj, tj = L[:, kk], t[:, kk]                                          # (F, V, 3, 3), (F, V, 3)
        moved = ((Lj[..., 0] * v[None, :, None, 0] + Lj[..., 1] * v[None, :, None, 1]) + Lj[..., 2] * v[None, :, None, 2]) + tj
        out += np.where(use[None, :, None], w[None, :, j, None] * moved, 0.0)
    return out
