"""Float64 numpy restatement of libenarf_pose.so's contract (include/enarf_pose.h): the reference's create_mask /
pose_to_image_coord for the SMPL property set after add_blank_part, evaluated element by element in the kernel's order
(no np.matmul, no reductions whose order numpy chooses), so that the kernel can be compared bit for bit."""
import numpy as np

# SMPLProperty (dataset/dataset.py) and HumanPoseDataset.add_blank_part, as the reference states them
IS_BLANK = [0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1]
PREV_SEQ = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 11, 9, 10, 11, 12, 13, 16, 17, 18, 20, 21, 22, 23, 24, 25]
BLANK_IDX = [0, 0] + list(range(10)) + [9, 9] + list(range(10, 24))
VALID_KEYPOINTS = [i for i in range(28) if i not in PREV_SEQ or IS_BLANK[i] == 0]
_GROUP_IDS = [PREV_SEQ[p] if IS_BLANK[p] else p for p in PREV_SEQ if p >= 0]
PART_IDS = sorted(set(_GROUP_IDS))
BONE_GROUP = [PART_IDS.index(g) for g in _GROUP_IDS]              # bone k + 1 -> part group
BONE_A = [BLANK_IDX[k] for k in range(1, 28)]                       # original joint of a, b for bone k + 1
BONE_B = [BLANK_IDX[PREV_SEQ[k]] for k in range(1, 28)]
KEY_JOINT = [BLANK_IDX[k] for k in VALID_KEYPOINTS]
NUM_PARTS, NUM_KEYPOINTS = len(PART_IDS), len(VALID_KEYPOINTS)


def project(pose, K):
    """(24, 2) fp64: (K[r][0] u + K[r][1] v) + K[r][2] w with u, v, w = x / z, y / z, z / z"""
    pose, K = np.asarray(pose, np.float64), np.asarray(K, np.float64)
    x, y, z = pose[:, 0, 3], pose[:, 1, 3], pose[:, 2, 3]
    with np.errstate(all="ignore"):
        u, v, w = x / z, y / z, z / z
        return np.stack([K[r, 0] * u + K[r, 1] * v + K[r, 2] * w for r in (0, 1)], axis=1)


def _max(m, v):
    """np.max's NaN rule, with the strict 'greater replaces' order of the kernel"""
    return np.where((v > m) | np.isnan(v), v, m)


def _ceil_int(v):
    c = np.ceil(v)
    return int(c) if np.isfinite(c) and -2.0 ** 31 <= c <= 2.0 ** 31 - 1 else None


def masks(pose, K, size, thickness, joint_pos=None):
    """One frame: {mask, disparity, part_disparity, keypoint_mask} fp32 and pose_2d fp64"""
    pose = np.asarray(pose, np.float64)
    pos = project(pose, K) if joint_pos is None else np.asarray(joint_pos, np.float64)
    z = pose[:, 2, 3]
    S, t = int(size), float(thickness)
    t2 = t * t
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    any_in = np.zeros((S, S), bool)
    dmax, pmax = None, [None] * NUM_PARTS
    with np.errstate(all="ignore"):
        for k in range(27):
            a, b = pos[BONE_A[k]], pos[BONE_B[k]]
            za, zb = z[BONE_A[k]], z[BONE_B[k]]
            abx, aby = b[0] - a[0], b[1] - a[1]
            abab = abx * abx + aby * aby
            acx, acy = x - a[0], y - a[1]
            acab = acx * abx + acy * aby
            acac = acx * acx + acy * acy
            inside = (0 <= acab) & (acab <= abab) & (acab * acab >= abab * (acac - t2)) & (abab > 1e-8)
            any_in |= inside
            s = acab / (abab + 1e-10)
            sza = s * za
            tt = sza / (sza + (1 - s) * zb)
            zc = za * (1 - tt) + zb * tt
            d = 1 / (zc + 1e-8) * inside.astype(np.float64)
            dmax = d if dmax is None else _max(dmax, d)
            g = BONE_GROUP[k]
            pmax[g] = d if pmax[g] is None else _max(pmax[g], d)
    key = np.zeros((NUM_KEYPOINTS, S, S))
    for i, j in enumerate(KEY_JOINT):
        kx, ky = pos[j]
        bounds = [_ceil_int(v) for v in (kx - t, kx + t, ky - t, ky + t)]
        if any(v is None for v in bounds):
            continue
        left, right, top, bottom = bounds
        key[i, top:bottom, left:right] = float(bottom >= 0 and right >= 0)
    return {"mask": any_in.astype(np.float32), "disparity": dmax.astype(np.float32),
            "part_disparity": np.stack(pmax).astype(np.float32), "keypoint_mask": key.astype(np.float32),
            "pose_2d": pos}


def batch(poses, Ks, size, thickness):
    outs = [masks(p, k, size, thickness) for p, k in zip(poses, Ks)]
    return {name: np.stack([o[name] for o in outs]) for name in outs[0]}


def margin(pose, K, size, thickness, joint_pos=None):
    """(S, S): the smallest |slack| over the bones' four mask inequalities, relative to their magnitude - where a mask
    pixel may differ between two roundings of the same pose"""
    pos = project(pose, K) if joint_pos is None else np.asarray(joint_pos, np.float64)
    S, t2 = int(size), float(thickness) ** 2
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    m = np.full((S, S), np.inf)
    for k in range(27):
        a, b = pos[BONE_A[k]], pos[BONE_B[k]]
        abx, aby = b[0] - a[0], b[1] - a[1]
        abab = abx * abx + aby * aby
        if not abab > 1e-8:
            continue
        acx, acy = x - a[0], y - a[1]
        acab = acx * abx + acy * aby
        acac = acx * acx + acy * acy
        scale = abab * (np.abs(acac) + t2) + acab * acab + 1.0
        for slack in (acab, abab - acab, acab * acab - abab * (acac - t2)):
            m = np.minimum(m, np.abs(slack) / scale)
    return m
