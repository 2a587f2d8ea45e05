"""numpy restatement of the contract of include/enarf_anim.h, generic in the dtype: float64 is the referee of the
kernels and of the reference's recorded outputs (tests/golden/pose_interp.npz), np.longdouble measures the referee's own
rounding. No scipy: the slerp is written out as the header writes it.

The tolerance rule of the animation tests: for each input, d = the largest absolute difference between
the float64 and the longdouble run of this restatement on that input; the reference's recording on the CPU and the
kernel's fp64 output on the GPU must lie within FACTOR * d of the float64 run."""
import numpy as np

SMPL_PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21])
FACTOR = 16


def quat(M, dt):
    """unit quaternion (x, y, z, w) by Shepperd's largest-of-four choice; the sign of w is left as it falls"""
    M = M.astype(dt)
    tr = (M[0, 0] + M[1, 1]) + M[2, 2]
    c = int(np.argmax([M[0, 0], M[1, 1], M[2, 2], tr]))
    q = np.zeros(4, dt)
    if c == 3:
        q[0], q[1], q[2], q[3] = M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1], 1 + tr
    else:
        i = c
        j = (i + 1) % 3
        k = (j + 1) % 3
        q[i] = (1 - tr) + 2 * M[i, i]
        q[j] = M[j, i] + M[i, j]
        q[k] = M[k, i] + M[i, k]
        q[3] = M[k, j] - M[j, k]
    return q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], q.dtype)


def slerp(q0, q1, alpha):
    dt = q0.dtype
    d = qmul(q0 * np.array([-1, -1, -1, 1], dt), q1)
    if d[3] < 0:
        d = -d
    s = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if s == 0:
        return q0
    angle = 2 * np.arctan2(s, d[3])
    h = alpha * angle / 2
    return qmul(q0, np.array([d[0] / s * np.sin(h), d[1] / s * np.sin(h), d[2] / s * np.sin(h), np.cos(h)], dt))


def inv_rigid(M):
    o = np.eye(4, dtype=M.dtype)
    o[:3, :3] = M[:3, :3].T
    o[:3, 3] = -(M[:3, :3].T @ M[:3, 3])
    return o


def clocks(i, K, num, loop, dt):
    """(rotation segment, alpha, translation segment, beta) of frame i"""
    S = K if loop else K - 1
    per = num // S
    t = dt(i) * dt(K) / dt(num) if loop else dt(i) * dt(K - 1) / dt(num - 1)
    s = min(int(np.floor(t)), S - 1)
    r = i % per
    beta = dt(r) / dt(per) if loop else (dt(r) / dt(per - 1) if per > 1 else dt(0))
    return s, t - dt(s), i // per, beta


def interpolate_pose(P, parents, num, loop, dt=np.float64, orbit=None):
    """(num, J, 4, 4) in dtype dt; ValueError where the reference's concatenate fails"""
    P = np.asarray(P).astype(dt)
    K, J = P.shape[:2]
    S = K if loop else K - 1
    if S < 1 or num < 1 or num % S or (not loop and num < 2):
        raise ValueError("num is not a multiple of the segments")
    loc = np.zeros_like(P)
    for k in range(K):
        for j in range(J):
            loc[k, j] = P[k, j] if parents[j] < 0 else inv_rigid(P[k, parents[j]]) @ P[k, j]
    out = np.zeros((num, J, 4, 4), dt)
    for i in range(num):
        s, alpha, u, beta = clocks(i, K, num, loop, dt)
        for j in range(J):
            q = slerp(quat(loc[s, j, :3, :3], dt), quat(loc[(s + 1) % K, j, :3, :3], dt), alpha)
            L = np.eye(4, dtype=dt)
            L[:3, :3] = qmat(q)
            t0, t1 = loc[u, j, :3, 3], loc[(u + 1) % K, j, :3, 3]
            L[:3, 3] = t0 + (t1 - t0) * beta
            out[i, j] = L if parents[j] < 0 else out[i, parents[j]] @ L
    if orbit is not None:
        out = rotate_pose(out, rotation_matrix(np.asarray(orbit).astype(dt)))
    return out


def rotation_matrix(theta):
    """the reference's rotation_matrix: (B,) angles about the y axis -> (B, 4, 4)"""
    theta = np.asarray(theta)
    c, s, z, o = np.cos(theta), np.sin(theta), np.zeros_like(theta), np.ones_like(theta)
    return np.stack([c, z, -s, z, z, o, z, z, s, z, c, z, z, z, z, o], axis=-1).reshape(-1, 4, 4)


def rotate_pose(pose, R):
    """the reference's rotate_pose in pose's dtype: R (pose - C) + C, C the mean joint translation as a 4 x 4"""
    dt = pose.dtype
    total = np.zeros((pose.shape[0], 3), dt)
    for j in range(pose.shape[1]):
        total = total + pose[:, j, :3, 3]
    center = np.zeros((pose.shape[0], 1, 4, 4), dt)
    center[:, 0, :3, 3] = total / dt.type(pose.shape[1])
    return np.matmul(R[:, None].astype(dt), pose - center) + center


def rotate_mesh(pose, vertices, angle):
    """the reference's rotate_mesh_by_angle on the vertices, in pose's dtype: pose (1, J, 4, 4), vertices (V, 3)"""
    dt = pose.dtype
    center = pose[0, :, :3, 3:].mean(axis=0)
    R = rotation_matrix(np.asarray(angle).astype(dt))
    return (R[0, :3, :3] @ (vertices.astype(dt).T - center) + R[0, :3, 3:] + center).T


def bone_length(poses, parents):
    """(num, J - 1, 1) in poses' dtype"""
    t = poses[:, :, :3, 3]
    d = t[:, 1:] - t[:, np.asarray(parents)[1:]]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]


def gap(P, parents, num, loop, orbit=None):
    """(the float64 run, d): d is the largest |float64 - longdouble| of this restatement on this input"""
    f64 = interpolate_pose(P, parents, num, loop, np.float64, orbit)
    ld = interpolate_pose(P, parents, num, loop, np.longdouble, orbit)
    return f64, float(np.abs(f64.astype(np.longdouble) - ld).max())


def random_key_poses(rng, K, J=24, parents=SMPL_PARENTS, spread=0.6, max_angle=np.pi - 0.05):
    """rigid key poses by forward kinematics from random local rotations (Rodrigues, no scipy); every consecutive pair's
    relative local angle is below max_angle (consecutive around the loop too), redrawn until it is"""
    def rot(v):
        a = np.sqrt((v * v).sum())
        k = v / a
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)

    def angle(A, B):
        return np.arccos(np.clip((np.trace(A.T @ B) - 1) / 2, -1, 1))
    off = rng.normal(size=(J, 3)) * 0.2
    local = np.zeros((K, J, 3, 3))
    for j in range(J):
        for k in range(K):
            while True:
                local[k, j] = rot(rng.normal(size=3) * spread)
                if k == 0 or angle(local[k - 1, j], local[k, j]) < max_angle:
                    if k < K - 1 or angle(local[k, j], local[0, j]) < max_angle:
                        break
    out = np.zeros((K, J, 4, 4))
    for k in range(K):
        for j in range(J):
            L = np.eye(4)
            L[:3, :3] = local[k, j]
            L[:3, 3] = off[j] if j else rng.normal(size=3)
            out[k, j] = L if parents[j] < 0 else out[k, parents[j]] @ L
    return out


# ------------------------------------------------------------------------------------------------- frames
def compose_frames(color, mask, background):
    """(frames (F, S, S, 3) uint8, masks (F, S, S) uint8): fp32 throughout, in the header's order; a NaN gives 0"""
    color, mask = np.asarray(color, np.float32), np.asarray(mask, np.float32)
    F, _, n = color.shape
    S = int(round(n ** 0.5))
    bg = np.asarray(background, np.float32)
    bg = bg.reshape(bg.shape[0], 3, n) if bg.ndim else bg
    one, half = np.float32(1), np.float32(127.5)
    with np.errstate(invalid="ignore", over="ignore"):
        v = color + (one - mask[:, None]) * bg
        w = v * half + half
        w = np.where(w > 0, w, np.float32(0))
        w = np.where(w < 255, w, np.float32(255))
        m = mask * np.float32(255)
        m = np.where(m > 0, m, np.float32(0))
        m = np.where(m < 255, m, np.float32(255))
    assert w.dtype == np.float32 and m.dtype == np.float32
    return (np.ascontiguousarray(w.astype(np.uint8).transpose(0, 2, 1)).reshape(F, S, S, 3), m.astype(np.uint8).reshape(F, S, S))


# ------------------------------------------------------------------------------------------------- the recorded cases
import functools  # noqa: E402
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_interp.npz")


@functools.lru_cache(maxsize=None)
def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


@functools.lru_cache(maxsize=None)
def golden_case(n):
    """(keys, num, loop, the reference's output, the float64 referee, d) of recorded case n, computed once"""
    g = load_golden()
    K, num, loop = (int(v) for v in g["cases"][n])
    keys = g[f"case{n}_keys"]
    assert keys.shape[0] == K
    f64, d = gap(keys, SMPL_PARENTS, num, bool(loop))
    for a in (keys, f64):
        a.setflags(write=False)
    return keys, num, bool(loop), g[f"case{n}_out"], f64, d


def num_golden_cases():
    return len(load_golden()["cases"])
