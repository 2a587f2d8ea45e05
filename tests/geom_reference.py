"""Plain-numpy float64 restatement of the two contracts of include/enarf_geom.h: the geometry buffers
of a (disparity, mask) pair and the running depth error. It takes the fp32 values the kernels take, rounds the scalars to
fp32 as the argument structure does, and works from nothing else. No GPU, nothing of the product."""
import numpy as np

SHADES = {"normal": 0, "lit": 1, "depth": 2}


def _f(x):
    """a scalar as the fp32 the kernel is handed, in float64"""
    return np.float64(np.float32(x))


def _shift(a, dr, dc, fill):
    """out[b, r, c] = a[b, r + dr, c + dc] inside the image, `fill` outside"""
    out = np.full_like(a, fill)
    H, W = a.shape[1:3]
    rs, rd = (slice(dr, H), slice(0, H - dr)) if dr >= 0 else (slice(0, H + dr), slice(-dr, H))
    cs, cd = (slice(dc, W), slice(0, W - dc)) if dc >= 0 else (slice(0, W + dc), slice(-dc, W))
    out[:, rd, cd] = a[:, rs, cs]
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def buffers(disparity, mask, inv_intrinsics, origin=(0, 0), step=1.0, depth_scale=1.0, mask_threshold=0.5, edge=0.05,
            normalise=True, shade="normal", near=None, far=None, background=1.0):
    """dict of depth (B, H, W), points and normals (B, H, W, 3) float64, flags (B, H, W) uint8 and image (B, H, W, 3) uint8"""
    q32, m32 = np.asarray(disparity, np.float32), np.asarray(mask, np.float32)
    B, H, W = q32.shape
    K = np.asarray(inv_intrinsics, np.float32).astype(np.float64).reshape(-1, 3, 3)
    K = np.broadcast_to(K, (B, 3, 3))
    bg = np.broadcast_to(np.asarray(background, np.float32).astype(np.float64), (3,))
    with np.errstate(all="ignore"):
        valid = np.isfinite(q32) & np.isfinite(m32) & (m32 >= np.float32(mask_threshold)) & (q32 > 0)
        q, m = q32.astype(np.float64), m32.astype(np.float64)
        z = np.where(valid, _f(depth_scale) * (m / q) if normalise else _f(depth_scale) / q, 0.0)
        x = _f(origin[0]) + (np.arange(W, dtype=np.float64) + 0.5) * _f(step)
        y = _f(origin[1]) + (np.arange(H, dtype=np.float64) + 0.5) * _f(step)
        ray = (K[:, None, None, :, 0] * x[None, None, :, None] + K[:, None, None, :, 1] * y[None, :, None, None]) + K[:, None, None, :, 2]
        p = z[..., None] * ray

        def neighbour(dr, dc):
            zn, pn = _shift(z, dr, dc, 0.0), _shift(p, dr, dc, 0.0)
            ok = _shift(valid, dr, dc, False)
            if not _f(edge) < 0:
                ok = ok & (np.abs(zn - z) <= _f(edge) * z)
            return ok, pn

        def difference(lo, hi):
            (use_lo, p_lo), (use_hi, p_hi) = lo, hi
            d = np.where(use_hi[..., None], p_hi, p) - np.where(use_lo[..., None], p_lo, p)
            return use_lo | use_hi, d

        has_dx, dx = difference(neighbour(0, -1), neighbour(0, 1))
        has_dy, dy = difference(neighbour(-1, 0), neighbour(1, 0))
        n = np.stack([dy[..., 1] * dx[..., 2] - dy[..., 2] * dx[..., 1],
                      dy[..., 2] * dx[..., 0] - dy[..., 0] * dx[..., 2],
                      dy[..., 0] * dx[..., 1] - dy[..., 1] * dx[..., 0]], -1)
        length = np.sqrt(_dot(n, n))
        has_normal = valid & has_dx & has_dy & (length > 0) & (length < np.inf)
        N = np.where(has_normal[..., None], n / length[..., None], 0.0)
        N = np.where((_dot(N, p) > 0)[..., None], -N, N)
        N = np.where(has_normal[..., None], N, 0.0)

        v = np.empty((B, H, W, 3))
        v[:] = bg
        mode = SHADES[shade]
        if mode == 0:
            rgb = np.stack([0.5 + 0.5 * N[..., 0], 0.5 + 0.5 * -N[..., 1], 0.5 + 0.5 * -N[..., 2]], -1)
            v = np.where(has_normal[..., None], rgb, v)
        elif mode == 1:
            dp = np.maximum(np.sqrt(_dot(p, p)), 1e-6)
            c = -_dot(N, p) / dp
            spec = np.where(c > 0, np.maximum(2.0 * c * c - 1.0, 0.0), 0.0)
            for _ in range(6):
                spec = spec * spec
            grey = (0.5 + 0.3 * np.where(c > 0, c, 0.0)) + 0.2 * spec
            v = np.where(has_normal[..., None], grey[..., None], v)
        else:
            inv_far = 1.0 / _f(far)
            grey = (1.0 / z - inv_far) / (1.0 / _f(near) - inv_far)
            v = np.where(valid[..., None], grey[..., None], v)
        image = np.floor(255.0 * np.clip(np.nan_to_num(v, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)).astype(np.uint8)
    flags = (valid.astype(np.uint8) | (has_normal.astype(np.uint8) << 1)).astype(np.uint8)
    return {"depth": z, "points": p, "normals": N, "flags": flags, "image": image, "shaded": v}


def depth_error(disparity, target, mask=None, mask_threshold=0.5):
    """the quantities of one update, as float64 / int: n, sse_all, n_fg, sse_fg, inter, union"""
    q32, g32 = np.asarray(disparity, np.float32).reshape(-1), np.asarray(target, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        sq = (q32.astype(np.float64) - g32.astype(np.float64)) ** 2
        fg = g32 > 0
        sil = q32 > 0 if mask is None else np.asarray(mask, np.float32).reshape(-1) >= np.float32(mask_threshold)
        return {"n": int(q32.size), "sse_all": float(sq.sum()), "n_fg": int(fg.sum()), "sse_fg": float(sq[fg].sum()),
                "inter": int((sil & fg).sum()), "union": int((sil | fg).sum())}


def merge(results):
    """the running totals after several updates, with the ratios DepthError.result() reports"""
    total = {k: sum(r[k] for r in results) for k in ("n", "sse_all", "n_fg", "sse_fg", "inter", "union")}
    total["inv_depth_mse"] = total["sse_all"] / total["n"]
    total["iou"] = total["inter"] / total["union"] if total["union"] else float("nan")
    return total


def ulps_from(got32, ref64):
    """how many fp32 steps got32 lies from ref64 rounded to fp32 (0 = equal); inf where exactly one of them is NaN"""
    with np.errstate(over="ignore"):
        want = np.asarray(ref64, np.float64).astype(np.float32)
    got = np.asarray(got32, np.float32)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.abs(got))).astype(np.float64)
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    return np.where(same, 0.0, np.where(np.isnan(d), np.inf, d))


def angle_deg(a, b):
    """angle between unit vectors, in degrees"""
    return np.degrees(np.arccos(np.clip(_dot(np.asarray(a, np.float64), np.asarray(b, np.float64)), -1.0, 1.0)))
