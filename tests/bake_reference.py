"""Plain-numpy float64 restatement of the texture-atlas contracts (include/enarf_bake.h): the layout, the
surface point of every texel, the RGBA8 / fp32 texture, and the deferred textured shading. It takes the fp32 / integer
buffers the kernels take and works from nothing else. No GPU, nothing of the product."""
import numpy as np

import paint_reference as PR


def ulps_from(got32, ref64):
    """paint_reference.ulps_from, with equal infinities counted as equal: how many fp32 steps got32 lies from ref64 rounded
    to fp32 (0 = equal); inf where exactly one of them is NaN"""
    want = np.asarray(ref64, np.float64).astype(np.float32)
    got = np.asarray(got32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(got == want, 0.0, PR.ulps_from(got, ref64))


class Unsupported(Exception):
    pass


def layout(T, A):
    """(c, n): the largest c >= 6 with 2 (A // c)^2 >= T, searched downward from A; Unsupported when there is none"""
    assert 6 <= A <= 8192 and T >= 0
    for c in range(A, 5, -1):
        n = A // c
        if 2 * n * n >= T:
            return c, n
    raise Unsupported(f"{T} triangles do not fit an atlas of {A}")


def local_corners(c):
    """(2, 3, 2): the corners of the lower and of the upper triangle of a cell, (x, y) in texels"""
    return np.array([[[1, 1], [c - 3, 1], [1, c - 3]], [[c - 1, c - 1], [3, c - 1], [c - 1, 3]]], np.float64)


def corners(T, A):
    """(T, 3, 2) float64: every corner's (x, y) in atlas texels"""
    c, n = layout(T, A)
    t = np.arange(T)
    q, h = t // 2, t % 2
    origin = np.stack([(q % n) * c, (q // n) * c], -1).astype(np.float64)
    return origin[:, None, :] + local_corners(c)[h]


def uv(T, A):
    """(T, 3, 2) float64 in [0, 1]: the corners over the atlas size (row 0 at the top, as glTF)"""
    return corners(T, A) / A


def owners(T, A):
    """(A, A) int64 [row, column]: the triangle slot that owns each texel by the layout alone (a slot >= T included), -1 in
    the margin; and the in-cell (i, j) of every texel"""
    c, n = layout(T, A)
    y, x = np.meshgrid(np.arange(A), np.arange(A), indexing="ij")
    cx, cy = x // c, y // c
    i, j = x - cx * c, y - cy * c
    h = np.where(i + j + 1 <= c, 0, 1)
    slot = 2 * (cy * n + cx) + h
    return np.where((cx < n) & (cy < n), slot, -1), i, j, h


def points(vertices, triangles, A):
    """dict of points (3, A A) float64 and texel_face (A, A) int32"""
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    c, n = layout(T, A)
    slot, i, j, h = owners(T, A)
    face = np.where(slot < T, slot, -1)
    if T:
        idx = t[np.clip(face, 0, T - 1)]
        face = np.where(((idx >= 0) & (idx < V)).all(-1), face, -1)
    own = face >= 0
    L = float(c - 4)
    u, w = i + 0.5, j + 0.5
    a1 = np.where(h == 0, u - 1.0, (c - 1) - u) / L
    a2 = np.where(h == 0, w - 1.0, (c - 1) - w) / L
    a0 = (1.0 - a1) - a2
    p = np.zeros((A, A, 3))
    if own.any():
        k = t[face[own]]
        q0, q1, q2 = v[k[:, 0]], v[k[:, 1]], v[k[:, 2]]
        p[own] = (a0[own][:, None] * q0 + a1[own][:, None] * q1) + a2[own][:, None] * q2
    return {"points": p.reshape(-1, 3).T.copy(), "texel_face": face.astype(np.int32)}


def _rgb(x):
    return np.broadcast_to(np.asarray(x, np.float32).astype(np.float64), (3,))


def level(x):
    with np.errstate(invalid="ignore"):
        return np.floor(255.0 * np.clip(np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf), 0.0, 1.0)).astype(np.uint8)


def resolve(texel_face, color=None, labels=None, palette=None, fill=0.0, neutral=0.5, unit=False):
    """dict of texture (rows, A, 4) uint8 and texture_f32 (rows, A, 3) float64"""
    assert (color is None) != (labels is None)
    face = np.asarray(texel_face, np.int32)
    own = (face >= 0).reshape(-1)
    M = face.size
    v = np.empty((M, 3))
    v[:] = _rgb(fill)
    if color is not None:
        x = np.asarray(color, np.float32).astype(np.float64).reshape(3, M).T
        with np.errstate(invalid="ignore", over="ignore"):
            val = x if unit else (x + 1.0) / 2.0
    else:
        pal = np.asarray(palette, np.float32).astype(np.float64).reshape(-1, 3)
        lab = np.asarray(labels, np.int32).reshape(M).astype(np.int64)
        known = (lab >= 0) & (lab < len(pal))
        val = np.where(known[:, None], pal[np.where(known, lab, 0)], _rgb(neutral)[None])
    v[own] = val[own]
    rgba = np.zeros((M, 4), np.uint8)
    rgba[:, :3] = level(v)
    rgba[:, 3] = np.where(own, 255, 0)
    return {"texture": rgba.reshape(face.shape + (4,)), "texture_f32": v.reshape(face.shape + (3,))}


def _axis(u, A):
    with np.errstate(invalid="ignore"):
        s = u - 0.5
        f = np.floor(s)
        w1 = s - f
        w0 = 1.0 - w1
        i0 = np.fmin(np.fmax(f, 0.0), A - 1.0).astype(np.int64)
        i1 = np.fmin(np.fmax(f + 1.0, 0.0), A - 1.0).astype(np.int64)
    return i0, i1, w0, w1


def tap(texture, u, w):
    """the bilinear tap of the contract at (u, w) (arrays): (n, 3) float64 and the four (row, column) index pairs"""
    tex = np.asarray(texture)
    A = tex.shape[0]
    t = tex[..., :3].astype(np.float64) / 255.0 if tex.dtype == np.uint8 else tex.astype(np.float32).astype(np.float64)
    x0, x1, wx0, wx1 = _axis(u, A)
    y0, y1, wy0, wy1 = _axis(w, A)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (((wx0 * wy0)[:, None] * t[y0, x0] + (wx1 * wy0)[:, None] * t[y0, x1]) + (wx0 * wy1)[:, None] * t[y1, x0]) \
            + (wx1 * wy1)[:, None] * t[y1, x1]
    return out, ((y0, x0), (y0, x1), (y1, x0), (y1, x1))


def shade(pix_to_face, bary, normals, vertices, triangles, texture, lit=True, background=1.0):
    """dict of albedo, shaded (R, R, 3) float64, image (R, R, 3) uint8, drawn (R, R) bool, uv (R, R, 2) float64 (NaN where
    nothing is drawn)"""
    f = np.asarray(pix_to_face, np.int64)
    R = f.shape[0]
    b = np.asarray(bary, np.float32).astype(np.float64).reshape(R, R, 3)
    n = np.asarray(normals, np.float32).astype(np.float64).reshape(R, R, 3)
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    A = np.asarray(texture).shape[0]
    bg = _rgb(background)
    albedo, shaded = np.empty((R, R, 3)), np.empty((R, R, 3))
    albedo[:], shaded[:] = bg, bg
    uvs = np.full((R, R, 2), np.nan)
    drawn = (f >= 0) & (f < T)
    idx = np.zeros((R, R, 3), np.int64)
    if T:
        idx[drawn] = t[f[drawn]]
        drawn &= ((idx >= 0) & (idx < V)).all(-1)
    if drawn.any():
        i, bb = idx[drawn], b[drawn]
        U = corners(T, A)[f[drawn]]                                          # (n, corner, xy)
        with np.errstate(invalid="ignore", over="ignore"):
            u = (bb[:, 0] * U[:, 0, 0] + bb[:, 1] * U[:, 1, 0]) + bb[:, 2] * U[:, 2, 0]
            w = (bb[:, 0] * U[:, 0, 1] + bb[:, 1] * U[:, 1, 1]) + bb[:, 2] * U[:, 2, 1]
        texel, _ = tap(texture, u, w)
        uvs[drawn] = np.stack([u, w], -1)
        if lit:
            p = v[i]
            q = (bb[:, 0, None] * p[:, 0] + bb[:, 1, None] * p[:, 1]) + bb[:, 2, None] * p[:, 2]
            nn = n[drawn]
            with np.errstate(all="ignore"):
                dn = np.maximum(np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2]), 1e-6)
                dq = np.maximum(np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]), 1e-6)
                N = nn / dn[:, None]
                c_ = -((N[:, 0] * q[:, 0] + N[:, 1] * q[:, 1]) + N[:, 2] * q[:, 2]) / dq
                spec = np.where(c_ > 0, np.maximum(2.0 * c_ * c_ - 1.0, 0.0) ** 64, 0.0)
                out = texel * (0.5 + 0.3 * np.where(c_ > 0, c_, 0.0))[:, None] + (0.2 * spec)[:, None]
        else:
            out = texel
        albedo[drawn], shaded[drawn] = texel, out
    with np.errstate(invalid="ignore"):
        image = np.floor(255.0 * np.clip(np.nan_to_num(shaded, nan=0.0), 0.0, 1.0)).astype(np.uint8)
    return {"albedo": albedo, "shaded": shaded, "image": image, "drawn": drawn, "uv": uvs}
