"""Plain-numpy float64 restatement of the normal-map contracts (include/enarf_nmap.h): the tangent frame,
the encoding of a vector per texel, and the normal-mapped deferred shading. It takes the fp32 / integer buffers the kernels
take and works from nothing else. The atlas layout and the bilinear tap are bake_reference's, imported; the light and Phong
terms restate paint_reference.shade's lines on a float64 unit normal (that function rounds its normals to fp32 on entry,
so it cannot be handed Ns; tests/test_nmap_cpu.py holds `lighting` to it bit for bit on stored normals). `bug=` plants one
of three mistakes for the test that shows the GPU test can see them. No GPU, nothing of the product."""
import numpy as np

import bake_reference as BR

BUGS = (None, "no_flip", "swapped_bitangent", "decode_without_shift")


def _len(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def frames(vertices, triangles, bug=None):
    """(tangent, bitangent, normal (T, 3) float64, valid (T,) bool): the frame of every triangle; rows of an invalid one
    (a vertex outside [0, V), |e1| or |e1 x e2| zero or not finite) are unspecified"""
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    inside = ((t >= 0) & (t < V)).all(-1) if T else np.zeros(0, bool)
    p = v[np.where(inside[:, None], t, 0)] if V else np.zeros((T, 3, 3))
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        c = _cross(e1, e2)
        l1, lc = _len(e1), _len(c)
        valid = inside & (l1 > 0) & (l1 < np.inf) & (lc > 0) & (lc < np.inf)
        s = np.where(np.arange(T) % 2 == 0, 1.0, -1.0)
        if bug == "no_flip":
            s = np.ones(T)
        n = c / lc[:, None]
        tg = (s[:, None] * e1) / l1[:, None]
        bt = _cross(n, tg) if bug == "swapped_bitangent" else _cross(tg, n)
    return tg, bt, n, valid


def channel(c):
    """floor(255 clamp((c + 1) / 2, 0, 1) + 0.5) and the value inside the floor"""
    h = np.clip((np.asarray(c, np.float64) + 1.0) / 2.0, 0.0, 1.0)
    x = 255.0 * h + 0.5
    return np.floor(x).astype(np.uint8), x


def encode(texel_face, vectors, vertices, triangles, negate=True, min_length=0.0, bug=None):
    """dict of texture (shape of texel_face, 4) uint8, texture_f32 (..., 3) float64, levels (..., 3) float64 (the values
    255 v + 0.5 whose floor is the byte) and flat (...) bool (owned texels that took (0, 0, 1))"""
    face = np.asarray(texel_face, np.int32)
    M = face.size
    f = face.reshape(-1).astype(np.int64)
    vec = np.asarray(vectors, np.float32).astype(np.float64).reshape(3, M).T
    T = len(np.asarray(triangles).reshape(-1, 3))
    tg, bt, n, valid = frames(vertices, triangles, bug)
    q = np.zeros((M, 3))
    q[:, 2] = 1.0
    framed = (f >= 0) & (f < T)
    framed[framed] = valid[f[framed]]
    g = -vec if negate else vec
    with np.errstate(all="ignore"):
        m = _len(g)
        ok = framed & (m > float(np.float32(min_length))) & (m < np.inf)
        k = f[ok]
        gg, mm = g[ok], m[ok]
        q[ok] = np.stack([_dot(gg, tg[k]) / mm, _dot(gg, bt[k]) / mm, _dot(gg, n[k]) / mm], -1)
    byte, x = channel(q)
    rgba = np.concatenate([byte, np.where(f >= 0, 255, 0).astype(np.uint8)[:, None]], 1)
    return {"texture": rgba.reshape(face.shape + (4,)), "texture_f32": q.reshape(face.shape + (3,)),
            "levels": x.reshape(face.shape + (3,)), "flat": ((f >= 0) & ~ok).reshape(face.shape)}


def lighting(texel, unit_normal, point):
    """paint_reference.shade's light and Phong terms: texel (0.5 + 0.3 max(c, 0)) + 0.2 max(2 c c - 1, 0)^64 with
    c = -(N . p) / max(|p|, 1e-6), N a unit normal in float64"""
    with np.errstate(all="ignore"):
        dq = np.maximum(_len(point), 1e-6)
        c_ = -_dot(unit_normal, point) / dq
        spec = np.where(c_ > 0, np.maximum(2.0 * c_ * c_ - 1.0, 0.0) ** 64, 0.0)
        return texel * (0.5 + 0.3 * np.where(c_ > 0, c_, 0.0))[:, None] + (0.2 * spec)[:, None]


def stored_unit(nn):
    """N = normals / max(|normals|, 1e-6) of enarf_paint.h"""
    with np.errstate(all="ignore"):
        return nn / np.maximum(_len(nn), 1e-6)[:, None]


def decode(texture, bug=None):
    """the normal texture as float64 (A, A, 3): a byte is 2 byte / 255 - 1, an fp32 texel is taken as it is (and so is a
    float64 one: encode's own unrounded texture_f32, for the round trip inside the referee)"""
    tex = np.asarray(texture)
    if tex.dtype == np.uint8:
        d = (2.0 * tex[..., :3].astype(np.float64)) / 255.0
        return d if bug == "decode_without_shift" else d - 1.0
    return tex.astype(np.float64)


def shade(pix_to_face, bary, normals, vertices, triangles, normal_texture, texture=None, base_color=1.0, lit=True,
          background=1.0, bug=None):
    """dict of albedo, normal, shaded (R, R, 3) float64, image (R, R, 3) uint8, drawn and framed (R, R) bool"""
    f = np.asarray(pix_to_face, np.int64)
    R = f.shape[0]
    b = np.asarray(bary, np.float32).astype(np.float64).reshape(R, R, 3)
    n = np.asarray(normals, np.float32).astype(np.float64).reshape(R, R, 3)
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    A = np.asarray(normal_texture).shape[0]
    bg = BR._rgb(background)
    albedo, shaded, normal = np.empty((R, R, 3)), np.empty((R, R, 3)), n.copy()
    albedo[:], shaded[:] = bg, bg
    drawn = (f >= 0) & (f < T)
    idx = np.zeros((R, R, 3), np.int64)
    if T:
        idx[drawn] = t[f[drawn]]
        drawn &= ((idx >= 0) & (idx < V)).all(-1)
    framed = np.zeros((R, R), bool)
    if drawn.any():
        i, bb, ff = idx[drawn], b[drawn], f[drawn]
        U = BR.corners(T, A)[ff]
        with np.errstate(invalid="ignore", over="ignore"):
            u = (bb[:, 0] * U[:, 0, 0] + bb[:, 1] * U[:, 1, 0]) + bb[:, 2] * U[:, 2, 0]
            w = (bb[:, 0] * U[:, 0, 1] + bb[:, 1] * U[:, 1, 1]) + bb[:, 2] * U[:, 2, 1]
        if texture is not None:
            texel, _ = BR.tap(texture, u, w)
        else:
            texel = np.broadcast_to(BR._rgb(base_color), (len(ff), 3)).copy()
        q, _ = _tap64(decode(normal_texture, bug), u, w)
        tg, bt, nr, valid = frames(vertices, t, bug)
        ok = valid[ff]
        with np.errstate(all="ignore"):
            lq = _len(q)
            bad = ~((lq > 0) & (lq < np.inf))
            q = np.where(bad[:, None], [0.0, 0.0, 1.0], q)
            wv = (q[:, 0, None] * tg[ff] + q[:, 1, None] * bt[ff]) + q[:, 2, None] * nr[ff]
            ns = wv / _len(wv)[:, None]
        stored = n[drawn]
        unit = np.where(ok[:, None], ns, stored_unit(stored))
        normal[drawn] = np.where(ok[:, None], ns, stored)
        framed[drawn] = ok
        if lit:
            p = v[i]
            point = (bb[:, 0, None] * p[:, 0] + bb[:, 1, None] * p[:, 1]) + bb[:, 2, None] * p[:, 2]
            out = lighting(texel, unit, point)
        else:
            out = texel
        albedo[drawn], shaded[drawn] = texel, out
    with np.errstate(invalid="ignore"):
        image = np.floor(255.0 * np.clip(np.nan_to_num(shaded, nan=0.0), 0.0, 1.0)).astype(np.uint8)
    return {"albedo": albedo, "normal": normal, "shaded": shaded, "image": image, "drawn": drawn, "framed": framed}


def _tap64(decoded, u, w):
    """bake_reference.tap's sum on already decoded float64 texels (a decoded byte is no fp32 number, and tap rounds a float
    texture to fp32 on entry): the indices and weights are bake_reference's, the four-term sum is restated"""
    t = np.asarray(decoded, np.float64)
    A = t.shape[0]
    x0, x1, wx0, wx1 = BR._axis(u, A)
    y0, y1, wy0, wy1 = BR._axis(w, A)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (((wx0 * wy0)[:, None] * t[y0, x0] + (wx1 * wy0)[:, None] * t[y0, x1]) + (wx0 * wy1)[:, None] * t[y1, x0]) \
            + (wx1 * wy1)[:, None] * t[y1, x1]
    return out, ((y0, x0), (y0, x1), (y1, x0), (y1, x1))


def tap_normal(normal_texture, T, face, bary, bug=None):
    """the decoded, tapped q (n, 3) at barycentrics `bary` (n, 3) float64 of faces `face` (n,): the round-trip tests' probe"""
    A = np.asarray(normal_texture).shape[0]
    U = BR.corners(T, A)[face]
    u = (bary[:, 0] * U[:, 0, 0] + bary[:, 1] * U[:, 1, 0]) + bary[:, 2] * U[:, 2, 0]
    w = (bary[:, 0] * U[:, 0, 1] + bary[:, 1] * U[:, 1, 1]) + bary[:, 2] * U[:, 2, 1]
    return _tap64(decode(normal_texture, bug), u, w)[0]
