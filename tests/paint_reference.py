"""Plain-numpy float64 restatement of the shade_fragments contract (include/enarf_paint.h): deferred
shading of the rasteriser's fragment buffers with a colour or a part label per vertex. It takes the fp32 buffers the
kernel takes and works from nothing else, so no pixel is ambiguous. No GPU, nothing of the product."""
import numpy as np


def _rgb(x):
    return np.broadcast_to(np.asarray(x, np.float32).astype(np.float64), (3,))


def shade(pix_to_face, bary, normals, vertices, triangles, vertex_colors=None, vertex_labels=None, palette=None, lit=True,
          background=1.0, neutral=0.5):
    """dict of albedo (R, R, 3) and shaded (R, R, 3) float64, image (R, R, 3) uint8 and drawn (R, R) bool"""
    assert (vertex_colors is None) != (vertex_labels is None)
    f = np.asarray(pix_to_face, np.int64)
    R = f.shape[0]
    b32 = np.asarray(bary, np.float32).reshape(R, R, 3)
    b = b32.astype(np.float64)
    n = np.asarray(normals, np.float32).astype(np.float64).reshape(R, R, 3)
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(v), len(t)
    bg, nt = _rgb(background), _rgb(neutral)
    albedo = np.empty((R, R, 3))
    shaded = np.empty((R, R, 3))
    albedo[:], shaded[:] = bg, bg
    drawn = (f >= 0) & (f < T)
    idx = np.zeros((R, R, 3), np.int64)
    if T:
        idx[drawn] = t[f[drawn]]
        drawn &= ((idx >= 0) & (idx < V)).all(-1)
    if drawn.any():
        i, bb, b3 = idx[drawn], b[drawn], b32[drawn]
        if vertex_colors is not None:
            c = np.asarray(vertex_colors, np.float32).astype(np.float64).reshape(V, 3)[i]          # (n, corner, channel)
            texel = (bb[:, 0, None] * c[:, 0] + bb[:, 1, None] * c[:, 1]) + bb[:, 2, None] * c[:, 2]
        else:
            pal = np.asarray(palette, np.float32).astype(np.float64).reshape(-1, 3)
            k = np.zeros(len(i), np.int64)                   # the largest fp32 b'; a later corner only when strictly larger
            best = b3[:, 0].copy()
            with np.errstate(invalid="ignore"):
                for corner in (1, 2):
                    more = b3[:, corner] > best
                    k[more], best[more] = corner, b3[more, corner]
            lab = np.asarray(vertex_labels, np.int32).reshape(V)[i[np.arange(len(i)), k]].astype(np.int64)
            known = (lab >= 0) & (lab < len(pal))
            texel = np.where(known[:, None], pal[np.where(known, lab, 0)], nt[None])
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
    return {"albedo": albedo, "shaded": shaded, "image": image, "drawn": drawn}


def ulps_from(got32, ref64):
    """how many fp32 steps got32 lies from ref64 rounded to fp32 (0 = equal); inf where exactly one of them is NaN"""
    want = np.asarray(ref64, np.float64).astype(np.float32)
    got = np.asarray(got32, np.float32)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.abs(got))).astype(np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    return np.where(both_nan, 0.0, np.where(np.isnan(d), np.inf, d))
