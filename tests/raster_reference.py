"""Plain-numpy float64 restatement of the rasterize_mesh contract (include/enarf_raster.h): projection,
coverage by 2-D barycentrics at pixel centres, perspective-correct depth and barycentrics, vertex normals in face order
and hard-Phong shading. No GPU. Each triangle's bounding box is evaluated at once; triangles are batched by box size.

`rasterize` also returns an `ambiguous` mask: the pixels whose outcome a rounding difference could change. A pixel is
ambiguous when a triangle that covers it or nearly covers it, in front of or level with the winner, has a smallest
barycentric within EPS_B of 0; when another covering triangle's zbuf is within EPS_Z (relative, but not equal) of the
winner's; or when the winner's screen area is below EPS_AREA px^2."""
import numpy as np

EPS_B, EPS_Z, EPS_AREA = 1e-4, 1e-5, 1e-6
_CHUNK = 1 << 20          # pixel candidates evaluated per batch


def project(vertices, K, img_size, R):
    """(px, py, z) float64: a vertex's position in output pixels (u / s, v / s), s = img_size / R, and its depth"""
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float32).reshape(3, 3).astype(np.float64)
    s = img_size / R
    with np.errstate(all="ignore"):
        px = (K[0, 0] * v[:, 0] / v[:, 2] + K[0, 2]) / s
        py = (K[1, 1] * v[:, 1] / v[:, 2] + K[1, 2]) / s
    return px, py, v[:, 2]


def vertex_normals(vertices, triangles):
    """(V, 3) float64: sum of (v1 - v0) x (v2 - v0) over the faces using a vertex, in face order, / max(|.|, 1e-6)"""
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    t = t[((t >= 0) & (t < len(v))).all(1)]
    p = v[t]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n = np.zeros_like(v)
    np.add.at(n, t.reshape(-1), np.repeat(fn, 3, axis=0))       # face-major: each vertex's faces in increasing id
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)


def shade(N, P):
    """uint8 level of unit normals N at points P (light and camera at the origin)"""
    c = -(N * P).sum(-1) / np.maximum(np.linalg.norm(P, axis=-1), 1e-6)
    spec = np.where(c > 0, np.maximum(2 * c * c - 1, 0) ** 64, 0.0)
    colour = 0.5 + 0.3 * np.maximum(c, 0) + 0.2 * spec
    return np.clip(np.floor(255 * colour), 0, 255).astype(np.uint8)


def _candidates(X, Y, Z, A, ids, c0, r0, c1, r1, k, R):
    """every pixel centre of the boxes (k x k, clipped) of triangles ids with min barycentric > -EPS_B"""
    out = []
    step = max(1, _CHUNK // (k * k))
    g = np.arange(k)
    for a in range(0, len(ids), step):
        sl = slice(a, a + step)
        cc = c0[sl, None, None] + g[None, None, :]
        rr = r0[sl, None, None] + g[None, :, None]
        inbox = (cc <= c1[sl, None, None]) & (rr <= r1[sl, None, None])
        x, y = cc + 0.5, rr + 0.5
        x0, x1, x2 = (X[sl, i, None, None] for i in range(3))
        y0, y1, y2 = (Y[sl, i, None, None] for i in range(3))
        area = A[sl, None, None]
        b = np.stack([((x1 - x) * (y2 - y) - (y1 - y) * (x2 - x)) / area,
                      ((x2 - x) * (y0 - y) - (y2 - y) * (x0 - x)) / area,
                      ((x0 - x) * (y1 - y) - (y0 - y) * (x1 - x)) / area], -1)
        minb = b.min(-1)
        n, i, j = np.nonzero(inbox & (minb > -EPS_B))
        tri = ids[sl][n]
        bb = b[n, i, j]
        q = bb / Z[sl][n]
        S = q.sum(-1)
        out.append((rr[n, i, 0] * R + cc[n, 0, j], tri, 1.0 / S, q / S[:, None], minb[n, i, j]))
    return out


def rasterize(vertices, triangles, K, img_size, R):
    """dict of image (R, R, 3) uint8, pix_to_face (R, R) int64, zbuf (R, R), bary (R, R, 3), normals (R, R, 3) (float64)
    and ambiguous (R, R) bool, exactly as the contract states the outputs"""
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    V = len(v)
    px, py, z = project(vertices, K, img_size, R)
    valid = ((tris >= 0) & (tris < V)).all(1)
    tc = np.where(valid[:, None], tris, 0)
    if V == 0:
        tc = np.zeros((0, 3), np.int64)
        valid = valid[:0]
    X, Y, Z = px[tc], py[tc], z[tc]
    with np.errstate(all="ignore"):
        A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        drawn = (valid & (Z > 0).all(1) & np.isfinite(Z).all(1) & np.isfinite(X).all(1) & np.isfinite(Y).all(1)
                 & (A != 0) & np.isfinite(A))
        c0 = np.maximum(np.floor(X.min(1) - 0.5), 0)
        c1 = np.minimum(np.ceil(X.max(1) - 0.5), R - 1)
        r0 = np.maximum(np.floor(Y.min(1) - 0.5), 0)
        r1 = np.minimum(np.ceil(Y.max(1) - 0.5), R - 1)
        drawn &= (c0 <= c1) & (r0 <= r1)
    ids = np.nonzero(drawn)[0]
    c0, c1, r0, r1 = (a[ids].astype(np.int64) for a in (c0, c1, r0, r1))
    X, Y, Z, A = X[ids], Y[ids], Z[ids], A[ids]
    side = np.maximum(c1 - c0, r1 - r0) + 1
    k = 2 ** np.ceil(np.log2(np.maximum(side, 1))).astype(np.int64)
    cands = []
    for kk in np.unique(k):
        m = k == kk
        cands += _candidates(X[m], Y[m], Z[m], A[m], ids[m], c0[m], r0[m], c1[m], r1[m], int(kk), R)
    npx = R * R
    p2f = np.full(npx, -1, np.int64)
    zbuf = np.full(npx, -1.0)
    bary = np.full((npx, 3), -1.0)
    normals = np.zeros((npx, 3))
    image = np.full((npx, 3), 255, np.uint8)
    amb = np.zeros(npx, bool)
    if cands:
        pix, tri, zb, bp, minb = (np.concatenate([c[i] for c in cands]) for i in range(5))
    else:
        pix, tri, zb, minb = (np.zeros(0, d) for d in (np.int64, np.int64, np.float64, np.float64))
        bp = np.zeros((0, 3))
    cov = np.nonzero(minb > 0)[0]
    order = cov[np.lexsort((tri[cov], zb[cov].astype(np.float32), pix[cov]))]
    first = order[np.r_[True, pix[order][1:] != pix[order][:-1]]] if len(order) else order
    wp = pix[first]
    p2f[wp], zbuf[wp], bary[wp] = tri[first], zb[first], bp[first]
    win_z = np.full(npx, np.inf)
    win_z[wp] = zb[first]
    win_i = np.full(npx, -1)
    win_i[wp] = first
    # another covering triangle within EPS_Z of the winner's depth (an exact tie is decided by the id: not ambiguous)
    with np.errstate(all="ignore"):
        gap = np.abs(zb[cov] - win_z[pix[cov]]) / win_z[pix[cov]]
    amb[pix[cov][(cov != win_i[pix[cov]]) & (gap > 0) & (gap < EPS_Z)]] = True
    # a triangle near an edge of its own, in front of or level with the winner
    near = np.abs(minb) <= EPS_B
    amb[pix[near & (zb <= win_z[pix] * (1 + EPS_Z))]] = True
    # a winner of (almost) no screen area
    half_area = np.zeros(len(tris))
    half_area[ids] = np.abs(A) / 2
    amb[wp[half_area[tri[first]] < EPS_AREA]] = True
    if len(wp):
        t = tris[p2f[wp]]
        w = bary[wp]
        vn = vertex_normals(vertices, triangles)
        N = (w[:, :, None] * vn[t]).sum(1)
        N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-6)
        P = (w[:, :, None] * v[t]).sum(1)
        normals[wp] = N
        image[wp] = shade(N, P)[:, None]
    return {"image": image.reshape(R, R, 3), "pix_to_face": p2f.reshape(R, R), "zbuf": zbuf.reshape(R, R),
            "bary": bary.reshape(R, R, 3), "normals": normals.reshape(R, R, 3), "ambiguous": amb.reshape(R, R)}
