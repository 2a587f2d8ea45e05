"""Referee of libenarf_sgrad.so: a float64 numpy restatement of the contract in include/enarf_sgrad.h, written from its
formulas (a lexsort by the key, running counts, cumulative sums, one segmented sum per avatar), not from the kernel (which
ranks by binary search, never sorts and scans in LDS). For every entry it also returns its magnitude: the same expression
with every leaf term replaced by its absolute value (r_j by sum |g_C s c| + sigma |g_M| + sigma |g_D| / t + sum |g_I s|,
S_j by the suffix sum of u times that, E_j's three terms added in absolute value), which is what the GPU tests' bound is
stated at. Vectorised over a ray's segments."""
import numpy as np

import scene_reference as SR

UPSTREAM = ("g_color", "g_mask", "g_disparity", "g_instance_mass")


def ray(depth, density, color, valid, render_scale, gC, gM, gD, gI):
    """one ray: depth, density (K, Nf), color (K, 3, Nf) fp32, valid (K,) or None; upstream gC (3,), gM, gD, gI (K,) float64
    -> (g_density (K, Nf), g_color (K, 3, Nf), magnitude of g_density, magnitude of g_color), float64"""
    K, Nf = depth.shape
    scale = float(np.float32(render_scale))
    gd, gc = np.zeros((K, Nf)), np.zeros((K, 3, Nf))
    md, mc = np.zeros((K, Nf)), np.zeros((K, 3, Nf))
    part = [k for k in range(K) if SR.takes_part(depth[k], density[k], color[k], 1 if valid is None else int(valid[k]))[0]]
    M = len(part) * Nf
    if M == 0:
        return gd, gc, md, mc
    s64, c64 = density.astype(np.float64), color.astype(np.float64)
    key_d = np.concatenate([np.maximum.accumulate(depth[k].astype(np.float64)) for k in part])
    key_k, key_i = np.repeat(part, Nf), np.tile(np.arange(Nf), len(part))
    order = np.lexsort((key_i, key_k, key_d))                     # by depth, then avatar, then sample
    t, who = key_d[order], key_k[order]
    where = np.empty(M, np.int64)
    where[order] = np.arange(M)                                   # position of breakpoint (part index, i)
    s_act, c_act = np.zeros((K, M)), np.zeros((K, 3, M))
    for k in part:
        active = np.cumsum(who == k) - 1
        has = (active >= 0) & (active <= Nf - 2)
        idx = np.clip(active, 0, Nf - 2)
        s_act[k] = np.where(has, s64[k][idx], 0.0)
        c_act[k] = np.where(has, c64[k][:, idx], 0.0)
    sigma = s_act.sum(0)
    a, tau = np.zeros(M), np.zeros(M)
    a[:-1] = (t[1:] - t[:-1]) * scale
    tau[:-1] = sigma[:-1] * (t[1:] - t[:-1]) * scale
    T = np.exp(-np.concatenate([[0.0], np.cumsum(tau)[:-1]]))
    dense = sigma > 0
    safe = np.where(dense, sigma, 1.0)
    u = np.where(dense, T * -np.expm1(-tau) / safe, T * a)
    u[-1] = 0.0
    h, h_abs = gM + gD / t, abs(gM) + abs(gD) / t
    sc = s_act[:, None] * c_act                                   # (K, 3, M)
    r = (gC[None, :, None] * sc).sum((0, 1)) + sigma * h + (gI[:, None] * s_act).sum(0)
    r_abs = np.abs(gC[None, :, None] * sc).sum((0, 1)) + sigma * h_abs + np.abs(gI[:, None] * s_act).sum(0)

    def after(x):                                                 # sum_{i>j} x_i
        return np.concatenate([np.cumsum(x[::-1])[::-1][1:], [0.0]])

    S, S_abs = after(u * r), after(u * r_abs)
    v, v_abs = np.where(dense, r / safe, 0.0), np.where(dense, r_abs / safe, 0.0)
    Te = T * np.exp(-tau)
    E = np.where(dense, a * (Te * v - S) - u * v, -a * S)
    E_abs = a * Te * v_abs + a * S_abs + u * v_abs
    G, G_abs = E + u * h, E_abs + u * h_abs
    for n_, k in enumerate(part):
        starts = where[n_ * Nf:(n_ + 1) * Nf]                     # ascending: the runs of samples 0 .. Nf - 2 lie between them
        run_g, run_ga, run_u = (np.add.reduceat(x, starts)[:-1] for x in (G, G_abs, u))
        lead = (gC[:, None] * c64[k][:, :-1]).sum(0) + gI[k]
        lead_abs = np.abs(gC[:, None] * c64[k][:, :-1]).sum(0) + abs(gI[k])
        gd[k, :-1], md[k, :-1] = run_g + lead * run_u, run_ga + lead_abs * run_u
        gc[k, :, :-1] = gC[:, None] * s64[k][None, :-1] * run_u
        mc[k, :, :-1] = np.abs(gc[k, :, :-1])
    return gd, gc, md, mc


def composite_bwd(depth, density, color, valid=None, render_scale=1.0, g_color=None, g_mask=None, g_disparity=None,
                  g_instance_mass=None):
    """depth, density (F, K, n, Nf), color (F, K, 3, n, Nf), valid (F, K, n) uint8 or None; upstream gradients in the
    library's layouts, None = zeros -> dict density (F, K, n, Nf), color (F, K, 3, n, Nf) in float64 and `abs` with the
    magnitudes of both"""
    F, K, n, Nf = depth.shape
    zeros = lambda *shape: np.zeros(shape)
    gC = zeros(F, 3, n) if g_color is None else np.asarray(g_color, np.float64)
    gM = zeros(F, n) if g_mask is None else np.asarray(g_mask, np.float64)
    gD = zeros(F, n) if g_disparity is None else np.asarray(g_disparity, np.float64)
    gI = zeros(F, K, n) if g_instance_mass is None else np.asarray(g_instance_mass, np.float64)
    out = dict(density=zeros(F, K, n, Nf), color=zeros(F, K, 3, n, Nf))
    out["abs"] = dict(density=zeros(F, K, n, Nf), color=zeros(F, K, 3, n, Nf))
    for f in range(F):
        for r in range(n):
            gd, gc, md, mc = ray(depth[f, :, r], density[f, :, r], color[f, :, :, r], None if valid is None else valid[f, :, r],
                                 render_scale, gC[f, :, r], float(gM[f, r]), float(gD[f, r]), gI[f, :, r])
            out["density"][f, :, r], out["color"][f, :, :, r] = gd, gc
            out["abs"]["density"][f, :, r], out["abs"]["color"][f, :, :, r] = md, mc
    return out


def upstream(F, K, n, seed=0):
    """random upstream gradients of a call, fp32 in the library's layouts: (g_color, g_mask, g_disparity, g_instance_mass)"""
    rs = np.random.RandomState(77 + seed)
    return tuple(rs.uniform(-1.0, 1.0, size=shape).astype(np.float32) for shape in ((F, 3, n), (F, n), (F, n), (F, K, n)))
