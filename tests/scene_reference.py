"""Referee of libenarf_scene.so: a float64 numpy restatement of the contract in include/enarf_scene.h, written from its
formulas (a sort by the key, running counts, a cumulative sum), not from the kernel (which ranks by binary search and never
sorts). For every ray output it also returns the sum of the absolute values of the terms it adds, the magnitude the GPU
tests' bound is stated at."""
import numpy as np

RAY_OUTPUTS = ("color", "mask", "disparity", "instance_mass")
EXACT_OUTPUTS = ("t", "source", "instance", "skipped")


def takes_part(d, s, c, valid_byte):
    """(takes part, sets its skipped bit) of one avatar on one ray: d, s (Nf,), c (3, Nf) as stored (fp32)"""
    if valid_byte == 0:
        return False, False
    ok = np.isfinite(d).all() and np.isfinite(s).all() and np.isfinite(c).all() and (d > 0).all() and (s >= 0).all()
    return bool(ok), not ok


def ray(depth, density, color, valid=None, render_scale=1.0, threshold=0.5):
    """one ray: depth, density (K, Nf), color (K, 3, Nf) fp32, valid (K,) or None -> dict of the outputs in float64 (t,
    weight (K Nf,), source (K Nf,), color (3,), mask, disparity, instance_mass (K,), instance, skipped) and `abs`, the
    sums of absolute terms of color, mask, disparity and instance_mass"""
    K, Nf = depth.shape
    scale = float(np.float32(render_scale))
    part, skipped = [], 0
    for k in range(K):
        ok, bit = takes_part(depth[k], density[k], color[k], 1 if valid is None else int(valid[k]))
        skipped |= int(bit) << k
        if ok:
            part.append(k)
    M = len(part) * Nf
    out = dict(t=np.full(K * Nf, np.inf), source=np.full(K * Nf, -1, np.int64), weight=np.zeros(K * Nf), color=np.zeros(3),
               mask=0.0, disparity=0.0, instance_mass=np.zeros(K), instance=-1, skipped=skipped)
    out["abs"] = dict(color=np.zeros(3), mask=0.0, disparity=0.0, instance_mass=np.zeros(K))
    if M == 0:
        return out
    D = {k: np.maximum.accumulate(depth[k].astype(np.float64)) for k in part}
    key_d = np.concatenate([D[k] for k in part])
    key_k = np.repeat(part, Nf)
    key_i = np.tile(np.arange(Nf), len(part))
    order = np.lexsort((key_i, key_k, key_d))                     # by depth, then avatar, then sample
    t, who = key_d[order], key_k[order]
    out["t"][:M], out["source"][:M] = t, key_k[order] * Nf + key_i[order]
    s_act, c_act = np.zeros((K, M)), np.zeros((K, 3, M))
    for k in part:
        active = np.cumsum(who == k) - 1                          # breakpoints of k at or before j, minus one
        has = (active >= 0) & (active <= Nf - 2)
        idx = np.clip(active, 0, Nf - 2)
        s_act[k] = np.where(has, density[k].astype(np.float64)[idx], 0.0)
        c_act[k] = np.where(has, color[k].astype(np.float64)[:, idx], 0.0)
    sigma = np.zeros(M)
    for k in range(K):
        sigma = sigma + s_act[k]
    tau = np.zeros(M)
    tau[:-1] = sigma[:-1] * (t[1:] - t[:-1]) * scale
    before = np.concatenate([[0.0], np.cumsum(tau)[:-1]])
    w = np.exp(-before) * -np.expm1(-tau)
    w[-1] = 0.0
    out["weight"][:M] = w
    dense = sigma > 0
    safe = np.where(dense, sigma, 1.0)
    share = np.where(dense, s_act / safe, 0.0)                    # (K, M)
    mixed = np.where(dense, (s_act[:, None] * c_act).sum(0) / safe, 0.0)      # (3, M)
    out["color"], out["abs"]["color"] = (w * mixed).sum(-1), np.abs(w * mixed).sum(-1)
    out["mask"] = out["abs"]["mask"] = float(w.sum())
    out["disparity"] = out["abs"]["disparity"] = float((w / t).sum())
    out["instance_mass"] = (w * share).sum(-1)
    out["abs"]["instance_mass"] = out["instance_mass"].copy()
    if np.float32(out["mask"]) >= np.float32(threshold):
        out["instance"] = int(np.argmax(out["instance_mass"]))   # the first of equals
    out["total_tau"] = float(tau.sum())
    return out


def composite(depth, density, color, valid=None, render_scale=1.0, threshold=0.5):
    """depth, density (F, K, n, Nf), color (F, K, 3, n, Nf), valid (F, K, n) uint8 or None -> dict of float64 / int64
    arrays in the library's layouts: color (F, 3, n), mask, disparity (F, n), instance_mass (F, K, n), instance, skipped
    (F, n), t, source, weight (F, n, K Nf), and `abs` with the sums of absolute terms of the four ray outputs"""
    F, K, n, Nf = depth.shape
    rays = [[ray(depth[f, :, r], density[f, :, r], color[f, :, :, r], None if valid is None else valid[f, :, r],
                 render_scale, threshold) for r in range(n)] for f in range(F)]

    def gather(get, shape, dtype=np.float64):
        a = np.array([[get(x) for x in row] for row in rays], dtype=dtype).reshape((F, n) + shape)
        return a

    out = {k: gather(lambda x, k=k: x[k], (K * Nf,), np.int64 if k == "source" else np.float64) for k in ("t", "source", "weight")}
    out["abs"] = {}
    for k, shape in (("color", (3,)), ("instance_mass", (K,))):
        out[k] = np.moveaxis(gather(lambda x, k=k: x[k], shape), -1, 1)
        out["abs"][k] = np.moveaxis(gather(lambda x, k=k: x["abs"][k], shape), -1, 1)
    for k in ("mask", "disparity"):
        out[k] = gather(lambda x, k=k: x[k], ())
        out["abs"][k] = gather(lambda x, k=k: x["abs"][k], ())
    out["abs"]["weight"] = np.abs(out["weight"])
    for k in ("instance", "skipped"):
        out[k] = gather(lambda x, k=k: x[k], (), np.int64)
    return out


def step32(magnitude):
    """one fp32 step at `magnitude` (>= 0, float64): the distance from it, rounded to fp32, to the next fp32 above"""
    m = np.minimum(np.abs(np.asarray(magnitude, np.float64)), float(np.finfo(np.float32).max))
    return np.spacing(m.astype(np.float32)).astype(np.float64)


def excess(got, ref, magnitude):
    """|got - fp32(ref)| in units of one fp32 step at `magnitude`, per entry: the GPU tests take <= 1"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(ref), (got.dtype, got.shape, np.shape(ref))
    with np.errstate(over="ignore"):
        want = np.asarray(ref, np.float64).astype(np.float32).astype(np.float64)
    return np.abs(got.astype(np.float64) - want) / step32(magnitude)


def composite_fine64(density, color, depth, render_scale=1.0):
    """rendering.composite_fine in float64 numpy on one ray: density, depth (Nf,), color (3, Nf) -> colour (3,), mask,
    disparity, weights (Nf - 1,)"""
    density, color, depth = (np.asarray(a, np.float64) for a in (density, color, depth))
    dd = density[:-1] * (depth[1:] - depth[:-1]) * float(np.float32(render_scale))
    w = np.exp(-(np.cumsum(dd) - dd)) * (1 - np.exp(-dd))
    return (w * color[:, :-1]).sum(-1), w.sum(), (w / depth[:-1]).sum(), w
