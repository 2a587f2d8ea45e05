"""A referee above fp32 for the tri-plane sampler (csrc/enarf_sampler.hip), the deformation-field producer beside it and
the ray sampler (csrc/enarf_raysample.hip), and a per-element bound to hold a kernel to. numpy only.

Why not float64 F.grid_sample. For fp32 inputs the operation's decisions - which texel is the floor, which taps are in
bounds, which way nearest mode rounds, how often a coordinate reflects, whether it was clipped - are DEFINED by the source
index evaluated in fp32 (ATen GridSampler.h and the reference's TriplaneSampler_kernel.cu evaluate it that way, and
gs_unnormalize switches fp contraction off to stay on it). The same index in float64 takes another decision on up to 13 % of
structured points (texel centres, edges, half-steps) at sizes that are no power of two. So:

  * the source index and its gradient multiplier are taken in np.float32, ONE IEEE operation per step, in the order of
    gs_unnormalize, gs_reflect (fmod, floor(in / span)) and gs_clip; floor, in-bounds flags and nearest rounding (half away
    from zero, ::round) come from that value;
  * everything after it is float64: the weights (ix - floor(ix) and (floor(ix) + 1) - ix are exact in fp32 and in float64
    alike for |ix| < 2^24), products, the sums over taps, planes, channels and points, and the multiplication by the
    multiplier.

Per output element the referee returns the value, S = the float64 sum of the absolute values of the terms that form it,
and k = the number of fp32 roundings on the longest path to it in ANY summation order. A kernel passes where

    |ours - ref|  <=  k * 2^-24 * S  +  1e-37        (within_bound)

on every element: a first-order forward error bound (each rounding moves a partial result, itself at most S, by at most
2^-24 of it). No tolerance is chosen by eye and no element is excused.

k, derived from the kernels' arithmetic (not from a run):
  * forward, bilinear: a term is texel * (ax * ay): the weight product rounds once, the product with the texel once, and
    the accumulation is counted as an fma-less add: 3 roundings per term at most; the 12 terms (4 taps x 3 planes) meet in
    at most 12 additions (4 into a plane's sum starting from 0, 3 plane sums into the accumulator, in any order no path is
    longer than 12).  k = 3 + 12 = 15.  With `separate` only a plane's 4 terms meet: k = 3 + 4 = 7.
  * forward, nearest: a copy. k = 0 (compared exactly).
  * grad_input: a contribution is (ax * ay) * grad_out: 2 roundings, 3 with the fast path's second addition (the
    channel-last accumulator folded into the NCHW gradient); the m contributions of a texel meet in m atomic additions in
    arbitrary order, the longest path sees all m.  k = 3 + m, m = the texel's own count of in-bounds taps.
    Nearest: a contribution is grad_out itself, k = m.
  * grad_grid: d/d ix of one plane is a sum of 4 * C terms texel * a * grad_out (2 roundings each, `a` is exact), up to
    4 * C additions; one multiplication by the multiplier; an axis receives from two planes (as x of plane d, as y of plane
    d + 2), 2 more additions: 2 + 4 * C + 1 + 2 along one plane, and the other plane's 4 * C terms can sit on the same path
    when the order is arbitrary (the fast path sums lanes by DPP).  k = 8 * C + 8 covers 8 * C + 5.
  * warp forward: 4 terms, w * texel: k = 3 + 4 = 7.  warp g_src: k = 3 + m.  warp g_flow: one plane, k = 4 * C + 4.

`_wrong` switches on one deliberate mistake (WRONG lists them). tests/test_sampler_reference_cpu.py shows that each one
breaks the bound on the structured cases, i.e. that the bound is tight enough to see the mistakes a kernel could make.
"""
import numpy as np

U = 2.0 ** -24
TINY = 1e-37
BILINEAR, NEAREST = 0, 1
ZEROS, BORDER, REFLECTION = 0, 1, 2
F32 = np.float32
_ONE, _TWO, _HALF = F32(1), F32(2), F32(0.5)

WRONG = ("plane_axes",            # plane p sampled at (c[p], c[(p+2)%3])
         "nearbyint",             # nearest mode rounds half to even
         "clip_mult_one",         # gs_clip leaves the gradient multiplier at 1
         "reflect_0_2size",       # reflection about 0 .. 2*size without align_corners
         "oob_tap_weight",        # the north-east tap keeps its weight when out of bounds (and reads the clamped texel)
         "drop_1_in_1000",        # every 1000th point contributes nothing to grad_input
         "grad_grid_31_channels")  # grad_grid summed over C - 1 channels


def within_bound(ours, ref, S, k):
    """-> (ok (bool array), ratio = |ours - ref| / (k * 2^-24 * S + 1e-37)); exact comparison where k * S == 0."""
    err = np.abs(np.asarray(ours, dtype=np.float64) - ref)
    lim = np.asarray(k, dtype=np.float64) * U * S + TINY
    return err <= lim, err / lim


# ------------------------------------------------------------------------------------------ the fp32 source index
def _clip(v, size, wrong):
    mx = F32(size - 1)
    lo, hi = v <= F32(0), v >= mx
    out = np.where(lo, F32(0), np.where(hi, mx, v)).astype(np.float32)
    g = np.where(lo | hi, F32(0), F32(1)).astype(np.float32)
    if "clip_mult_one" in wrong:
        g = np.ones_like(g)
    return out, g


def _reflect(v, twice_low, twice_high):
    if twice_low == twice_high:
        return np.zeros_like(v), np.zeros_like(v)
    mn, span = F32(twice_low) / _TWO, F32(twice_high - twice_low) / _TWO
    x = v - mn
    neg = x < F32(0)
    sgn = np.where(neg, F32(-1), F32(1)).astype(np.float32)
    x = np.where(neg, -x, x).astype(np.float32)
    extra = np.fmod(x, span)
    flips = np.floor(x / span).astype(np.int64)
    even = (flips & 1) == 0
    assert x.dtype == extra.dtype == np.float32
    out = np.where(even, extra + mn, (span - extra) + mn).astype(np.float32)
    return out, np.where(even, sgn, -sgn).astype(np.float32)


def source_index(c, size, padding, align, _wrong=frozenset()):
    """grid coordinate (fp32) -> (source index, d index / d coordinate), both np.float32, one IEEE operation per step."""
    c = np.asarray(c)
    assert c.dtype == np.float32
    if align:
        g0 = F32(size - 1) / _TWO
        v = ((c + _ONE) / _TWO) * F32(size - 1)
    else:
        g0 = F32(size) / _TWO
        v = ((c + _ONE) * F32(size) - _ONE) / _TWO
    assert v.dtype == np.float32
    g = np.full(c.shape, g0, dtype=np.float32)
    if padding == BORDER:
        v, g1 = _clip(v, size, _wrong)
        g = g * g1
    elif padding == REFLECTION:
        if align:
            v, g1 = _reflect(v, 0, 2 * (size - 1))
        elif "reflect_0_2size" in _wrong:
            v, g1 = _reflect(v, 0, 2 * size)
        else:
            v, g1 = _reflect(v, -1, 2 * size - 1)
        v, g2 = _clip(v, size, _wrong)
        g = g * g1 * g2
    assert v.dtype == np.float32 and g.dtype == np.float32
    return v, g


def nearest_index(v, _wrong=frozenset()):
    """::round of the fp32 index (half away from zero), as int64."""
    v64 = v.astype(np.float64)
    if "nearbyint" in _wrong:
        return np.rint(v64).astype(np.int64)
    return (np.sign(v64) * np.floor(np.abs(v64) + 0.5)).astype(np.int64)


def _taps(ix, iy, H, W, wrong=frozenset()):
    """[(clamped x, clamped y, weight (float64, 0 where out of bounds), in bounds, ax, ay, sign_x, sign_y)] for nw ne sw se;
    ax / ay are the factors of d weight / d iy and d weight / d ix."""
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    ix, iy, fx, fy = (a.astype(np.float64) for a in (ix, iy, fx, fy))
    ax1, ax0, ay1, ay0 = ix - fx, (fx + 1.0) - ix, iy - fy, (fy + 1.0) - iy
    out = []
    for k, (dx, dy, ax, ay, sx, sy) in enumerate(((0, 0, ax0, ay0, -1.0, -1.0), (1, 0, ax1, ay0, 1.0, -1.0),
                                                  (0, 1, ax0, ay1, -1.0, 1.0), (1, 1, ax1, ay1, 1.0, 1.0))):
        x, y = x0 + dx, y0 + dy
        inb = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        if k == 1 and "oob_tap_weight" in wrong:
            inb = np.ones_like(inb)
        out.append((np.clip(x, 0, W - 1), np.clip(y, 0, H - 1), np.where(inb, ax * ay, 0.0), inb, ax, ay, sx, sy))
    return out


def _images(point_image, b, n, n_images):
    img = np.full(n, b, dtype=np.int64) if point_image is None else np.asarray(point_image).astype(np.int64)
    live = (img >= 0) & (img < n_images)
    return np.where(live, img, 0), live


def _second_axis(p, wrong):
    return (p + 2) % 3 if "plane_axes" in wrong else (p + 1) % 3


# ------------------------------------------------------------------------------------------ the sampler
def sample(inp, grid, interp, padding, align, separate=False, point_image=None, _wrong=frozenset()):
    """inp (n_images, 3C, H, W) fp32, grid (B, n, 3) fp32 -> (value, S, k): value and S float64 (B, C, n), or (B, 3, C, n)
    with `separate`; k an int. With point_image ((n,) ints, B == 1) point i samples image point_image[i]."""
    inp, grid = np.asarray(inp), np.asarray(grid)
    assert inp.dtype == np.float32 and grid.dtype == np.float32
    n_img, C3, H, W = inp.shape
    C, (B, n, _) = C3 // 3, grid.shape
    assert point_image is not None or n_img == B
    x64 = inp.astype(np.float64)
    P = 3 if separate else 1
    val, S = np.zeros((B, P, C, n)), np.zeros((B, P, C, n))
    ch = np.arange(C)[:, None]
    for b in range(B):
        im, live = _images(point_image, b, n, n_img)
        if interp == BILINEAR:
            for p in range(3):
                ix, _ = source_index(grid[b, :, p], W, padding, align, _wrong)
                iy, _ = source_index(grid[b, :, _second_axis(p, _wrong)], H, padding, align, _wrong)
                for x, y, w, _inb, *_ in _taps(ix, iy, H, W, _wrong):
                    t = x64[im[None], p * C + ch, y[None], x[None]] * (w * live)[None]
                    val[b, p if separate else 0] += t
                    S[b, p if separate else 0] += np.abs(t)
        else:   # the reference overwrites per plane: the last plane (zx) wins
            xi = nearest_index(source_index(grid[b, :, 2], W, padding, align, _wrong)[0], _wrong)
            yi = nearest_index(source_index(grid[b, :, 0], H, padding, align, _wrong)[0], _wrong)
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H) & live
            t = x64[im[None], 2 * C + ch, np.clip(yi, 0, H - 1)[None], np.clip(xi, 0, W - 1)[None]] * ok[None]
            val[b, 2 if separate else 0] = t
            S[b, 2 if separate else 0] = np.abs(t)
    k = 0 if interp == NEAREST else (7 if separate else 15)
    if not separate:
        val, S = val[:, 0], S[:, 0]
    return val, S, k


def _scatter(flat, weights, size):
    return np.bincount(flat.ravel(), weights=weights.ravel(), minlength=size)[:size]


def sample_grads(grad_out, inp, grid, interp, padding, align, separate=False, point_image=None, _wrong=frozenset()):
    """Gradients of sum(sample(...) * grad_out). grad_out (B, C, n) or (B, 3, C, n) fp32 -> dict:
    grad_input, gi_S (n_images, 3C, H, W) float64, gi_k (same shape, ints: 3 + m, nearest m);
    grad_grid, gg_S (B, n, 3) float64, gg_k (int: 8C + 8; nearest sends nothing: zeros, S 0)."""
    inp, grid, go = np.asarray(inp), np.asarray(grid), np.asarray(grad_out)
    assert inp.dtype == np.float32 and grid.dtype == np.float32 and go.dtype == np.float32
    n_img, C3, H, W = inp.shape
    C, (B, n, _) = C3 // 3, grid.shape
    x64 = inp.astype(np.float64)
    go = go.astype(np.float64).reshape(B, 3 if separate else 1, C, n)
    N = inp.size
    gi, gi_S, gi_m = np.zeros(N), np.zeros(N), np.zeros(N)
    gg, gg_S = np.zeros((B, n, 3)), np.zeros((B, n, 3))
    ch = np.arange(C)[:, None]
    Cg = C - 1 if "grad_grid_31_channels" in _wrong else C
    for b in range(B):
        im, live = _images(point_image, b, n, n_img)
        give = live & (np.arange(n) % 1000 != 999) if "drop_1_in_1000" in _wrong else live
        if interp == BILINEAR:
            for p in range(3):
                q = _second_axis(p, _wrong)
                gO = go[b, p if separate else 0]
                ix, gxm = source_index(grid[b, :, p], W, padding, align, _wrong)
                iy, gym = source_index(grid[b, :, q], H, padding, align, _wrong)
                gix, giy, sx_abs, sy_abs = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
                for x, y, w, inb, ax, ay, sx, sy in _taps(ix, iy, H, W, _wrong):
                    flat = ((im[None] * C3 + p * C + ch) * H + y[None]) * W + x[None]
                    on = (inb & give)[None] * np.ones((C, 1))
                    t = (w * give)[None] * gO
                    gi += _scatter(flat, t, N)
                    gi_S += _scatter(flat, np.abs(t), N)
                    gi_m += _scatter(flat, on, N)
                    v = (x64[im[None], p * C + ch, y[None], x[None]] * (inb & live)[None] * gO)[:Cg]
                    gix += sx * (v * ay[None]).sum(0)
                    giy += sy * (v * ax[None]).sum(0)
                    sx_abs += np.abs(v * ay[None]).sum(0)
                    sy_abs += np.abs(v * ax[None]).sum(0)
                gxm, gym = gxm.astype(np.float64), gym.astype(np.float64)
                gg[b, :, p] += gxm * gix
                gg[b, :, q] += gym * giy
                gg_S[b, :, p] += np.abs(gxm) * sx_abs
                gg_S[b, :, q] += np.abs(gym) * sy_abs
        else:   # only the plane the forward read receives gradient; the grid gets none
            xi = nearest_index(source_index(grid[b, :, 2], W, padding, align, _wrong)[0], _wrong)
            yi = nearest_index(source_index(grid[b, :, 0], H, padding, align, _wrong)[0], _wrong)
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H) & give
            flat = ((im[None] * C3 + 2 * C + ch) * H + np.clip(yi, 0, H - 1)[None]) * W + np.clip(xi, 0, W - 1)[None]
            t = go[b, 2 if separate else 0] * ok[None]
            gi += _scatter(flat, t, N)
            gi_S += _scatter(flat, np.abs(t), N)
            gi_m += _scatter(flat, ok[None] * np.ones((C, 1)), N)
    m = np.rint(gi_m).astype(np.int64).reshape(inp.shape)
    return {"grad_input": gi.reshape(inp.shape), "gi_S": gi_S.reshape(inp.shape), "gi_k": m if interp == NEAREST else 3 + m,
            "gi_m": m, "grad_grid": gg, "gg_S": gg_S, "gg_k": 8 * C + 8}


# ------------------------------------------------------------------------------------------ the deformation-field producer
def warp_index(flow, H, W):
    """warp_taps' own fp32 expression: flow (B, 6, H, W) fp32 -> ix, iy (B, 3, H, W) np.float32."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32
    xs = np.arange(W, dtype=np.float32)[None, None, None, :]
    ys = np.arange(H, dtype=np.float32)[None, None, :, None]
    gx = ((xs + _HALF) + flow[:, 0::2]) / (_HALF * F32(W)) - _ONE
    gy = ((ys + _HALF) + flow[:, 1::2]) / (_HALF * F32(H)) - _ONE
    ix = ((gx + _ONE) * F32(W) - _ONE) / _TWO
    iy = ((gy + _ONE) * F32(H) - _ONE) / _TWO
    assert ix.dtype == np.float32 and iy.dtype == np.float32
    return ix, iy


def warp(src_cl, flow):
    """src_cl (3, H, W, C) fp32 channel-last constant planes, flow (B, 6, H, W) fp32 -> (value, S, k), (B, 3, H, W, C):
    plane p sampled at (x + flow[2p], y + flow[2p + 1]), bilinear, zeros padding, align_corners False."""
    src = np.asarray(src_cl)
    assert src.dtype == np.float32
    _, H, W, C = src.shape
    B = flow.shape[0]
    ix, iy = warp_index(flow, H, W)
    s64 = src.astype(np.float64)
    pl = np.arange(3)[None, :, None, None]
    val, S = np.zeros((B, 3, H, W, C)), np.zeros((B, 3, H, W, C))
    for x, y, w, _inb, *_ in _taps(ix, iy, H, W):
        t = s64[pl, y, x] * w[..., None]
        val += t
        S += np.abs(t)
    return val, S, 7


def warp_grads(g_out_cl, src_cl, flow):
    """-> dict g_src, gs_S (3, H, W, C) float64, gs_k (3 + m); g_flow, gf_S (B, 6, H, W) float64, gf_k (4C + 4)."""
    src, go = np.asarray(src_cl), np.asarray(g_out_cl)
    assert src.dtype == np.float32 and go.dtype == np.float32
    _, H, W, C = src.shape
    B = flow.shape[0]
    ix, iy = warp_index(flow, H, W)
    s64, go = src.astype(np.float64), go.astype(np.float64)
    pl = np.broadcast_to(np.arange(3)[None, :, None, None], ix.shape)
    N = src.size
    gs, gs_S, gs_m = np.zeros(N), np.zeros(N), np.zeros(N)
    gf, gf_S = np.zeros((B, 6, H, W)), np.zeros((B, 6, H, W))
    ch = np.arange(C)
    for x, y, w, inb, ax, ay, sx, sy in _taps(ix, iy, H, W):
        flat = (((pl * H + y) * W + x)[..., None] * C + ch)
        t = w[..., None] * go
        gs += _scatter(flat, t, N)
        gs_S += _scatter(flat, np.abs(t), N)
        gs_m += _scatter(flat, inb[..., None] * np.ones(C), N)
        v = s64[pl, y, x] * inb[..., None] * go
        gf[:, 0::2] += sx * (v * ay[..., None]).sum(-1)
        gf[:, 1::2] += sy * (v * ax[..., None]).sum(-1)
        gf_S[:, 0::2] += np.abs(v * ay[..., None]).sum(-1)
        gf_S[:, 1::2] += np.abs(v * ax[..., None]).sum(-1)
    m = np.rint(gs_m).astype(np.int64).reshape(src.shape)
    return {"g_src": gs.reshape(src.shape), "gs_S": gs_S.reshape(src.shape), "gs_k": 3 + m, "gs_m": m,
            "g_flow": gf, "gf_S": gf_S, "gf_k": 4 * C + 4}


# ------------------------------------------------------------------------------------------ the ray sampler
def _window_max(a, radius, axis):
    """max over |d| <= radius along `axis`; positions outside the image do not take part."""
    out = a.copy()
    a = np.moveaxis(a, axis, -1)
    o = np.moveaxis(out, axis, -1)          # a view: writes land in `out`
    L = a.shape[-1]
    for d in range(1, min(radius, L - 1) + 1):
        np.maximum(o[..., :L - d], a[..., d:], out=o[..., :L - d])
        np.maximum(o[..., d:], a[..., :L - d], out=o[..., d:])
    return out


def dilate_topk(mask, noise, k, radius):
    """mask (B, h, w), noise (B, h*w) -> (score (B, h*w) np.float32, threshold (B,) np.float32): score = fp32(window
    maximum of the mask over (2r+1)^2 in-image positions) + fp32(noise), one fp32 addition; threshold = the k-th largest
    score of each image. The k largest are every pixel above the threshold and k - (that count) of those equal to it."""
    m = np.asarray(mask, dtype=np.float32)
    nz = np.asarray(noise, dtype=np.float32)
    B, h, w = m.shape
    dil = _window_max(_window_max(m, radius, 2), radius, 1)
    score = dil.reshape(B, h * w) + nz
    assert score.dtype == np.float32
    thr = np.sort(score, axis=1)[:, h * w - k]
    return score, thr


# ------------------------------------------------------------------------------------------ structured points
def axis_points(sizes, seed, n=None):
    """Grid coordinates that sit ON the sampler's decisions, for an axis that indexes planes of the given sizes:
      * +-1, +-(1 - 2^-24), +-(1 + 2^-23), 0 (the ends of the plane, one ulp inside, one ulp outside);
      * for each size and both align_corners conventions, the coordinate of every source index that is a multiple of 0.5
        from two sizes below the plane to three above: texel centres (weights exactly 0 and 1), texel edges, the
        half-steps of nearest mode, the clip limits, the reflection boundaries and the periods beyond them;
      * +-1.5, +-3, +-7.25, +-1000, +-4097.3 (several reflection periods; |c| <= 1e4 keeps every index below 2^24);
      * uniform draws in [-4, 4] up to one more than a multiple of 256 points (every kernel's points per workgroup - 32,
        64, 128, 256 - divides 256), or up to n.
    float32, in a seeded random order; an n below the length of the list keeps the first n of that order."""
    pts = [0.0]
    for s in (1.0, -1.0):
        pts += [s, s * (1.0 - 2.0 ** -24), s * (1.0 + 2.0 ** -23), s * 1.5, s * 3.0, s * 7.25, s * 1000.0, s * 4097.3]
    for size in sorted(set(sizes)):
        t = np.arange(-4 * size, 6 * size + 1) * 0.5                # source index, -2 size .. 3 size in steps of 0.5
        pts += list((2.0 * t + 1.0) / size - 1.0)                    # align_corners False
        if size > 1:
            pts += list(2.0 * t / (size - 1) - 1.0)                  # align_corners True
    rng = np.random.default_rng(seed)
    full = max(-(-(len(pts) + 8) // 256) * 256 + 1, n or 0)
    pts = np.concatenate([np.asarray(pts), rng.uniform(-4.0, 4.0, full - len(pts))]).astype(np.float32)
    assert np.isfinite(pts).all() and np.abs(pts).max() <= 1e4
    return pts[rng.permutation(full)][:n]


def structured_grid(H, W, B, seed, n=None):
    """(B, n, 3) fp32: every axis carries axis_points((H, W)) (each coordinate indexes a W-wide plane as x and an H-high
    plane as y), the axes combined by independent seeded shuffles, not the full product."""
    return np.ascontiguousarray(np.stack([np.stack([axis_points((H, W), seed + 101 * b + 7 * d, n) for d in range(3)], axis=-1)
                                          for b in range(B)]))


def random_f32(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
