"""The sampler referee (tests/sampler_reference.py) and its bound, settled on the CPU before any kernel is involved:
it agrees with float64 F.grid_sample and autograd away from decisions, takes fp32 ATen's decisions on them, reproduces the
reference's goldens, lets the fp32 torch evaluation through on every element and stops each deliberate mistake."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampler_reference as R
from _helpers import load_golden

PADS = ["zeros", "border", "reflection"]
OPTIONS = [(pad, align) for pad in range(3) for align in (False, True)]


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def torch_sample(inp, grid, interp, padding, align, dtype, separate=False, grad_out=None):
    """The tri-plane operator as three F.grid_sample calls in `dtype` (nearest: the last plane alone) -> value, or
    (value, grad_input, grad_grid) with grad_out. inp (B, 3C, H, W), grid (B, n, 3) numpy.

    In fp32 the calls go to ATen's scalar grid sampler (GridSampler.h, the functions the reference's CUDA operator calls;
    torch reaches it as _grid_sampler_2d_cpu_fallback). F.grid_sample's default CPU path is a vectorised kernel that
    contracts the unnormalisation to one fma, (c + 1) * (size / 2) - 0.5, and reflects by another formula: an index
    that differs in the last bit, i.e. not the operation the reference defines. Measured on the structured list of
    C 5, H 5, W 70, zeros, align_corners False: 4 of 15370 forward elements leave the bound, by up to 12.4x, all at
    c[2] = 0.44285714626312256, whose index is 50.0 step by step and 50.0000001 exactly - a texel centre the fma
    steps over."""
    x, q = _t(inp, dtype).requires_grad_(True), _t(grid, dtype).requires_grad_(True)
    C = x.shape[1] // 3
    mode = "bilinear" if interp == R.BILINEAR else "nearest"
    outs = []
    for p in range(3):
        g2 = torch.stack([q[..., p], q[..., (p + 1) % 3]], dim=-1)[:, :, None]
        if dtype == torch.float32:
            outs.append(torch._grid_sampler_2d_cpu_fallback(x[:, p * C:(p + 1) * C], g2, interp, padding, align)[..., 0])
        else:
            outs.append(F.grid_sample(x[:, p * C:(p + 1) * C], g2, mode=mode, padding_mode=PADS[padding], align_corners=align)[..., 0])
    if interp == R.NEAREST:
        out = torch.stack([torch.zeros_like(outs[2])] * 2 + [outs[2]], dim=1) if separate else outs[2]
    else:
        out = torch.stack(outs, dim=1) if separate else outs[0] + outs[1] + outs[2]
    if grad_out is None:
        return out.detach().numpy()
    gi, gg = torch.autograd.grad(out, [x, q], _t(grad_out, dtype), allow_unused=True)
    gg = torch.zeros_like(q) if gg is None else gg
    return out.detach().numpy(), gi.numpy(), gg.numpy()


def _inputs(C, H, W, B, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, 3 * C, H, W)).astype(np.float32), rng.standard_normal((B, C, n)).astype(np.float32)


def _check(name, ours, ref, S, k):
    ok, ratio = R.within_bound(ours, ref, S, k)
    assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.size} elements outside k u S, worst ratio {ratio.max():.3g}"
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ agreement with torch
def _continuous_grid(H, W, B, n, align, seed):
    """Coordinates whose source index (for both sizes) stays >= 1e-3 from every multiple of 0.5 - texel centres, edges,
    half-steps, clip limits, reflection boundaries - by construction: index = j / 2 + [0.05, 0.45] on the W axis, and
    rejected (redrawn) where the H axis' index comes closer than 0.01."""
    rng = np.random.default_rng(seed)

    def index(c, size):
        return (c + 1) / 2 * (size - 1) if align else ((c + 1) * size - 1) / 2

    def coord(t, size):
        return 2 * t / (size - 1) - 1 if align else (2 * t + 1) / size - 1
    out = np.empty(B * n * 3)
    filled = 0
    while filled < out.size:
        t = rng.integers(-2 * W, 6 * W, 4 * out.size) / 2 + rng.uniform(0.05, 0.45, 4 * out.size)
        c = coord(t, W).astype(np.float32).astype(np.float64)
        th = index(c, H)
        c = c[np.abs(th * 2 - np.rint(th * 2)) > 0.02][:out.size - filled]
        out[filled:filled + c.size] = c
        filled += c.size
    grid = out.reshape(B, n, 3).astype(np.float32)
    for size in (H, W):        # asserted, in float64 and in the referee's fp32
        for t in (index(grid.astype(np.float64), size), R.source_index(grid, size, R.ZEROS, align)[0].astype(np.float64)):
            assert (np.abs(t * 2 - np.rint(t * 2)) >= 2e-3).all()
    return grid


@pytest.mark.parametrize("interp", [R.BILINEAR, R.NEAREST])
@pytest.mark.parametrize("padding,align", OPTIONS)
def test_referee_agrees_with_float64_grid_sample_away_from_decisions(interp, padding, align):
    """Away from decisions the only difference between the referee and float64 torch is the fp32 rounding of the index:
    at most 5 operations on magnitudes up to 5 * size + 1 <= 6 * size (|c| <= 4), so |d index| <= 30 * size * 2^-24 = e.
    A weight moves by at most 2e (ax, ay <= 1): forward 12 taps * 2e * max|inp|; a grad_input texel m * 2e * max|grad_out|;
    grad_grid size/2 * 2 planes * 4C terms * e * max|inp| * max|grad_out|. A structural mistake is O(1) of these scales."""
    C, H, W, B, n = 5, 7, 9, 2, 400
    inp, go = _inputs(C, H, W, B, n, 3)
    grid = _continuous_grid(H, W, B, n, align, 5 + padding)
    e = 30 * max(H, W) * R.U
    ref, gi, gg = torch_sample(inp, grid, interp, padding, align, torch.float64, grad_out=go)
    val, S, k = R.sample(inp, grid, interp, padding, align)
    g = R.sample_grads(go, inp, grid, interp, padding, align)
    a, d = np.abs(inp).max(), np.abs(go).max()
    if interp == R.NEAREST:
        assert np.array_equal(val, ref) and np.array_equal(g["grad_grid"], gg) and not g["grad_grid"].any()
        assert np.abs(g["grad_input"] - gi).max() <= g["gi_m"].max() * 2.0 ** -52 * d * n
        return
    assert np.abs(val - ref).max() <= 24 * e * a
    assert np.abs(g["grad_input"] - gi).max() <= g["gi_m"].max() * 2 * e * d
    assert np.abs(g["grad_grid"] - gg).max() <= max(H, W) / 2 * 8 * C * e * a * d
    assert np.abs(ref).max() > 0.5 and np.abs(gi).max() > 0.5 and np.abs(gg).max() > 0.5


def test_referee_separate_and_point_image_against_float64_torch():
    C, H, W, n = 4, 6, 5, 300
    inp, _ = _inputs(C, H, W, 3, n, 8)
    grid = _continuous_grid(H, W, 1, n, False, 2)
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 3, n)
    bad = ids.copy()
    bad[::7], bad[3::11], bad[5::13] = 3, -1, 1 << 30
    live = (bad >= 0) & (bad < 3)
    go = rng.standard_normal((1, 3, C, n)).astype(np.float32)
    val, S, k = R.sample(inp, grid, R.BILINEAR, R.ZEROS, False, separate=True, point_image=bad)
    g = R.sample_grads(go, inp, grid, R.BILINEAR, R.ZEROS, False, separate=True, point_image=bad)
    assert k == 7 and not val[..., ~live].any() and not g["grad_grid"][0, ~live].any()
    e = 30 * max(H, W) * R.U
    gi_ref = np.zeros(inp.shape)
    for i in range(3):
        sel = np.nonzero(bad == i)[0]
        ref, gi, gg = torch_sample(inp[i:i + 1], grid[:, sel], R.BILINEAR, R.ZEROS, False, torch.float64, separate=True,
                                   grad_out=go[..., sel])
        assert np.abs(val[..., sel] - ref).max() <= 8 * e * np.abs(inp).max()
        assert np.abs(g["grad_grid"][:, sel] - gg).max() <= max(H, W) / 2 * 8 * C * e * np.abs(inp).max() * np.abs(go).max()
        gi_ref[i] = gi[0]
    assert np.abs(g["grad_input"] - gi_ref).max() <= g["gi_m"].max() * 2 * e * np.abs(go).max()


# ------------------------------------------------------------------------------------------ decisions and the bound
STRUCTURED = [(5, 5, 70), (5, 37, 100), (8, 1, 7), (8, 7, 1), (32, 16, 16)]     # (C, H, W)


@pytest.fixture(scope="module")
def structured():
    """{(C, H, W): (inp, grid, grad_out)}: the structured point lists of the GPU cases, batch 2, computed once."""
    out = {}
    for C, H, W in STRUCTURED:
        grid = R.structured_grid(H, W, 2, 11)
        inp, go = _inputs(C, H, W, 2, grid.shape[1], C + H)
        out[C, H, W] = (inp, grid, go)
    return out


@pytest.mark.parametrize("C,H,W", STRUCTURED)
def test_referee_takes_fp32_atens_decisions_and_fp32_torch_passes_the_bound(structured, C, H, W):
    """On the structured lists - points ON floors, edges, clip limits and reflection boundaries - fp32 CPU F.grid_sample
    and its autograd lie within k * 2^-24 * S of the referee on EVERY element, forward, grad_input and grad_grid, all six
    padding / align_corners settings: one differing floor, in-bounds flag, reflection count or clip multiplier is an O(1)
    error on that element. Nearest mode: ATen rounds half to even where the reference kernel rounds half away from zero
    (::round), so fp32 torch meets the referee's `nearbyint` variant exactly, and the referee proper wherever the two
    roundings agree."""
    inp, grid, go = structured[C, H, W]
    for padding, align in OPTIONS:
        name = f"C={C} H={H} W={W} {PADS[padding]} align={align}"
        out, gi, gg = torch_sample(inp, grid, R.BILINEAR, padding, align, torch.float32, grad_out=go)
        val, S, k = R.sample(inp, grid, R.BILINEAR, padding, align)
        g = R.sample_grads(go, inp, grid, R.BILINEAR, padding, align)
        _check(name + " forward", out, val, S, k)
        _check(name + " grad_input", gi, g["grad_input"], g["gi_S"], g["gi_k"])
        _check(name + " grad_grid", gg, g["grad_grid"], g["gg_S"], g["gg_k"])
        near = torch_sample(inp, grid, R.NEAREST, padding, align, torch.float32)
        even, _, _ = R.sample(inp, grid, R.NEAREST, padding, align, _wrong={"nearbyint"})
        away, _, _ = R.sample(inp, grid, R.NEAREST, padding, align)
        assert np.array_equal(near, even), name + " nearest"
        same = np.ones(grid.shape[:2], dtype=bool)
        for axis, size in ((2, W), (0, H)):
            v = R.source_index(grid[..., axis], size, padding, align)[0]
            same &= R.nearest_index(v) == R.nearest_index(v, {"nearbyint"})
        for b in range(grid.shape[0]):
            assert np.array_equal(near[b][:, same[b]], away[b][:, same[b]]), name + " nearest, away from half-steps"
        assert not same.all() or H * W == 1, "the structured list must hold half-steps"


def test_source_index_spot_values():
    """Hand-checked decisions: the ends of the plane, a half-step, a clip limit, size 1."""
    f = lambda *c: np.asarray(c, dtype=np.float32)
    v, g = R.source_index(f(-1, 1, 0), 4, R.ZEROS, False)
    assert v.tolist() == [-0.5, 3.5, 1.5] and g.tolist() == [2, 2, 2]
    v, g = R.source_index(f(-1, 1, 0, 1.5), 5, R.BORDER, True)
    assert v.tolist() == [0, 4, 2, 4] and g.tolist() == [0, 0, 2, 0]          # the multiplier is 0 AT the limits
    v, g = R.source_index(f(-1.5, 1.5, 3), 4, R.REFLECTION, False)             # -1.5 | 4.5 | 7.5 reflect about -0.5 .. 3.5
    assert v.tolist() == [0.5, 2.5, 0] and g.tolist() == [-2, -2, 0]
    v, g = R.source_index(f(-3, 0.3, 1000), 1, R.REFLECTION, True)             # twice_low == twice_high
    assert not v.any() and not g.any()
    v, g = R.source_index(f(-3, 0.25, 7.25), 1, R.REFLECTION, False)           # span 1 about -0.5 .. 0.5, then clipped to 0
    assert not v.any() and not g.any()
    assert R.nearest_index(f(0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997)).tolist() == [1, 2, 3, -1, -2, 0]
    assert R.nearest_index(f(0.5, 1.5, 2.5, -0.5), {"nearbyint"}).tolist() == [0, 2, 2, 0]


# ------------------------------------------------------------------------------------------ goldens
def _near(name, ours, ref, S, k, slack):
    err = np.abs(np.asarray(ours, dtype=np.float64) - ref)
    assert (err <= k * R.U * S + slack).all(), f"{name}: worst excess {(err - k * R.U * S - slack).max():.3g}"


def test_referee_reproduces_the_reference_goldens():
    """tests/golden/sampler_b2.npz (forward and both gradients) and the sampler entries of sampling_api.npz (sample_feature:
    sum over planes, batch 2; batch_idx on the side-by-side planes).

    The goldens were recorded from the reference's F.grid_sample formulation on the CPU, whose vectorised kernel takes
    the unnormalisation as one fma (see torch_sample): its index is the referee's up to the two roundings the fma
    saves, e = 2 * 2^-24 * (max|c| + 1) * size. So each element is held to k u S plus what e can move it, the forward
    and grad_input being continuous in the index: a weight moves by at most e per axis, i.e. forward 3 planes * 2 axes *
    2 max|input| * e (adjacent texels differ by at most 2 max), a grad_input texel m * 2e * max|grad_out|, and grad_grid -
    constant in its own axis between texel centres, linear in the other - size/2 * 2 planes * 4C * e * max|input| *
    max|grad_out|. (A mistake in the operator is O(1) of these scales; the per-element k u S comparisons are those of
    test_referee_takes_fp32_atens_decisions_and_fp32_torch_passes_the_bound and of the GPU tests.)"""
    g = load_golden("sampler_b2")
    grid = np.ascontiguousarray(g["position"].transpose(0, 2, 1))
    C, (H, W) = g["input"].shape[1] // 3, g["input"].shape[2:]
    e = 2 * R.U * (np.abs(grid).max() + 1) * max(H, W)
    a, d = np.abs(g["input"]).max(), np.abs(g["grad_output"]).max()
    val, S, k = R.sample(g["input"], grid, R.BILINEAR, R.ZEROS, False)
    _near("sampler_b2 forward", g["output"], val, S, k, 12 * e * a)
    r = R.sample_grads(g["grad_output"], g["input"], grid, R.BILINEAR, R.ZEROS, False)
    _near("sampler_b2 grad_input", g["grad_input"], r["grad_input"], r["gi_S"], r["gi_k"], r["gi_m"] * 2 * e * d)
    _near("sampler_b2 grad_grid", g["grad_position"].transpose(0, 2, 1), r["grad_grid"], r["gg_S"], r["gg_k"],
          max(H, W) / 2 * 8 * C * e * a * d)
    a = load_golden("sampling_api")
    B, _, h, w = a["planes"].shape
    pos = np.ascontiguousarray(a["pos"].reshape(B, 3, -1).transpose(0, 2, 1))
    val, S, k = R.sample(a["planes"], pos, R.BILINEAR, R.ZEROS, False)
    _near("sampling_api out_sum", a["out_sum"].reshape(val.shape), val, S, k,
          12 * 2 * R.U * (np.abs(pos).max() + 1) * max(h, w) * np.abs(a["planes"]).max())
    # out_bidx: the reference laid the planes side by side, (h + 1) * B wide, and transformed the x coordinate in fp32
    # (sampling.py:34-38: a multiplication and two additions, then the unnormalisation on the wider plane): its index is the
    # per-image index up to e = 4 roundings * 2^-24 * (h + 1) * B; zeros padding and the zero column between the images
    # keep the output continuous in it.
    feat = a["feat"]
    pos1 = np.ascontiguousarray(a["pos1"].reshape(1, 3, -1).transpose(0, 2, 1))
    val, S, k = R.sample(feat, pos1, R.BILINEAR, R.ZEROS, False, point_image=a["bidx"].reshape(-1))
    e = 4 * R.U * (feat.shape[2] + 1) * feat.shape[0]
    _near("sampling_api out_bidx", a["out_bidx"].reshape(val.shape), val, S, k, 12 * e * np.abs(feat).max())


# ------------------------------------------------------------------------------------------ the bound discriminates
# mutant -> the structured case it is shown to fail on: (C, H, W), padding, align_corners, output
MUTANT_FAILS = {
    "plane_axes": ((5, 5, 70), R.ZEROS, False, "forward"),
    "nearbyint": ((5, 5, 70), R.ZEROS, False, "nearest"),
    "clip_mult_one": ((5, 5, 70), R.BORDER, False, "grad_grid"),
    "reflect_0_2size": ((5, 5, 70), R.REFLECTION, False, "forward"),
    "oob_tap_weight": ((5, 5, 70), R.ZEROS, False, "forward"),
    "drop_1_in_1000": ((5, 5, 70), R.BORDER, False, "grad_input"),
    "grad_grid_31_channels": ((32, 16, 16), R.ZEROS, False, "grad_grid"),
}


def _outputs(inp, grid, go, padding, align, wrong=frozenset()):
    val, S, k = R.sample(inp, grid, R.BILINEAR, padding, align, _wrong=wrong)
    g = R.sample_grads(go, inp, grid, R.BILINEAR, padding, align, _wrong=wrong)
    near = R.sample(inp, grid, R.NEAREST, padding, align, _wrong=wrong)
    return {"forward": (val, S, k), "grad_input": (g["grad_input"], g["gi_S"], g["gi_k"]),
            "grad_grid": (g["grad_grid"], g["gg_S"], g["gg_k"]), "nearest": near}


@pytest.mark.parametrize("mutant", R.WRONG)
def test_bound_rejects_each_deliberate_mistake(structured, mutant):
    """Each mistake a kernel could make, evaluated in float64 and rounded to fp32 (so nothing but the mistake separates it
    from the referee), leaves k * 2^-24 * S on at least one element of the structured case named in MUTANT_FAILS - where
    the fp32 torch evaluation passes on every element (test_referee_takes_fp32_atens_decisions_...)."""
    assert set(MUTANT_FAILS) == set(R.WRONG)
    shape, padding, align, what = MUTANT_FAILS[mutant]
    inp, grid, go = structured[shape]
    ref, S, k = _outputs(inp, grid, go, padding, align)[what]
    bad = _outputs(inp, grid, go, padding, align, {mutant})[what][0].astype(np.float32)
    ok, ratio = R.within_bound(bad, ref, S, k)
    assert not ok.all(), f"{mutant} passes {what} of {shape} {PADS[padding]} align={align}"
    assert ratio.max() > 100, ratio.max()            # not a near miss: an O(1) error on that element


def test_bound_sees_one_lost_atomic_in_a_thousand_under_contention():
    """The contention case of the GPU tests (4133 points per image in one 2 x 2 footprint, C = 32): with every 1000th point's
    contribution lost, a texel misses 4 of its m = 4133 terms, ~1e-3 of S, against (3 + m) * 2^-24 = 2.5e-4."""
    C, n = 32, 4096 + 37
    grid = np.random.default_rng(31).uniform(-0.24, 0.24, (2, n, 3)).astype(np.float32)
    inp, go = R.random_f32((2, 3 * C, 4, 4), 14), R.random_f32((2, C, n), 15)
    g = R.sample_grads(go, inp, grid, R.BILINEAR, R.ZEROS, False)
    assert set(np.unique(g["gi_m"])) == {0, n}
    _, gi, _ = torch_sample(inp, grid, R.BILINEAR, R.ZEROS, False, torch.float32, grad_out=go)
    _check("fp32 torch under contention", gi, g["grad_input"], g["gi_S"], g["gi_k"])
    bad = R.sample_grads(go, inp, grid, R.BILINEAR, R.ZEROS, False, _wrong={"drop_1_in_1000"})["grad_input"].astype(np.float32)
    ok, ratio = R.within_bound(bad, g["grad_input"], g["gi_S"], g["gi_k"])
    assert not ok.all() and ratio.max() > 2, ratio.max()


# ------------------------------------------------------------------------------------------ warp and ray sampler
@pytest.mark.parametrize("H,W", [(5, 7), (3, 3), (1, 9), (32, 40)])
def test_warp_referee_against_grid_sample(H, W):
    """warp / warp_grads against the reference's formulation (models/narf.py:40-58: F.grid_sample on (pixel centre + flow)
    / (W / 2) - 1) through ATen's scalar sampler in fp32, per element within k u S; the flow gradient passes through the
    multiplier W/2 and the division by W/2 on the way back, the two roundings k = 4C + 4 has to spare."""
    B, C = 2, 32
    rng = np.random.default_rng(H * W)
    flow = (3.0 * rng.standard_normal((B, 6, H, W))).astype(np.float32)
    flow[:, :, :, :1] = np.rint(flow[:, :, :, :1]) + 0.5
    flow[:, :, :, 1:2] = np.rint(flow[:, :, :, 1:2])
    src, go = R.random_f32((3, H, W, C), 16), R.random_f32((B, 3, H, W, C), 17)
    x, f = _t(src).requires_grad_(True), _t(flow).requires_grad_(True)
    gx = (torch.arange(W) + 0.5 + f[:, 0::2]) / (0.5 * W) - 1
    gy = (torch.arange(H)[:, None] + 0.5 + f[:, 1::2]) / (0.5 * H) - 1
    grid = torch.stack([gx, gy], dim=-1).reshape(B * 3, H, W, 2)
    planes = x.permute(0, 3, 1, 2)[None].expand(B, -1, -1, -1, -1).reshape(B * 3, C, H, W)
    out = torch._grid_sampler_2d_cpu_fallback(planes, grid, 0, 0, False).reshape(B, 3, C, H, W).permute(0, 1, 3, 4, 2)
    gs, gf = torch.autograd.grad(out, [x, f], _t(go))
    _check("warp forward", out.detach().numpy(), *R.warp(src, flow))
    g = R.warp_grads(go, src, flow)
    _check("warp g_src", gs.numpy(), g["g_src"], g["gs_S"], g["gs_k"])
    _check("warp g_flow", gf.numpy(), g["g_flow"], g["gf_S"], g["gf_k"])
    assert np.abs(g["g_flow"]).max() > 0.5 and g["gs_m"].max() > 1


@pytest.mark.parametrize("B,h,w,k,radius", [(1, 1, 1, 1, 0), (2, 3, 257, 1, 128), (1, 300, 5, 1500, 64), (3, 40, 56, 100, 0),
                                            (1, 40, 56, 2239, 5), (1, 9, 9, 20, 128)])
def test_dilate_topk_referee_against_max_pool_and_topk(B, h, w, k, radius):
    """dilate_topk against the reference's formulation, F.max_pool2d(2r + 1, stride 1, padding r) + noise -> torch.topk
    (ray_sampler.py:23-30), on the shapes of the GPU cases: the same scores bit for bit, and the k-th largest as threshold."""
    rng = np.random.default_rng(h * w + k)
    mask = rng.choice(np.asarray([-1.5, -0.25, 0.0, 0.5, 2.0], dtype=np.float32), (B, h, w))
    noise = rng.uniform(-1.0, 1.0, (B, h * w)).astype(np.float32)
    score, thr = R.dilate_topk(mask, noise, k, radius)
    dil = _t(mask)
    for r in [64] * (radius // 64) + [radius % 64]:          # max_pool2d wants padding <= kernel / 2: windows compose
        dil = F.max_pool2d(dil[:, None], 2 * r + 1, stride=1, padding=r)[:, 0] if r else dil
    ref = dil.reshape(B, h * w) + _t(noise)
    assert np.array_equal(score, ref.numpy())
    top = torch.topk(ref, k, dim=1)[0]
    assert np.array_equal(thr, top[:, -1].numpy())
    assert ((score > thr[:, None]).sum(1) < k).all() and ((score >= thr[:, None]).sum(1) >= k).all()
