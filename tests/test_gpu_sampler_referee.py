"""The tri-plane sampler, the deformation-field producer and the ray sampler against the referee of
tests/sampler_reference.py, per element:  |ours - ref| <= k * 2^-24 * S + 1e-37  (fp32 source index, float64 after it; S the
sum of the absolute terms of that element, k its rounding count). No tolerance chosen by eye, no fraction allowed to
fail, no point excluded; integer outputs and exact zeros are compared exactly. The points sit ON the decisions: c = +-1 and
one ulp either side, every texel centre, edge and half-step from two sizes below the plane to three above, the clip
limits, the reflection boundaries and several periods beyond them (sampler_reference.axis_points).

The `worst` figures in the comments are the largest |ours - ref| / (k * 2^-24 * S) an MI355X gave: records of the kernels
against the referee, not thresholds - the threshold is 1."""
import numpy as np
import pytest
import torch

import sampler_reference as R

pytestmark = pytest.mark.gpu
OPTIONS = [(pad, align) for pad in range(3) for align in (False, True)]
PADS = ["zeros", "border", "reflection"]


@pytest.fixture(scope="module")
def ops():
    from enarf_gan_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h(t):
    return t.detach().cpu().numpy()


def _hold(name, ours, ref, S, k):
    ours = _h(ours).reshape(ref.shape)
    ok, ratio = R.within_bound(ours, ref, S, k)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"ratio {worst:.3f}  {name}")
    if not ok.all():
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.size} elements outside k u S; worst at {i}: ours {ours[i]!r} "
                             f"referee {ref[i]!r} S {S[i]!r} k {np.broadcast_to(k, ref.shape)[i]} ratio {worst:.3g}")
    return worst


def _exact(name, ours, ref):
    ours = _h(ours).reshape(ref.shape)
    assert np.array_equal(ours, ref.astype(ours.dtype)), f"{name}: {int((ours != ref).sum())} elements differ"


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("C", [8, 16, 32, 64, 5, 1])
@pytest.mark.parametrize("H,W", [(5, 70), (37, 100), (1, 7), (7, 1), (16, 16)])
def test_sampler_forward_on_decisions(ops, C, H, W):
    """pack_kernel<C> + sample_fwd_cl<C/8> (workspace; C 8, 16, 32, 64) and sample_fwd_direct<false> (no workspace; C 5 and 1
    only have it), batch 2, all six padding / align_corners settings, n one more than a multiple of 256 and n = 1.
    H == 1 and W == 1 take gs_reflect's twice_low == twice_high branch under align_corners.
    worst: 0.212 (channel-last), 0.212 (direct)."""
    grid = R.structured_grid(H, W, 2, 11)
    assert grid.shape[1] % 256 == 1
    inp = R.random_f32((2, 3 * C, H, W), C + H)
    for padding, align in OPTIONS:
        ref = R.sample(inp, grid, R.BILINEAR, padding, align)
        for ws in (True, False):
            name = f"fwd C={C} {H}x{W} {PADS[padding]} align={align} ws={ws}"
            out = ops.triplane_sample_fwd(_d(inp), _d(grid)[:, :, None], 0, padding, align, use_workspace=ws)
            _hold(name, out, *ref)
            one = ops.triplane_sample_fwd(_d(inp), _d(grid[:, :1])[:, :, None], 0, padding, align, use_workspace=ws)
            _hold(name + " n=1", one, *(a[..., :1] if isinstance(a, np.ndarray) else a for a in ref))


@pytest.mark.parametrize("H,W", [(5, 70), (16, 16)])
def test_sampler_nearest_rounds_half_away_from_zero(ops, H, W):
    """Nearest mode on the half-steps (source index exactly j + 0.5): the reference's ::round, not ATen's nearbyint; the
    last plane alone, read at (c[2], c[0]). A copy: compared exactly. Its backward: grad_input per element, no gradient to
    the grid. worst (grad_input): 0.500 (two contributions, one addition: 1 of k = m = 2 roundings)."""
    C = 5
    grid = R.structured_grid(H, W, 2, 13)
    inp, go = R.random_f32((2, 3 * C, H, W), 3), R.random_f32((2, C, grid.shape[1]), 4)
    halves = 0
    for padding, align in OPTIONS:
        name = f"nearest {H}x{W} {PADS[padding]} align={align}"
        v = R.source_index(grid[..., 2], W, padding, align)[0].astype(np.float64)
        halves += int((np.abs(v - np.floor(v) - 0.5) == 0).sum())
        ref, _, k = R.sample(inp, grid, R.NEAREST, padding, align)
        assert k == 0
        _exact(name, ops.triplane_sample_fwd(_d(inp), _d(grid)[:, :, None], 1, padding, align), ref)
        g = R.sample_grads(go, inp, grid, R.NEAREST, padding, align)
        gi, gg = ops.triplane_sample_bwd(_d(go)[..., None], _d(inp), _d(grid)[:, :, None], 1, padding, align, True, True)
        _hold(name + " grad_input", gi, g["grad_input"], g["gi_S"], g["gi_k"])
        _exact(name + " grad_grid", gg, np.zeros(gg.shape))
    assert halves > 100, "the list must hold half-steps"


def _point_image_case(n_images=3, C=8, H=5, W=70):
    grid = R.structured_grid(H, W, 1, 17)
    n = grid.shape[1]
    ids = np.random.default_rng(5).integers(0, n_images, n).astype(np.int32)
    ids[::7], ids[3::11], ids[5::13] = n_images, -1, 1 << 30
    return R.random_f32((n_images, 3 * C, H, W), 6), grid, ids, (ids < 0) | (ids >= n_images)


@pytest.mark.parametrize("separate", [True, False])
def test_sampler_separate_planes_and_point_image(ops, separate):
    """sample_fwd_direct<true> (`separate`: the planes side by side) and <false> with a per-point image id, 3 images, ids
    outside the batch (negative, n_images, 1 << 30): those sample exact zeros. Then sample_bwd_direct's `separate` and
    point_image branches: out-of-batch points send and receive nothing. worst: 0.294 forward, 0.461 grad_input,
    0.047 grad_grid."""
    inp, grid, ids, off = _point_image_case()
    C, n = inp.shape[1] // 3, grid.shape[1]
    ref, S, k = R.sample(inp, grid, R.BILINEAR, R.ZEROS, False, separate=separate, point_image=ids)
    out = ops.triplane_sample_ex_fwd(_d(inp), _d(grid), separate=separate, point_image=_d(ids))
    _hold(f"ex fwd separate={separate}", out, ref, S, k)
    assert off.sum() > 100 and not _h(out)[..., off].any()
    go = R.random_f32((1, 3, C, n) if separate else (1, C, n), 7)
    g = R.sample_grads(go, inp, grid, R.BILINEAR, R.ZEROS, False, separate=separate, point_image=ids)
    gi, gg = ops.triplane_sample_ex_bwd(_d(go), _d(inp), _d(grid), separate, _d(ids), True, True)
    _hold(f"ex bwd separate={separate} grad_input", gi, g["grad_input"], g["gi_S"], g["gi_k"])
    _hold(f"ex bwd separate={separate} grad_grid", gg, g["grad_grid"], g["gg_S"], g["gg_k"])
    assert not _h(gg)[0, off].any()
    # without point_image: batch 2, the planes apart
    if separate:
        grid2, inp2 = R.structured_grid(7, 5, 2, 19), R.random_f32((2, 3 * C, 7, 5), 8)
        go2 = R.random_f32((2, 3, C, grid2.shape[1]), 9)
        _hold("ex fwd separate, batch 2", ops.triplane_sample_ex_fwd(_d(inp2), _d(grid2), separate=True),
              *R.sample(inp2, grid2, R.BILINEAR, R.ZEROS, False, separate=True))
        g = R.sample_grads(go2, inp2, grid2, R.BILINEAR, R.ZEROS, False, separate=True)
        gi, gg = ops.triplane_sample_ex_bwd(_d(go2), _d(inp2), _d(grid2), True, None, True, True)
        _hold("ex bwd separate, batch 2 grad_input", gi, g["grad_input"], g["gi_S"], g["gi_k"])
        _hold("ex bwd separate, batch 2 grad_grid", gg, g["grad_grid"], g["gg_S"], g["gg_k"])


# ------------------------------------------------------------------------------------------ backward
def _backward_case(ops, name, inp, grid, go, padding, align, ws):
    g = R.sample_grads(go, inp, grid, R.BILINEAR, padding, align)
    args = (_d(go)[..., None], _d(inp), _d(grid)[:, :, None], 0, padding, align)
    worst = [0.0, 0.0]
    for need_input, need_grid in ((True, True), (True, False), (False, True)):
        gi, gg = ops.triplane_sample_bwd(*args, need_input, need_grid, use_workspace=ws)
        assert (gi is None) == (not need_input) and (gg is None) == (not need_grid)
        tag = f"{name} needs=({int(need_input)},{int(need_grid)})"
        if need_input:
            worst[0] = max(worst[0], _hold(tag + " grad_input", gi, g["grad_input"], g["gi_S"], g["gi_k"]))
        if need_grid:
            worst[1] = max(worst[1], _hold(tag + " grad_grid", gg, g["grad_grid"], g["gg_S"], g["gg_k"]))
    return worst


@pytest.mark.parametrize("n", [1, 33, 64, 65, 1037, None])
@pytest.mark.parametrize("H,W", [(5, 70), (24, 40), (1, 7)])
def test_sampler_backward_fast_path_on_decisions(ops, H, W, n):
    """sample_bwd_cl32 + unpack_add_kernel (+ pack_kernel<32> for grad_grid): C = 32 with the workspace, batch 2, all six
    padding / align_corners settings, need_input and need_grid each alone and together; n around the 64 points of a
    workgroup and the 2 points of a wave instruction, and the whole structured list (n None).
    worst: 0.562 grad_input (texels with m = 2: 2 roundings per term and 1 addition of the k = 5 counted), 0.005 grad_grid."""
    C = 32
    grid = R.structured_grid(H, W, 2, 23, n)
    inp, go = R.random_f32((2, 3 * C, H, W), 10), R.random_f32((2, C, grid.shape[1]), 11)
    for padding, align in OPTIONS:
        _backward_case(ops, f"bwd cl32 {H}x{W} n={grid.shape[1]} {PADS[padding]} align={align}", inp, grid, go, padding, align, True)


@pytest.mark.parametrize("C", [1, 5, 8, 32])
@pytest.mark.parametrize("H,W", [(5, 70), (1, 7)])
def test_sampler_backward_direct_on_decisions(ops, C, H, W):
    """sample_bwd_direct, bilinear, without the workspace: C = 1, 5, 8 and 32 on the same options.
    worst: 0.560 grad_input (m = 2, as on the fast path), 0.178 grad_grid."""
    grid = R.structured_grid(H, W, 2, 29)
    inp, go = R.random_f32((2, 3 * C, H, W), 12), R.random_f32((2, C, grid.shape[1]), 13)
    for padding, align in OPTIONS:
        _backward_case(ops, f"bwd direct C={C} {H}x{W} {PADS[padding]} align={align}", inp, grid, go, padding, align, False)


@pytest.mark.parametrize("ws", [True, False])
def test_sampler_backward_contention_on_one_footprint(ops, ws):
    """4096 + 37 points per image, all inside ONE 2 x 2 footprint of each 4 x 4 plane: every texel of it receives 4133
    atomic additions per channel, and sample_bwd_cl32's two-points-per-wave layout is full. The bound uses each texel's own
    m and S: (3 + m) * 2^-24 = 2.5e-4 of S at m = 4133, which one contribution lost in a thousand (4 of a texel's, ~1e-3 of S)
    exceeds (tests/test_sampler_reference_cpu.py shows it).
    worst: 0.001 grad_input, 0.010 grad_grid."""
    C, H, W, n = 32, 4, 4, 4096 + 37
    rng = np.random.default_rng(31)
    grid = rng.uniform(-0.24, 0.24, (2, n, 3)).astype(np.float32)          # source index in (1.02, 1.98) on every axis
    inp, go = R.random_f32((2, 3 * C, H, W), 14), R.random_f32((2, C, n), 15)
    g = R.sample_grads(go, inp, grid, R.BILINEAR, R.ZEROS, False)
    assert set(np.unique(g["gi_m"])) == {0, n}
    _backward_case(ops, f"contention ws={ws}", inp, grid, go, R.ZEROS, False, ws)


# ------------------------------------------------------------------------------------------ deformation-field producer
@pytest.mark.parametrize("H,W", [(5, 7), (3, 3), (1, 9), (32, 40)])
def test_warp_on_decisions_and_tails(ops, H, W):
    """warp_fwd_kernel / warp_bwd_kernel: H * W no multiple of 32 (the forward's `t >= hw` return) nor of 8 (the backward's
    clamped tail lanes inside the wave-wide DPP sum), batch 2. Flows: exact integers and half-integers (texel centres
    and edges), some pointing out of the plane on each side, otherwise 3 * randn. Forward, g_src, g_flow, need_src False.
    worst: 0.472 forward, 0.540 g_src (m = 2), 0.011 g_flow."""
    B, C = 2, 32
    rng = np.random.default_rng(H * W)
    flow = (3.0 * rng.standard_normal((B, 6, H, W))).astype(np.float32)
    kind = rng.integers(0, 8, flow.shape)
    flow = np.where(kind == 0, np.rint(flow), flow)
    flow = np.where(kind == 1, np.rint(flow) + 0.5, flow)
    flow = np.where(kind == 2, flow - (max(H, W) + 2), flow)
    flow = np.where(kind == 3, flow + (max(H, W) + 2), flow).astype(np.float32)
    src, go = R.random_f32((3, H, W, C), 16), R.random_f32((B, 3, H, W, C), 17)
    out = ops.triplane_warp_fwd(_d(src)[None], _d(flow))
    _hold(f"warp fwd {H}x{W}", out, *R.warp(src, flow))
    g = R.warp_grads(go, src, flow)
    gs, gf = ops.triplane_warp_bwd(_d(go), _d(src)[None], _d(flow))
    _hold(f"warp g_src {H}x{W}", gs, g["g_src"], g["gs_S"], g["gs_k"])
    _hold(f"warp g_flow {H}x{W}", gf, g["g_flow"], g["gf_S"], g["gf_k"])
    only = ops.triplane_warp_bwd(_d(go), _d(src)[None], _d(flow), need_src=False)
    assert only[0] is None
    _hold(f"warp g_flow alone {H}x{W}", only[1], g["g_flow"], g["gf_S"], g["gf_k"])


# ------------------------------------------------------------------------------------------ ray sampler
def _mask_noise(B, h, w, seed, levels=None, all_negative=False):
    rng = np.random.default_rng(seed)
    # the largest value 0.25: under any window, the whole image included, dilated mask + noise still crosses zero
    mask = rng.choice(np.asarray([-1.5, -0.75, -0.25, 0.0, 0.25], dtype=np.float32), (B, h, w), p=[0.5, 0.3, 0.1, 0.07, 0.03])
    if all_negative:
        mask = -2.0 - np.abs(mask)
    noise = rng.uniform(-1.0, 1.0, (B, h * w)).astype(np.float32)
    if levels:
        noise = (np.floor(noise * levels / 2) * 2 / levels).astype(np.float32)
    noise[noise == 0] = 0.0          # no -0.0
    return mask.astype(np.float32), noise


def _check_topk(name, ids, score, thr, k):
    """ids (B, k) against the referee's scores: k distinct in-range ids; every pixel above the threshold present; no
    selected pixel below it -> per image (selected ties, all ties), flat indices ascending."""
    ids = _h(ids)
    assert ids.dtype == np.int64 and ids.shape == (score.shape[0], k)
    out = []
    for b in range(score.shape[0]):
        sel = np.sort(ids[b])
        assert sel[0] >= 0 and sel[-1] < score.shape[1] and (np.diff(sel) > 0).all(), f"{name}[{b}]: ids repeat or leave the image"
        chosen = np.zeros(score.shape[1], dtype=bool)
        chosen[sel] = True
        assert chosen[score[b] > thr[b]].all(), f"{name}[{b}]: a pixel above the threshold is missing"
        assert not chosen[score[b] < thr[b]].any(), f"{name}[{b}]: a pixel below the threshold was selected"
        out.append((np.nonzero(chosen & (score[b] == thr[b]))[0], np.nonzero(score[b] == thr[b])[0]))
    return out


@pytest.mark.parametrize("B,h,w,k,radius", [(1, 1, 1, 1, 0), (2, 3, 257, 1, 128), (1, 300, 5, 1500, 64), (3, 40, 56, 100, 0),
                                            (1, 40, 56, 2239, 5), (1, 9, 9, 20, 128)])
def test_ray_sampler_against_the_referee(ops, B, h, w, k, radius):
    """window_max_kernel<true|false> + topk_select_kernel: masks of mixed sign and noise in [-1, 1), so scores cross zero
    (order_key's sign branch); k == 1, k == n, k == n - 1; radius 0, the maximum 128, and larger than the image; w = 257
    (one output past a 256-wide segment), the 1 x 1 image and a 300 x 5 one. Each case also with every score negative."""
    for all_negative in (False, True):
        mask, noise = _mask_noise(B, h, w, h * w + k, all_negative=all_negative)
        score, thr = R.dilate_topk(mask, noise, k, radius)
        assert h * w == 1 or ((score < 0).any() and (all_negative or (score > 0).any()))
        assert not all_negative or (score < 0).all()
        ids = ops.mask_dilate_topk(_d(mask), _d(noise), k, radius)
        _check_topk(f"topk {B}x{h}x{w} k={k} r={radius} negative={all_negative}", ids, score, thr, k)


@pytest.mark.parametrize("B,h,w,radius", [(3, 40, 56, 0), (1, 40, 56, 5), (2, 3, 257, 1)])
def test_ray_sampler_ties_take_the_lowest_flat_indices(ops, B, h, w, radius):
    """The documented tie rule: among pixels whose key equals the threshold, the lowest flat indices, while the ties fit the
    1024-entry buffer. Noise quantised to 8 levels on a 5-valued mask: 2 to 1000 pixels share the threshold, and k is set
    so that only some of them are wanted."""
    mask, noise = _mask_noise(B, h, w, 41 + radius, levels=8)
    score, _ = R.dilate_topk(mask, noise, 1, radius)
    values, counts = np.unique(score[0], return_counts=True)
    pick = [i for i in range(len(values)) if all(2 <= int((score[b] == values[i]).sum()) <= 1000 for b in range(B))]
    level = values[pick[len(pick) // 2]]
    for wanted in (1, None):            # one of the ties, and all but one
        ks = [int((score[b] > level).sum()) + (wanted or int((score[b] == level).sum()) - 1) for b in range(B)]
        for b in range(B):              # k is per call: one image at a time
            sc, thr = R.dilate_topk(mask[b:b + 1], noise[b:b + 1], ks[b], radius)
            assert thr[0] == level
            ids = ops.mask_dilate_topk(_d(mask[b:b + 1]), _d(noise[b:b + 1]), ks[b], radius)
            (sel, ties), = _check_topk(f"ties {h}x{w} image {b}", ids, sc, thr, ks[b])
            need = ks[b] - int((sc[0] > level).sum())
            assert 0 < need < len(ties) <= 1000
            assert np.array_equal(sel, ties[:need]), f"image {b}: ties {sel.tolist()} are not the lowest {need} of {ties.tolist()}"


def test_ray_sampler_more_ties_than_the_buffer_holds(ops):
    """More than 1024 pixels share the threshold (constant noise on a flat region): the kernel documents `any of them`, so
    only the set property is asserted."""
    B, h, w, k, radius = 2, 40, 56, 700, 3
    mask, _ = _mask_noise(B, h, w, 43)
    noise = np.full((B, h * w), -0.125, dtype=np.float32)
    score, thr = R.dilate_topk(mask, noise, k, radius)
    ids = ops.mask_dilate_topk(_d(mask), _d(noise), k, radius)
    for sel, ties in _check_topk("ties beyond the buffer", ids, score, thr, k):
        assert len(ties) > 1024
