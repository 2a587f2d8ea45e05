"""CPU checks that every kernel instantiation of libenarf_hip.so is reached by a GPU test. The inventory itself is held
against tests/kernel_coverage.py by tests/test_libraries_cpu.py, as every library's is; here are its size and upfirdn2d's
launch plans (enarf_upfirdn2d_plan, no device needed) over the GPU test matrix, its boundaries and the calls the 2-D
networks make."""
from types import SimpleNamespace

import pytest
import torch

import libraries as L

CUS = 256                  # MI355X


def test_every_built_kernel_instantiation_has_tests():
    assert len(L.kernels("hip")) >= 65


# ------------------------------------------------------------------------------------------------- upfirdn2d plans
def _op():
    from enarf_gan_amd.libraries.custom_stylegan2 import op
    return op


def _gpu_cases():
    """(planes, H, W, kh, kw, up, down, pad) of every upfirdn2d launch the GPU tests in test_gpu_gan2d.py make directly"""
    import test_gpu_gan2d as g
    cases = []
    for up, down, pad in g.UPFIRDN_CASES:
        for H, W in ((9, 13), (64, 64), (33, 130), (128, 128)):
            for kw in (3, 4):
                cases.append((6, H, W, 4, kw, up, down, pad))
    for up, down in ((1, 1), (2, 1), (1, 2)):
        for pad in g.FILTER_PADS:
            for kh, kw in g.FILTER_SIZES:
                for H, W in ((19, 23), (67, 130)):
                    cases.append((6, H, W, kh, kw, up, down, pad))
    cases += [(6, H, W, kh, kw, up, down, pad) for H, W, kh, kw, up, down, pad, _ in g.UPFIRDN_BOUNDARY_CASES]
    cases += [(5, H, W, kh, kw, up, down, pad) for _, H, W, kh, kw, up, down, pad, _ in g.UPFIRDN_PIPELINE_CASES]
    cases += [c[:8] for c in g.UPFIRDN_PIPELINE_CASES]
    return cases


def _tile(plan):
    """output tile (columns, rows) of the plan's instantiation"""
    return {4: (128, 32), 5: (128, 32), 2: (64, 32), 3: (64, 32)}.get(plan["index"], (64, 64))


def test_upfirdn2d_plan_of_the_listed_cases():
    """each boundary / pipeline case of test_gpu_gan2d.py plans the instantiation its table names"""
    import test_gpu_gan2d as g
    op = _op()
    for H, W, kh, kw, up, down, pad, index in g.UPFIRDN_BOUNDARY_CASES:
        assert op.upfirdn2d_plan(6, H, W, kh, kw, up, down, pad, CUS)["index"] == index, (H, W, kh, kw, up, down, pad)
    for planes, H, W, kh, kw, up, down, pad, index in g.UPFIRDN_PIPELINE_CASES:
        p = op.upfirdn2d_plan(planes, H, W, kh, kw, up, down, pad, CUS)
        assert p["index"] == index and p["ppw"] >= 2 and planes % p["ppw"], (planes, H, W, p)


def test_upfirdn2d_gpu_matrix_reaches_every_plan_and_boundary():
    op = _op()
    plans = [(c, op.upfirdn2d_plan(c[0], *c[1:7], pad=c[7], num_cus=CUS)) for c in _gpu_cases()]
    every = set(range(len(op.UPFIRDN2D_KERNELS)))
    assert {p["index"] for _, p in plans if p["ppw"] == 1} == every
    assert {p["index"] for _, p in plans if p["ppw"] >= 2} == every

    def some(what, pred):
        assert any(pred(c, p) for c, p in plans), what
    ext = {4, 6}
    rem = lambda p: (p["OW"] % _tile(p)[0], p["OH"] % _tile(p)[1])          # noqa: E731
    some("a remainder of exactly 1 absorbed", lambda c, p: p["index"] in ext and 1 in (p["ex"], p["ey"]))
    some("a remainder of exactly 8 absorbed", lambda c, p: p["index"] in ext and 8 in (p["ex"], p["ey"]))
    some("a column remainder of 9: not EXT", lambda c, p: p["index"] == 5 and rem(p)[0] == 9 and p["ex"] == 0)
    some("a row remainder of 9: not EXT", lambda c, p: p["index"] in (5, 7) and rem(p)[1] == 9 and p["ey"] == 0)
    for idx in every:          # OW equal to the tile width and one more, in every instantiation's tile
        tw = _tile({"index": idx})[0]
        some(f"OW == {tw} planned by {idx}", lambda c, p: p["index"] == idx and p["OW"] == tw)
    some("OW == 65 (one more than the 64-column tile)", lambda c, p: p["OW"] == 65)
    some("OW == 129 (one more than the 128-column tile)", lambda c, p: p["OW"] == 129)
    some("narrow and tall: OW <= 64, OH in 65..72", lambda c, p: p["OW"] <= 64 and 65 <= p["OH"] <= 72 and p["index"] == 6)
    some("short and wide: OH <= 64, OW in 65..72", lambda c, p: p["OH"] <= 64 and 65 <= p["OW"] <= 72)
    some("planes not divisible by ppw", lambda c, p: p["ppw"] >= 2 and c[0] % p["ppw"] != 0)
    some("more than 65 535 x 8 planes (grid z capped)", lambda c, p: c[0] > 65535 * 8 and p["grid"][2] == 65535)


def test_upfirdn2d_plan_refuses_what_the_launch_refuses():
    op = _op()
    with pytest.raises(NotImplementedError):
        op.upfirdn2d_plan(1, 16, 16, 9, 9, pad=(4, 4))
    with pytest.raises(NotImplementedError):
        op.upfirdn2d_plan(1, 16, 16, 4, 4, up=2, down=2, pad=(2, 1))
    with pytest.raises(ValueError):
        op.upfirdn2d_plan(1, 2, 2, 4, 4, pad=(0, 0))
    with pytest.raises(ValueError):
        op.upfirdn2d_plan(1, 16, 16, 4, 4, pad=(2, 1), num_cus=0)
    p = op.upfirdn2d_plan(6, 128, 128, 4, 4, pad=(2, 2))
    assert (p["OH"], p["OW"], p["ex"], p["ey"], p["grid"]) == (129, 129, 1, 1, (1, 4, 6))


def _network_calls(size=128, batch=32):
    """(planes, H, W, kh, kw, up, down, pads) of every upfirdn2d call Discriminator and the background Generator (plain and
    cropped) make at this size and batch, forward and their adjoints (the backward's calls), recorded with the networks on
    the meta device (shapes only) and the oracle's op standing in for the HIP one"""
    from oracle import gan_ops_oracle as third
    from enarf_gan_amd.libraries.custom_stylegan2 import net
    op = _op()
    calls = []

    def record(x, k, up=1, down=1, pad=(0, 0), gain=1.0):
        pads = tuple(pad) if len(pad) == 4 else (pad[0], pad[1], pad[0], pad[1])
        calls.append((x.shape[0] * x.shape[1], x.shape[2], x.shape[3], k.shape[0], k.shape[1], up, down, pads))
        return third.upfirdn2d(x, k.to(x.dtype), up, down, pad)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(op, "upfirdn2d", record)
        mp.setattr(op, "fused_leaky_relu", third.fused_leaky_relu)
        mp.setattr(net, "fused_leaky_relu", third.fused_leaky_relu)
        with torch.device("meta"):
            net.Discriminator(SimpleNamespace(minibatch_std=True), size=size)(torch.empty(batch, 3, size, size))
            for crop in (False, True):
                net.Generator(size=size, style_dim=64, n_mlp=4, last_channel=3, crop_background=crop)([torch.empty(batch, 64)])
    finally:
        mp.undo()
    out = set()
    for planes, H, W, kh, kw, up, down, pads in calls:
        OH = (H * up + pads[2] + pads[3] - kh) // down + 1
        OW = (W * up + pads[0] + pads[1] - kw) // down + 1
        out.add((planes, H, W, kh, kw, up, down, pads))
        out.add((planes, OH, OW, kh, kw, down, up, op.adjoint_pads(H, W, OH, OW, kh, kw, up, down, pads)))
    return sorted(out)


def test_network_upfirdn2d_plans_are_covered_at_ppw_above_one():
    """the discriminator and background generator at 128 px, batch 32: every plan they make (EXT or not) is run by a GPU case
    of the same instantiation with more than one plane per workgroup"""
    op = _op()
    calls = _network_calls()
    assert len(calls) >= 20
    covered = set()
    for c in _gpu_cases():
        p = op.upfirdn2d_plan(c[0], *c[1:7], pad=c[7], num_cus=CUS)
        if p["ppw"] >= 2:
            covered.add((p["index"], bool(p["ex"]), bool(p["ey"])))
    kinds = set()
    for c in calls:
        p = op.upfirdn2d_plan(c[0], *c[1:7], pad=c[7], num_cus=CUS)
        kinds.add(p["index"])
        assert any(k[0] == p["index"] for k in covered), (c, p)
        if p["ex"] or p["ey"]:
            assert (p["index"], bool(p["ex"]), bool(p["ey"])) in covered or (p["index"], True, True) in covered, (c, p)
    assert {0, 4, 5, 7} <= kinds          # up-sampler, the wide blur with and without the absorbed remainder, the 4 x 4 blur
