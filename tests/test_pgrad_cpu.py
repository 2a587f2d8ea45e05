"""CPU checks around the query's pose gradients: what the referee of tests/pgrad_reference.py accepts and rejects, the
referee against central differences, PoseCorrection, the torch compositing, and the binding's argument errors."""
import numpy as np
import pytest
import torch

import grad_referee as R
import pgrad_reference as PR
from _helpers import Scene
from oracle import enarf_oracle as O

N = 512


@pytest.fixture(scope="module")
def case():
    """Scene(32, 2), 512 points an image around the part centres, the default mode, random upstream gradients"""
    sc = Scene(32, 2)
    pts = PR.scene_points(sc, N)
    gd, gc = PR.upstream(sc.B, N)
    ref = PR.Referee(sc, pts, "default")
    return dict(sc=sc, pts=pts, gd=gd, gc=gc, ref=ref, g=ref.grads(gd, gc))


def _ratios(case, ours):
    g = case["g"]
    return {k: R.bound_ratios(k, ours[k].numpy(), g["g64"][k].numpy(), g["g32"][k].numpy(),
                              draws=[d[k].numpy() for d in g["draws"]]) for k in ("g_points", "g_parts")}


def test_points_lie_in_several_cubes_and_few_are_excluded(case):
    m = case["ref"].f32["decisions"]["valid"].sum(dim=1)
    assert float((m >= 2).float().mean()) > 0.95 and float((m >= 3).float().mean()) > 0.75
    assert case["ref"].excluded <= PR.MAX_EXCLUDED
    assert float(case["g"]["g64"]["g_parts"].abs().max()) > 0


def test_fp32_computations_outside_the_yardstick_pass(case):
    """The same graph in fp32 on inputs moved by up to one ulp with other seeds than the yardstick's draws. A point on which
    such a run takes another discrete decision than float64 is excluded for that run, by the rule (a handful at most)."""
    ref, loss = case["ref"], PR.point_loss(case["gd"], case["gc"])
    for j in (50, 51, 52):
        fw = PR.forward(case["sc"], case["pts"], torch.float32, "default", draw=j)
        keep = ref.keep & ~PR.disagreeing_points(ref.f64["decisions"], fw["decisions"], False)
        assert int((ref.keep & ~keep).sum()) <= 3
        PR.check(PR.grads(fw, loss, keep), ref.grads_of(loss, keep), f"held-out fp32 draw {j}", ("g_points", "g_parts"))


def test_bound_rejects_one_percent_of_points_off_by_one_percent(case):
    sel = torch.rand(case["gd"].shape, generator=torch.Generator().manual_seed(0)) < 0.01
    f = torch.where(sel, torch.tensor(0.99), torch.tensor(1.0))
    ours = PR.grads(case["ref"].f32, PR.point_loss(case["gd"] * f, case["gc"] * f[:, None]), case["g"]["keep"])
    rt = _ratios(case, ours)
    assert rt["g_points"].max() > 10 and (rt["g_points"] > 1).sum() >= 10, (rt["g_points"].max(), (rt["g_points"] > 1).sum())
    with pytest.raises(AssertionError):
        PR.check(ours, case["g"], "1 % of the points off by 1 %", ("g_points",))


def test_bound_rejects_a_dropped_weight_term(case):
    """A backward that treats the part weights as constants (no dw/dc term) fails on the points and on the part frames."""
    fw = PR.forward(case["sc"], case["pts"], torch.float32, "default", drop_w_term=True)
    ours = PR.grads(fw, PR.point_loss(case["gd"], case["gc"]), case["g"]["keep"])
    rt = _ratios(case, ours)
    assert rt["g_points"].max() > 10 and rt["g_parts"].max() > 10, (rt["g_points"].max(), rt["g_parts"].max())


def test_referee_matches_central_differences_on_colour():
    """Central differences of sum(colour * g) in float64 against the referee's autograd, for pose and scale entries. The
    density is left out: MyReLU's backward (activation.py:12-16) passes a negative gradient through the negative region
    with slope 0.1, which is not the derivative of the ReLU it computes, so no difference quotient can reproduce it. An
    entry is used when two step sizes agree, i.e. no point crosses a cube face or a texel edge inside the step."""
    sc = Scene(32, 2)
    n = 128
    pts = PR.scene_points(sc, n, seed=3)
    gc = PR.upstream(sc.B, n, seed=7)[1].double()
    fw = PR.forward(sc, pts, torch.float64, "default")
    g = PR.grads(fw, PR.point_loss(None, gc), torch.ones(sc.B, n, dtype=torch.bool))
    x = PR._inputs(sc, pts, torch.float64)

    def value(pose, scale):
        _, col, _ = O.query(x["points"], pose, scale, sc.cpose.double(), x["tri"], x["weights"])
        return float((col * gc).sum())

    entries = [("pose", (0, 3, 0, 1)), ("pose", (0, 3, 1, 3)), ("pose", (1, 7, 2, 2)), ("pose", (1, 12, 0, 3)),
               ("pose", (0, 16, 2, 0)), ("scale", (0, 3)), ("scale", (1, 12)), ("scale", (0, 9)), ("scale", (1, 18))]
    used = 0
    for name, idx in entries:
        quotients = []
        for h in (1e-6, 5e-7):
            vals = []
            for sgn in (1, -1):
                pose, scale = x["pose_scaled"].clone(), x["scale"].clone()
                (pose if name == "pose" else scale)[idx] += sgn * h
                vals.append(value(pose, scale))
            quotients.append((vals[0] - vals[1]) / (2 * h))
        auto = float(g[name][idx])
        top = max(abs(quotients[0]), abs(auto), 1e-12)
        if abs(quotients[0] - quotients[1]) > 1e-5 * top:
            continue                                    # a point crossed a face or an edge inside the step
        used += 1
        assert abs(quotients[1] - auto) <= 1e-5 * top, (name, idx, quotients, auto)
    assert used >= 5, used


# ---------------------------------------------------------------------------------------------------- PoseCorrection
def _poses(B=3):
    from enarf_gan_amd import synth
    return synth.make_scene(16, B)["pose_to_camera"], synth.SMPL_PARENTS


def _descendants(parents, j):
    out = set()
    for c in range(len(parents)):
        a = c
        while a > 0:
            a = int(parents[a])
            if a == j:
                out.add(c)
                break
    return out


def test_pose_correction_zero_residuals_reproduce_the_pose():
    from enarf_gan_amd.models.fit import PoseCorrection
    pose, parents = _poses()
    c = PoseCorrection(pose.shape[0], parents)
    assert not bool(c.rotation.any()) and not bool(c.translation.any())
    out = c(pose)
    assert out.shape == pose.shape
    assert float((out.detach() - pose).abs().max()) <= 32 * 2 ** -24 * float(pose.abs().max())     # a chain of up to 9 products
    out.sum().backward()
    assert torch.isfinite(c.rotation.grad).all() and torch.isfinite(c.translation.grad).all()
    idx = torch.tensor([2, 0])
    assert torch.equal(c(pose[idx], idx), out[idx])


def test_pose_correction_residual_at_one_joint_moves_exactly_its_descendants():
    from enarf_gan_amd.models.fit import PoseCorrection
    pose, parents = _poses(1)
    c = PoseCorrection(1, parents)
    base = c(pose).detach()
    j = 16                                             # a shoulder: the arm below it follows
    with torch.no_grad():
        c.rotation[0, j] = torch.tensor([0.0, 0.0, 0.3])
    out = c(pose).detach()
    below = _descendants(parents, j)
    assert below and j not in below
    for q in range(24):
        if q in below:
            assert float((out[0, q, :3, 3] - base[0, q, :3, 3]).norm()) > 1e-3, q
        elif q == j:
            assert torch.equal(out[0, q, :3, 3], base[0, q, :3, 3]) and not torch.equal(out[0, q, :3, :3], base[0, q, :3, :3])
        else:
            assert torch.equal(out[0, q], base[0, q]), q
    R_rel = base[0, j, :3, :3].t() @ out[0, j, :3, :3]
    assert abs(float(torch.acos(((R_rel.trace() - 1) / 2).clamp(-1, 1))) - 0.3) < 1e-5
    with torch.no_grad():
        c.rotation.zero_()
        c.translation[0] = torch.tensor([0.1, -0.2, 0.3])
    moved = c(pose).detach()
    assert float((moved[0, :, :3, 3] - base[0, :, :3, 3] - torch.tensor([0.1, -0.2, 0.3])).abs().max()) < 1e-5
    assert float((moved[0, :, :3, :3] - base[0, :, :3, :3]).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ compositing, binding
def test_torch_compositing_matches_the_oracle():
    from enarf_gan_amd.libraries.NeRF.rendering import composite_fine
    g = torch.Generator().manual_seed(2)
    B, n, Nf = 2, 37, 32
    density = torch.rand(B, n, Nf, generator=g) * 30 * (torch.rand(B, n, Nf, generator=g) > 0.4)
    color = torch.rand(B, 3, n, Nf, generator=g) * 2 - 1
    depth = 1.0 + torch.rand(B, n, Nf, generator=g).sort(-1).values * 3
    for dt, scale in ((torch.float32, 1.0), (torch.float64, 0.5)):
        ours = composite_fine(density.to(dt), color.to(dt), depth.to(dt), scale)
        ref = O.composite(density.to(dt), color.to(dt), depth.to(dt), scale)
        for a, b in zip(ours, ref):
            assert torch.equal(a, b)


def _args(B=2, n=10, P=23, H=8, W=8):
    return dict(points=torch.zeros(B, 3, n), parts=torch.zeros(B, P, 16), canonical_pose=torch.zeros(P, 4, 4),
                tri_nchw=torch.zeros(B, 96 + 3 * P, H, W), feat_cl=torch.zeros(B, 3, H, W, 32),
                mlp_pack=torch.zeros(B, 112192, dtype=torch.uint8), g_density=torch.zeros(B, n), g_color=torch.zeros(B, 3, n))


def test_binding_rejects_cpu_tensors_and_wrong_shapes():
    from enarf_gan_amd import _pgrad_lib, ops
    from enarf_gan_amd._loader import EnarfHipError
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.query_pose_bwd(**_args())
    assert _pgrad_lib.check_query_args(*[None if v is None else v.shape for v in _args().values()]) == (2, 10, 23, 8, 8)
    for bad in (dict(points=torch.zeros(2, 10, 3)), dict(parts=torch.zeros(2, 23, 12)), dict(parts=torch.zeros(1, 23, 16)),
                dict(canonical_pose=torch.zeros(24, 4, 4)), dict(tri_nchw=torch.zeros(2, 96 + 3 * 24, 8, 8)),
                dict(tri_nchw=torch.zeros(3, 96 + 3 * 23, 8, 8)), dict(feat_cl=torch.zeros(2, 3, 8, 8, 16)),
                dict(feat_cl=torch.zeros(1, 3, 8, 8, 32)), dict(mlp_pack=torch.zeros(2, 100, dtype=torch.uint8)),
                dict(g_density=torch.zeros(2, 11)), dict(g_color=torch.zeros(2, 10, 3)),
                dict(parts=torch.zeros(2, 33, 16), canonical_pose=torch.zeros(33, 4, 4), tri_nchw=torch.zeros(2, 96 + 99, 8, 8))):
        with pytest.raises(ValueError):
            ops.query_pose_bwd(**{**_args(), **bad})
    assert _pgrad_lib.load().enarf_pgrad_workspace_bytes(2, 23, 1000) == (2 * 4 * 23 * 13 * 8 + 255) // 256 * 256
    assert _pgrad_lib.load().enarf_pgrad_workspace_bytes(2, 23, 0) == 0
