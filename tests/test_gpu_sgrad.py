"""GPU tests of libenarf_sgrad.so and the interface over it: sgrad_composite_bwd_kernel against the float64 numpy
restatement of its contract (tests/sgrad_reference.py) on the shared cases of tests/scene_cases.py, each upstream gradient
alone, `want` subsets on poisoned outputs, determinism, and the entry points above it (ops.scene_composite_posable,
rendering.render_scene_posable, models.fit.fit_scene).

The bound of every comparison of a kernel output with the referee is per entry and no entry is left out: |got -
fp32(ref)| <= one fp32 step at the entry's magnitude (the referee's sum of absolute terms; gradients are signed, so an ulp
of the result would punish cancellation). All of the kernel's arithmetic is fp64: a few thousand roundings of 2^-53 are
about 2^-29 of an fp32 step at that magnitude, so what remains is the one rounding to fp32 on each side."""
import functools

import numpy as np
import pytest
import torch

import scene_cases as SC
import scene_reference as SR
import sgrad_reference as GR

pytestmark = pytest.mark.gpu

NAMES = ("density", "color")


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()       # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def _case(K, Nf, n, F):
    """the shared inputs of a shape, the render_scale it is run at, random upstream gradients, and the referee's
    gradients for all four (computed once)"""
    inputs = SC.case(K, Nf, n, F)
    scale = 0.37 if F == 2 else 1.0
    up = GR.upstream(F, K, n)
    return inputs, scale, up, GR.composite_bwd(*inputs, scale, *up)


def _bwd(inputs, scale, up, want=NAMES, **kw):
    from enarf_gan_amd import ops
    out = ops.scene_composite_bwd(*(_dev(a) for a in inputs), scale, *(_dev(g) for g in up), want=want, **kw)
    torch.cuda.synchronize()
    assert out._fields == NAMES
    return {k: None if getattr(out, k) is None else getattr(out, k).cpu().numpy() for k in NAMES}


def _check(got, ref, what, names=NAMES):
    worst = {k: SR.excess(got[k], ref[k], ref["abs"][k]) for k in names}
    print(f"{what}: " + ", ".join(f"{k} {w.max():.2f} steps" for k, w in worst.items()))
    for k, w in worst.items():
        assert np.isfinite(got[k]).all(), (what, k)
        assert w.max() <= 1, (what, k)


# ------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("K,Nf,n,F", SC.SHAPES)
def test_cases_match_the_referee(K, Nf, n, F):
    """the seven shapes of tests/scene_cases.py (kPer 1, 2, 4 and 8), all four upstream gradients random, render_scale 1
    and, on the two-frame shapes, 0.37; with n = 67 every frame carries the planted rays. Every entry is held to the
    referee; the entries the contract sets to zero are exact zeros"""
    inputs, scale, up, ref = _case(K, Nf, n, F)
    got = _bwd(inputs, scale, up)
    assert got["density"].shape == (F, K, n, Nf) and got["color"].shape == (F, K, 3, n, Nf)
    _check(got, ref, f"K {K} Nf {Nf} n {n} F {F} scale {scale}")
    assert not got["density"][..., Nf - 1].any() and not got["color"][..., Nf - 1].any()
    valid = inputs[3]
    for f in range(F):
        for r in range(n):
            kind = SC.kind_of(r, f, n)
            out = [k for k in range(K) if valid[f, k, r] == 0]
            if kind in SC.SKIPPED_BIT:
                out += [k for k in range(K) if SC.SKIPPED_BIT[kind](K) >> k & 1]
            for k in out:
                assert not got["density"][f, k, r].any() and not got["color"][f, k, :, r].any(), (f, r, kind, k)
    assert np.abs(got["density"]).max() > 0 and np.abs(got["color"]).max() > 0


def test_each_upstream_gradient_alone_and_want_writes_nothing_else():
    """one upstream gradient given and the other three NULL equals the referee with zeros for them; want=("density",)
    or ("color",) into NaN-filled tensors between guard bands overwrites every entry of the wanted one and nothing else"""
    from enarf_gan_amd import ops
    inputs, scale, up, _ = _case(3, 5, 67, 1)
    F, K, n, Nf = inputs[0].shape
    for only in range(4):
        alone = tuple(g if i == only else None for i, g in enumerate(up))
        _check(_bwd(inputs, scale, alone), GR.composite_bwd(*inputs, scale, *alone), f"{GR.UPSTREAM[only]} alone")
    full = _bwd(inputs, scale, up)
    dev, gdev = [_dev(x) for x in inputs], [_dev(g) for g in up]
    shapes = dict(density=(F, K, n, Nf), color=(F, K, 3, n, Nf))
    for want in (("density",), ("color",), ("color", "density")):
        sizes = {k: int(np.prod(shapes[k])) for k in NAMES}
        arena = torch.full((sum(sizes.values()) + 16 * 3,), float("nan"), device="cuda")
        views, at = {}, 16
        for k in NAMES:
            views[k] = arena[at:at + sizes[k]].view(shapes[k])
            at += sizes[k] + 16
        out = ops.scene_composite_bwd(*dev, scale, *gdev, want=want, out={k: views[k] for k in want})
        torch.cuda.synchronize()
        assert all((getattr(out, k) is None) == (k not in want) for k in NAMES)
        for k in want:
            assert getattr(out, k).data_ptr() == views[k].data_ptr()
            assert views[k].cpu().numpy().tobytes() == full[k].tobytes(), (want, k)       # fully overwritten: no NaN left
            views[k].fill_(float("nan"))
        assert torch.isnan(arena).all(), want


def test_two_runs_are_bit_identical_one_frame_and_no_rays():
    from enarf_gan_amd import ops
    for shape in ((5, 13, 67, 2), (3, 5, 67, 1)):
        inputs, scale, up, _ = _case(*shape)
        a, b = _bwd(inputs, scale, up), _bwd(inputs, scale, up)
        for k in NAMES:
            assert a[k].tobytes() == b[k].tobytes(), k
    flat = _bwd(tuple(x[0] for x in inputs), scale, tuple(g[0] for g in up))               # (K, n, Nf) is one frame
    for k in NAMES:
        assert flat[k].shape == a[k].shape[1:] and flat[k].tobytes() == a[k].tobytes(), k
    for F, n in ((1, 0), (0, 4)):
        z = lambda *s: torch.zeros(*s).cuda()
        out = ops.scene_composite_bwd(z(F, 2, n, 4), z(F, 2, n, 4), z(F, 2, 3, n, 4), g_mask=z(F, n))
        assert out.density.shape == (F, 2, n, 4) and out.color.shape == (F, 2, 3, n, 4) and out.color.is_cuda


def test_posable_composite_is_the_forward_and_the_raw_backward():
    """ops.scene_composite_posable: the forward is ops.scene_composite bit for bit, .backward() through it is the raw
    call bit for bit, and ops.scene_composite keeps refusing a density that requires a gradient"""
    from enarf_gan_amd import ops
    inputs, scale, up, _ = _case(5, 13, 67, 2)
    depth, density, color, valid = (_dev(x) for x in inputs)
    density.requires_grad_(True), color.requires_grad_(True)
    plain = ops.scene_composite(depth, density.detach(), color.detach(), valid, render_scale=scale)
    outs = ops.scene_composite_posable(depth, density, color, valid, scale)
    for got, name in zip(outs, ("color", "mask", "disparity", "instance_mass")):
        assert got.requires_grad and torch.equal(got.detach(), getattr(plain, name)), name
    g = [_dev(x) for x in up]
    torch.autograd.backward(outs, g)
    raw = ops.scene_composite_bwd(depth, density.detach(), color.detach(), valid, scale, *g)
    assert torch.equal(density.grad, raw.density) and torch.equal(color.grad, raw.color)
    density.grad = color.grad = None
    outs = ops.scene_composite_posable(depth, density, color, valid, scale)             # a loss on two outputs only
    (outs[1] * g[1]).sum().add((outs[3] * g[3]).sum()).backward()
    raw = ops.scene_composite_bwd(depth, density.detach(), color.detach(), valid, scale, g_mask=g[1], g_instance_mass=g[3])
    assert torch.equal(density.grad, raw.density) and torch.equal(color.grad, raw.color)
    with pytest.raises(NotImplementedError):
        ops.scene_composite(depth, density, color, valid, render_scale=scale)
    with pytest.raises(NotImplementedError):
        ops.scene_composite_posable(depth.clone().requires_grad_(True), density, color, valid, scale)


# ------------------------------------------------------------------------------------------- render_scene_posable
N_RAYS, NC, NF = 64, 24, 32
FIRST_RAY = 32 * 13                   # rows 13 and 14 of the 32 x 32 frame: through the bodies
MAX_EXCLUDED_RAYS = 0.25


def _scene_loss(depth, valid, gc, gm, gd, gi, K, n, Nf):
    """loss_fn(fw, keep) of pgrad_reference.Referee.grads_of: the K images' densities and colours composed ray by ray
    by the torch restatement of the scene composite (test_sgrad_cpu.smooth_ray, float64 whatever the query's dtype),
    times the upstream gradients; a ray is excluded when any fine point of any avatar on it is"""
    from test_sgrad_cpu import smooth_ray
    depth, valid = depth.numpy(), valid.numpy()

    def loss_fn(fw, keep):
        den, col = fw["density"].reshape(K, n, Nf), fw["color"].reshape(K, 3, n, Nf)
        kr = keep.reshape(K, n, Nf).all(dim=-1).all(dim=0)
        total = den.sum().double() * 0
        for r in range(n):
            if not bool(kr[r]):
                continue
            c_, m_, d_, i_ = smooth_ray(depth[:, r], den[:, r], col[:, :, r], valid[:, r], 1.0)
            total = total + (c_ * gc[:, r].double()).sum() + m_ * float(gm[r]) + d_ * float(gd[r]) + (i_ * gi[:, r].double()).sum()
        return total
    return loss_fn


def test_render_scene_posable_two_avatars():
    """The two images of the synthetic scene taken as two avatars in front of the first image's camera, on its 64 rays
    through the bodies, Nc 24 / Nf 32. Forward: render_scene's outputs on the same seed and avatars_per_batch, to the
    forward parity bound (1e-4 of each output's scale). Backward, on given bins: the gradients of both avatars' part
    frames and bone lengths (colour, mask, disparity and instance_mass all carry a random upstream gradient) against
    pgrad_reference's float64 referee on the same fine points, composed by the float64 torch restatement of the
    composite. A ray is excluded when any fine point of either avatar on it is (pgrad_reference's rule); the points are
    those of test_gpu_pgrad's render_posable test (the same march of the two images on the same rays and bins), on
    which the referee (float64 against fp32 and its draws, all on the CPU) excludes 7 of 64 rays, 10.9 %; the cap
    asserted is 25 %: at the 0.35 % of points pgrad_reference's docstring reports, a ray of 2 x 32 points is excluded
    with probability 1 - 0.9965^64 = 20 %. The referee's own cap of 1 % of the points holds as well."""
    import pgrad_reference as PR
    from _helpers import assert_close
    from enarf_gan_amd.libraries.NeRF.rendering import render_scene, render_scene_posable
    from test_gpu_pgrad import _model, _scene
    sc, ds = _scene()
    s = sc.raw
    m = _model(sc)
    K, n, Nc, Nf = 2, N_RAYS, NC, NF
    coord = s["image_coord"][:1, ..., FIRST_RAY:FIRST_RAY + n].contiguous().cuda()
    K_inv = s["inv_intrinsics"][:1].cuda()
    pp, blp = sc.pose_parts.cuda().requires_grad_(True), sc.bl_parts.cuda().requires_grad_(True)
    mi = {"z": None, "z_rend": s["z_rend"].cuda(), "bone_length": blp, "tri_plane_feature": ds.tri}
    for per in (None, 1):
        with torch.no_grad():
            c0, m0, d0 = render_scene(m, coord, pp.detach(), K_inv, Nc=Nc, Nf=Nf, model_input={**mi, "bone_length": blp.detach()},
                                      seed=5, avatars_per_batch=per)
            mass0, inst0 = m.buffers_tensors["instance_mass"], m.buffers_tensors["instance"]
        rc, rm, rd = render_scene_posable(m, coord, pp, K_inv, Nc=Nc, Nf=Nf, model_input=mi, seed=5, avatars_per_batch=per)
        assert rc.shape == (1, 3, n) and rm.shape == (1, n) and rd.shape == (1, n) and rc.requires_grad
        side = m.buffers_tensors
        for ours, ref_, what in ((rc, c0, "colour"), (rm, m0, "mask"), (rd, d0, "disparity"), (side["instance_mass"], mass0, "mass")):
            assert_close(ours.detach().cpu(), ref_.cpu(), f"render_scene_posable {what} vs render_scene", 1e-4)
        assert side["instance_mass"].shape == (1, K, n) and side["instance_mass"].requires_grad
        assert side["instance"].dtype == torch.int32 and side["skipped"].shape == (1, n) and not side["skipped"].any()
        sure = (m0 - 0.5).abs() > 1e-3
        assert torch.equal(side["instance"][sure], inst0[sure])
        assert float(m0.max()) > 0.5 and float(mass0[0, 0].max()) > 0.05 and float(mass0[0, 1].max()) > 0.05   # both are seen

    g = torch.Generator().manual_seed(4)
    bins = torch.rand(K, n, Nf, generator=g).sort(-1).values.cuda()
    gc, gm, gd = torch.randn(3, n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    gi = torch.randn(K, n, generator=g)
    rc, rm, rd = render_scene_posable(m, coord, pp, K_inv, Nc=Nc, Nf=Nf, model_input=mi, bins=bins)
    side = m.buffers_tensors
    pts, fdepth = side["fine_points"].cpu(), side["fine_depth"][:, 0].cpu()
    with torch.no_grad():
        valid = ds.render(s["image_coord"][:1, ..., FIRST_RAY:FIRST_RAY + n].expand(K, -1, -1, -1).contiguous(), Nc, Nf, bins=bins,
                          debug=True).taps["ray_validity"].cpu()
    ref = PR.Referee(sc, pts, "default", leaves="frames")
    r = ref.grads_of(_scene_loss(fdepth, valid, gc, gm, gd, gi, K, n, Nf))
    kr = ref.keep.reshape(K, n, Nf).all(dim=-1).all(dim=0).float()
    excluded = float((kr == 0).float().mean())
    w = kr.cuda()
    ((rc[0] * (gc.cuda() * w)).sum() + (rm[0] * (gm.cuda() * w)).sum() + (rd[0] * (gd.cuda() * w)).sum()
     + (side["instance_mass"][0] * (gi.cuda() * w)).sum()).backward()
    worst = PR.check({"pose_parts": pp.grad.cpu(), "bl_parts": blp.grad.cpu()}, r, "render_scene_posable", ("pose_parts", "bl_parts"))
    print(f"render_scene_posable: {int((kr == 0).sum())} of {n} rays excluded, worst ratio to the bound {worst}")
    assert excluded <= MAX_EXCLUDED_RAYS
    for k in range(K):
        assert bool(torch.isfinite(pp.grad[k]).all()) and float(pp.grad[k].abs().max()) > 0.0, k
        assert bool(torch.isfinite(blp.grad[k]).all()) and float(blp.grad[k].abs().max()) > 0.0, k


def test_one_avatar_scene_and_render_posable_meet_the_same_referee():
    """K = 1: render_scene_posable and render_posable on the same seed fix the same fine points; the pose gradients of
    each are held, each on its own, to one float64 referee (O.query and O.composite on those points) within
    pgrad_reference's bound; they are not compared with each other"""
    import pgrad_reference as PR
    from _helpers import DeviceScene, Scene
    from enarf_gan_amd.libraries.NeRF.rendering import render_posable, render_scene_posable
    from oracle import enarf_oracle as O
    from test_gpu_pgrad import _model
    sc = Scene(32, 1)
    ds, s, m = DeviceScene(sc), sc.raw, _model(sc)
    n, Nc, Nf = N_RAYS, NC, NF
    coord = s["image_coord"][..., FIRST_RAY:FIRST_RAY + n].contiguous().cuda()
    g = torch.Generator().manual_seed(8)
    gc, gm, gd = torch.randn(1, 3, n, generator=g), torch.randn(1, n, generator=g), torch.randn(1, n, generator=g)
    grads, points = {}, {}
    for name, fn in (("render_posable", render_posable), ("render_scene_posable", render_scene_posable)):
        pp, blp = sc.pose_parts.cuda().requires_grad_(True), sc.bl_parts.cuda().requires_grad_(True)
        mi = {"z": None, "z_rend": s["z_rend"].cuda(), "bone_length": blp, "tri_plane_feature": ds.tri}
        out = fn(m, coord, pp, s["inv_intrinsics"].cuda(), Nc=Nc, Nf=Nf, model_input=mi, seed=11)
        points[name] = (m.buffers_tensors["fine_points"].cpu(), m.buffers_tensors["fine_depth"][:, 0].cpu())
        grads[name] = (out, pp, blp)
    assert torch.equal(points["render_posable"][0], points["render_scene_posable"][0])
    pts, fdepth = points["render_posable"]
    with torch.no_grad():
        live = (grads["render_posable"][0][1] != 0).float().cpu()     # a dropped ray is zero on both routes and in the referee
    ref = PR.Referee(sc, pts, "default", leaves="frames")

    def loss_fn(fw, keep):
        dt = fw["density"].dtype
        c_, m_, d_, _ = O.composite(fw["density"].reshape(1, n, Nf), fw["color"].reshape(1, 3, n, Nf), fdepth.to(dt))
        kr = keep.reshape(1, n, Nf).all(dim=-1).to(dt) * live.to(dt)
        return (c_ * (gc.to(dt) * kr[:, None])).sum() + (m_ * (gm.to(dt) * kr)).sum() + (d_ * (gd.to(dt) * kr)).sum()

    r = ref.grads_of(loss_fn)
    kr = (ref.keep.reshape(1, n, Nf).all(dim=-1).float() * live).cuda()
    for name, ((rc, rm, rd), pp, blp) in grads.items():
        ((rc * (gc.cuda() * kr[:, None])).sum() + (rm * (gm.cuda() * kr)).sum() + (rd * (gd.cuda() * kr)).sum()).backward()
        worst = PR.check({"pose_parts": pp.grad.cpu(), "bl_parts": blp.grad.cpu()}, r, name, ("pose_parts", "bl_parts"))
        print(f"{name}, K = 1: {int((kr == 0).sum())} of {n} rays without a gradient, worst ratio to the bound {worst}")
        assert float(pp.grad.abs().max()) > 0.0 and float(blp.grad.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------- fit_scene
FIT = dict(apart=0.3, shift=0.05, steps=25, lr=5e-3, n_rays=512, Nc=24, Nf=32, pool=16, gain=4.0)


def test_fit_scene_descends():
    """Two avatars of the synthetic scene side by side (their roots 0.6 m apart: the arms cross, 12 of 256 pixels of
    the 16^2 frame see both), the second one's root shifted by 5 cm; the target is rendered from the true poses by
    render_scene. After FIT["steps"] steps the photometric loss of the whole frame and the position error of that root
    are both below their starting values; the values reached are printed, not asserted.

    The setting was chosen on the CPU, as test_gpu_pgrad.test_fit_pose_descends chose its own and starting from it (the
    feature planes averaged over 16 x 16 texels, x 4): the same descent with the float64 referee alone - Adam on a
    PoseCorrection(2), the gradient at fixed sample positions through O.query and the float64 torch restatement of the
    composite (test_sgrad_cpu.smooth_ray), the whole 16^2 frame a step. At lr 5e-3 the referee descends: frame loss
    0.0433 -> 0.0128, root error 0.0500 -> 0.0290 m in 25 steps (0.0307, 0.0173, 0.0120, 0.0230 m after 5, 10, 15 and 20
    steps: Adam at this rate overshoots the minimum and comes back, and stays below the start throughout). Reached on
    the GPU (512 sampled rays a step of the 32^2 frame): frame loss 0.0496 -> 0.0090, root error 0.0500 -> 0.0328 m."""
    from _helpers import Scene
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.rendering import render_scene
    from enarf_gan_amd.models.fit import PoseCorrection, fit_scene
    from test_gpu_pgrad import _model
    torch.manual_seed(0)                               # the ray sampler's noise comes from torch's device generator
    sc = Scene(32, 1)
    s = sc.raw
    m = _model(sc)
    feat = torch.nn.functional.avg_pool2d(s["tri_plane"][:1, :96], FIT["pool"])
    feat = torch.nn.functional.interpolate(feat, size=s["tri_plane"].shape[-2:], mode="bilinear", align_corners=False) * FIT["gain"]
    with torch.no_grad():
        m.tri_plane.copy_(torch.cat([feat, s["tri_plane"][:1, 96:]], dim=1))
    K = 2
    pose = s["pose_to_camera"].cuda().repeat(K, 1, 1, 1)
    pose[0, :, 0, 3] -= FIT["apart"]
    pose[1, :, 0, 3] += FIT["apart"]
    bl, z_rend, inv_K = s["bone_length"].cuda().repeat(K, 1, 1), s["z_rend"].cuda().repeat(K, 1), s["inv_intrinsics"][:1].cuda()
    move = PoseCorrection(K, s["parents"]).cuda()
    with torch.no_grad():
        move.translation[1, 0] = FIT["shift"]
        start = move(pose)
    pixels = s["image_coord"][:1].cuda()

    def frame(p):
        with torch.no_grad():
            pp, blp = m.transform_pose(p, bl)
            c, a, _ = render_scene(m, pixels, pp, inv_K, Nc=FIT["Nc"], Nf=FIT["Nf"],
                                   model_input={"z": None, "z_rend": z_rend, "bone_length": blp}, seed=3)
        return (c + (-1.0) * (1 - a[:, None])).reshape(1, 3, 32, 32), a.reshape(1, 32, 32), m.buffers_tensors["instance"].reshape(1, 32, 32)

    def frame_loss(p):
        c, a, _ = frame(p)
        lc, lm = ops.photometric_loss(None, c.reshape(1, 3, -1), a.reshape(1, -1), target.reshape(1, 3, -1), target_mask.reshape(1, -1))
        return float(lc + lm)

    def root_error(p):
        return float((p[1, 0, :3, 3] - pose[1, 0, :3, 3]).norm())

    target, target_mask, target_instance = frame(pose)
    assert float(target_mask.max()) > 0.5 and int((target_instance == 0).sum()) > 20 and int((target_instance == 1).sum()) > 20
    loss0, err0 = frame_loss(start), root_error(start)
    fitted, history = fit_scene(m, target, target_mask, start, bl, (None, z_rend), inv_K, steps=FIT["steps"], lr=FIT["lr"],
                                n_rays=FIT["n_rays"], Nc=FIT["Nc"], Nf=FIT["Nf"])
    assert fitted.shape == (K, 24, 4, 4) and not fitted.requires_grad
    assert history.is_cuda and history.shape == (FIT["steps"],) and bool(torch.isfinite(history).all())
    loss1, err1 = frame_loss(fitted), root_error(fitted)
    print(f"fit_scene: frame loss {loss0:.6g} -> {loss1:.6g}, root error {err0:.4f} -> {err1:.4f} m, "
          f"sampled loss {float(history[0]):.6g} -> {float(history[-1]):.6g}")
    assert abs(err0 - FIT["shift"]) < 1e-4
    assert loss1 < loss0 and err1 < err0
    assert all(p.requires_grad for p in m.parameters())
    # the instance term: three steps with the owner map as a target run, and move the history
    _, with_owner = fit_scene(m, target, target_mask, start, bl, (None, z_rend), inv_K, steps=3, lr=FIT["lr"], n_rays=FIT["n_rays"],
                              Nc=FIT["Nc"], Nf=FIT["Nf"], target_instance=target_instance, instance_weight=2.0)
    assert bool(torch.isfinite(with_owner).all()) and float(with_owner[0]) > 0


def test_generator_scene_posable():
    """TriNARFGenerator.render_scene_posable at size 32 with K = 2: the whole frame over a black background is
    rendering.render_scene's colour over it, on the same seed and on the part frames the method itself forms
    (transform_pose in torch; gen.render_scene takes them from ops.prepare, whose last-bit differences move a few
    samples across a cube's face), to the forward parity bound; both avatars' joints receive a finite non-zero gradient,
    and given pixels take a number or one colour a ray as their background"""
    from _helpers import assert_close
    from enarf_gan_amd.libraries.NeRF.rendering import render_scene
    from test_gpu_anim import _generator
    S = 32
    gen, s, z = _generator(S, 24, 32)
    first = s["pose_to_camera"][:1]
    second = first.clone()
    second[:, :, 0, 3] += 0.4
    second[:, :, 2, 3] += 0.3
    pose = torch.cat([first, second]).cuda().requires_grad_(True)
    z2 = torch.cat([z, torch.randn(1, z.shape[1], generator=torch.Generator().manual_seed(3)).cuda()])
    bl = s["bone_length"][:1].cuda().repeat(2, 1, 1)
    K_inv = torch.linalg.inv_ex(s["intrinsics"][:1].cuda().float()).inverse
    _, pixels = gen.ray_sampler(S, S, 1, device="cuda")
    with torch.no_grad():                              # render_scene on the part frames the method itself forms
        z_nerf, z_render, _ = gen._latent_parts(z2)
        pose_parts, bl_parts = gen.nerf.transform_pose(pose.detach(), bl)
        mi = {"z": z_nerf, "z_rend": z_render, "bone_length": bl_parts, "truncation_psi": 0.4}
        c0, m0, _ = render_scene(gen.nerf, pixels, pose_parts, K_inv, model_input=mi, seed=9, **gen._samples)
    image, mask = gen.render_scene_posable(pose, bl, z2, K_inv, truncation_psi=0.4, background=-1.0, seed=9)
    assert image.shape == (1, 3, S * S) and mask.shape == (1, S * S) and image.requires_grad and float(m0.max()) > 0.9
    assert_close(image.detach().cpu(), (c0 + (1 - m0[:, None]) * -1.0).cpu(), "generator scene, image", 1e-4)
    assert_close(mask.detach().cpu(), m0.cpu(), "generator scene, mask", 1e-4)
    (image.sum() + mask.sum()).backward()
    for k in (0, 1):
        assert bool(torch.isfinite(pose.grad[k]).all()) and float(pose.grad[k].abs().max()) > 0, k
    some = pixels[..., 300:364].contiguous()
    given = torch.rand(1, 3, 64, generator=torch.Generator().manual_seed(1)).cuda()
    part, part_mask = gen.render_scene_posable(pose, bl, z2, K_inv, truncation_psi=0.4, background=given, pixels=some, seed=9)
    assert part.shape == (1, 3, 64) and part_mask.shape == (1, 64)
    with pytest.raises(ValueError, match="background"):
        gen.render_scene_posable(pose, bl, z2, K_inv, pixels=some)
    with pytest.raises(AssertionError):
        gen.render_scene_posable(pose, bl, z, K_inv)
