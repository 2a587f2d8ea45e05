"""GPU tests of libenarf_pgrad.so (pgrad_query_kernel, pgrad_finish_kernel) and the interface over it: the gradient of the
articulated query with respect to its sample points and its part frames, held to the float64 referee of
tests/pgrad_reference.py, whose docstring holds the exclusion rule; the bound is tests/grad_referee.py's, every entry to its
own scale. Scene(32, 2): two images with tri-planes and z_rend of their own, 23 parts, points drawn around the part
centres so that most lie in several cubes. A referee is computed once per mode and shared."""
import functools

import numpy as np
import pytest
import torch

import pgrad_reference as PR
from _helpers import DeviceScene, Scene, assert_close
from test_host_cpu import _nerf_cfg

pytestmark = pytest.mark.gpu
N_ALL = 1000
SIZES = (1, 64, 65, 300, 1000)      # a lone lane, a full wave, a wave and one lane, two workgroups (one ragged), four


@functools.lru_cache(maxsize=None)
def _scene():
    sc = Scene(32, 2)
    return sc, DeviceScene(sc)


@functools.lru_cache(maxsize=None)
def _points():
    sc, _ = _scene()
    return PR.scene_points(sc, N_ALL), PR.upstream(sc.B, N_ALL)


@functools.lru_cache(maxsize=None)
def _referee(mode):
    sc, _ = _scene()
    return PR.Referee(sc, _points()[0], mode)


def _kernel(mode, pts, gd, gc):
    from enarf_gan_amd import ops
    _, ds = _scene()
    d = (lambda t: None if t is None else t.contiguous().to(ds.dev))
    out = ops.query_pose_bwd(d(pts), ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, d(gd), d(gc), **PR.MODES[mode][1])
    torch.cuda.synchronize()
    return out


def _run_and_check(mode, n, gd, gc, what):
    ref = _referee(mode)
    pts = _points()[0]
    r = ref.grads(gd, gc, n)
    keep = ref.keep[:, :n]
    g_points, g_parts = _kernel(mode, pts[:, :, :n], None if gd is None else gd[:, :n] * keep,
                                None if gc is None else gc[:, :, :n] * keep[:, None])
    assert g_points.shape == (2, 3, n) and g_parts.shape == (2, 23, 16)
    full = torch.zeros(2, 3, N_ALL)
    full[:, :, :n] = g_points.cpu()
    worst = PR.check({"g_points": full, "g_parts": g_parts.cpu()}, r, what, ("g_points", "g_parts"))
    assert float(g_parts[:, :, 13:].abs().max()) == 0.0
    print(f"{what}: excluded {ref.excluded * 100:.2f} %, worst ratio to the bound {worst}")
    return g_points, g_parts


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", list(PR.MODES))
def test_gradients_match_the_float64_referee(mode, n):
    (gd, gc) = _points()[1]
    g_points, _ = _run_and_check(mode, n, gd, gc, f"{mode}, N = {n}")
    assert float(g_points.abs().max()) > 0.0


@pytest.mark.parametrize("missing", ["g_density", "g_color"])
def test_one_upstream_gradient_missing(missing):
    (gd, gc) = _points()[1]
    _run_and_check("default", 300, None if missing == "g_density" else gd, None if missing == "g_color" else gc,
                   f"{missing} null")


def test_points_outside_every_cube_get_exact_zeros():
    sc, ds = _scene()
    pts = PR.outside_points(sc, 300)
    assert not bool(PR.forward(sc, pts, torch.float32, "default")["decisions"]["valid"].any())
    gd, gc = PR.upstream(sc.B, 300)
    for mode in PR.MODES:
        g_points, g_parts = _kernel(mode, pts, gd, gc)
        assert not bool(g_points.any()) and not bool(g_parts.any()), mode
    from enarf_gan_amd import ops
    g_points, g_parts = ops.query_pose_bwd(pts[:, :, :0].to(ds.dev), ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, None, None)
    assert g_points.shape == (2, 3, 0) and g_parts.shape == (2, 23, 16) and not bool(g_parts.any())     # N = 0: no launch


def test_two_runs_give_equal_bits():
    pts, (gd, gc) = _points()
    for mode in ("default", "multiply_density_with_weight"):
        a, b = _kernel(mode, pts, gd, gc), _kernel(mode, pts, gd, gc)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), mode


def _model(sc):
    from enarf_gan_amd.models.narf import TriPlaneNARF
    m = TriPlaneNARF(_nerf_cfg(origin_location=sc.ol, Nc=24, Nf=32, mlp_mode="f32"), 256, 24, parent=sc.raw["parents"],
                     num_bone_param=23)
    m.register_canonical_pose(sc.raw["canonical_pose"])
    m.load_state_dict({f"mlp.{k}": v for k, v in sc.raw["mlp"].items()}, strict=False)
    return m.cuda().eval()


def _scaled_frames(m, pose_to_camera, bone_length):
    """24 joints -> (part frames with the translation x coordinate_scale, the parts' bone lengths), in torch"""
    pose_parts, bl_parts = m.transform_pose(pose_to_camera, bone_length)
    s = torch.ones(4, 4, device=pose_parts.device)
    s[:3, 3] = m.coordinate_scale
    return pose_parts * s, bl_parts


def test_query_posable_forward_and_pose_gradients():
    """The outputs are query_fwd's bit for bit; the gradients torch carries from the part records to the 24 joints and the
    bone lengths are held to the referee carried through O.transform_pose / O.canonical_scale."""
    from enarf_gan_amd import ops
    sc, ds = _scene()
    n = 300
    pts, (gd, gc) = _points()[0][:, :, :n].contiguous(), PR.upstream(sc.B, n, seed=9)
    ref = PR.Referee(sc, pts, "default", leaves="joints")
    r = ref.grads(gd, gc)
    m = _model(sc)
    a = sc.raw["pose_to_camera"].cuda().requires_grad_(True)
    bl = sc.raw["bone_length"].cuda().requires_grad_(True)
    p = pts.cuda().requires_grad_(True)
    frames, bl_parts = _scaled_frames(m, a, bl)
    mi = {"z": None, "z_rend": sc.raw["z_rend"].cuda(), "bone_length": bl_parts, "tri_plane_feature": ds.tri}
    den, col = m.query_posable(p, frames, mi)
    with torch.no_grad():
        parts = torch.zeros(sc.B, sc.P, 16, device="cuda")
        parts[:, :, :9] = frames[:, :, :3, :3].reshape(sc.B, sc.P, 9)
        parts[:, :, 9:12] = frames[:, :, :3, 3]
        parts[:, :, 12] = (m.canonical_bone_length[:, None] / bl_parts / m.coordinate_scale)[:, :, 0]
        den0, col0 = ops.query_fwd(pts.cuda(), parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, mlp_mode="f32")
    assert torch.equal(den, den0) and torch.equal(col, col0)
    assert float(den.detach().max()) > 0.0
    keep = ref.keep.cuda()
    ((den[:, 0] * gd.cuda() * keep).sum() + (col * gc.cuda() * keep[:, None]).sum()).backward()
    worst = PR.check({"g_points": p.grad.cpu(), "pose_to_camera": a.grad.cpu(), "bone_length": bl.grad.cpu()}, r,
                     "query_posable", ("g_points", "pose_to_camera", "bone_length"))
    print(f"query_posable: excluded {ref.excluded * 100:.2f} %, worst ratio to the bound {worst}")
    assert float(a.grad.abs().max()) > 0.0 and float(bl.grad.abs().max()) > 0.0


def test_query_posable_also_differentiates_the_field():
    """Where the tri-plane and z_rend require gradients too, they receive query_bwd's, as on the existing entry point."""
    sc, ds = _scene()
    n = 300
    pts, (gd, gc) = _points()[0][:, :, :n].contiguous().cuda(), PR.upstream(sc.B, n, seed=9)
    m = _model(sc)
    tri = ds.tri.clone().requires_grad_(True)
    z = sc.raw["z_rend"].cuda().requires_grad_(True)
    frames = sc.pose_scaled.cuda().requires_grad_(True)
    mi = {"z": None, "z_rend": z, "bone_length": sc.bl_parts.cuda(), "tri_plane_feature": tri}
    den, col = m.query_posable(pts, frames, mi)
    ((den[:, 0] * gd.cuda()).sum() + (col * gc.cuda()).sum()).backward()
    with torch.enable_grad():
        tri2 = ds.tri.clone().requires_grad_(True)
        z2 = sc.raw["z_rend"].cuda().requires_grad_(True)
        mi2 = {"z": None, "z_rend": z2, "bone_length": sc.bl_parts.cuda(), "tri_plane_feature": tri2}
        den2, col2 = m.calc_density_and_color_from_camera_coord_v2(pts, sc.pose_scaled.cuda(), None, mi2)
        ((den2[:, 0] * gd.cuda()).sum() + (col2 * gc.cuda()).sum()).backward()
    assert_close(tri.grad.cpu(), tri2.grad.cpu(), "tri-plane gradient", 1e-5)     # query_bwd's atomics: not bit for bit
    assert_close(z.grad.cpu(), z2.grad.cpu(), "z_rend gradient", 1e-5)
    assert frames.grad is not None and float(frames.grad.abs().max()) > 0.0


def test_existing_entry_points_still_raise():
    sc, ds = _scene()
    m = _model(sc)
    pts = _points()[0][:, :, :64].contiguous().cuda()
    mi = {"z": None, "z_rend": sc.raw["z_rend"].cuda(), "bone_length": sc.bl_parts.cuda(), "tri_plane_feature": ds.tri}
    with pytest.raises(NotImplementedError):
        m.calc_density_and_color_from_camera_coord_v2(pts, sc.pose_scaled.cuda().requires_grad_(True), None, mi)
    with pytest.raises(NotImplementedError):
        m.calc_density_and_color_from_camera_coord_v2(pts.clone().requires_grad_(True), sc.pose_scaled.cuda(), None, mi)
    from enarf_gan_amd.libraries.NeRF.rendering import render
    s = sc.raw
    with pytest.raises(NotImplementedError):
        render(m, s["image_coord"][..., :64].contiguous().cuda(), sc.pose_parts.cuda().requires_grad_(True),
               s["inv_intrinsics"].cuda(), Nc=24, Nf=32, model_input=mi)


def test_render_posable_forward_and_pose_gradients():
    """64 rays through the bodies, Nc 24 / Nf 32, given bins. Forward: render()'s outputs on the same bins, to the
    forward parity bound (1e-4 of each output's scale). Backward: the gradients of the part frames and their bone
    lengths against a float64 referee built from the same fine points, O.query and O.composite; a ray is excluded when
    any of its fine points is (pgrad_reference's rule)."""
    from enarf_gan_amd.libraries.NeRF.rendering import render, render_posable
    from oracle import enarf_oracle as O
    sc, ds = _scene()
    s = sc.raw
    m = _model(sc)
    B, n, Nc, Nf = sc.B, 64, 24, 32
    coord = s["image_coord"][..., 32 * 13:32 * 13 + n].contiguous().cuda()
    g = torch.Generator().manual_seed(4)
    bins = torch.rand(B, n, Nf, generator=g).sort(-1).values.cuda()
    gc, gm, gdisp = torch.randn(B, 3, n, generator=g), torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    pp, blp = sc.pose_parts.cuda().requires_grad_(True), sc.bl_parts.cuda().requires_grad_(True)
    mi = {"z": None, "z_rend": s["z_rend"].cuda(), "bone_length": blp, "tri_plane_feature": ds.tri}
    rc, rm, rd = render_posable(m, coord, pp, s["inv_intrinsics"].cuda(), Nc=Nc, Nf=Nf, model_input=mi, bins=bins)
    with torch.no_grad():
        c0, m0, d0 = render(m, coord, pp.detach(), s["inv_intrinsics"].cuda(), Nc=Nc, Nf=Nf,
                            model_input={**mi, "bone_length": blp.detach()}, bins=bins)
    for ours, ref_, what in ((rc, c0, "colour"), (rm, m0, "mask"), (rd, d0, "disparity")):
        assert_close(ours.detach().cpu(), ref_.cpu(), f"render_posable {what} vs render", 1e-4)
    assert float(m0.max()) > 0.5

    pts, fdepth = m.buffers_tensors["fine_points"].cpu(), m.buffers_tensors["fine_depth"][:, 0].cpu()
    ref = PR.Referee(sc, pts, "default", leaves="frames")

    def loss_fn(fw, keep):
        dt = fw["density"].dtype
        c_, m_, d_, _ = O.composite(fw["density"].reshape(B, n, Nf), fw["color"].reshape(B, 3, n, Nf), fdepth.to(dt))
        kr = keep.reshape(B, n, Nf).all(dim=-1).to(dt)
        return (c_ * (gc.to(dt) * kr[:, None])).sum() + (m_ * (gm.to(dt) * kr)).sum() + (d_ * (gdisp.to(dt) * kr)).sum()

    r = ref.grads_of(loss_fn)
    kr = ref.keep.reshape(B, n, Nf).all(dim=-1).float().cuda()
    ((rc * (gc.cuda() * kr[:, None])).sum() + (rm * (gm.cuda() * kr)).sum() + (rd * (gdisp.cuda() * kr)).sum()).backward()
    worst = PR.check({"pose_parts": pp.grad.cpu(), "bl_parts": blp.grad.cpu()}, r, "render_posable", ("pose_parts", "bl_parts"))
    print(f"render_posable: {int((kr == 0).sum())} of {B * n} rays excluded, worst ratio to the bound {worst}")
    assert float(pp.grad.abs().max()) > 0.0 and float(blp.grad.abs().max()) > 0.0


FIT = dict(joint=16, angle=0.1, steps=25, lr=5e-3, n_rays=512, Nc=24, Nf=32, pool=16, gain=4.0)


def _rotation_angle(Ra, Rb):
    return float(torch.acos((((Ra.t() @ Rb).trace() - 1) / 2).clamp(-1, 1)))


def test_fit_pose_descends():
    """One joint turned by 0.1 rad, the target rendered from the true pose with the same z_rend: after FIT["steps"] steps
    the photometric loss of the whole frame and the rotation error of that joint (of its global rotation) are both below
    their starting values; the values reached are printed, not asserted.

    The setting was chosen on the CPU: the same descent (Adam on a PoseCorrection, gradient at fixed sample positions
    through O.query and O.composite in float64, whole 16^2 frame a step). On the synthetic scene as it stands the referee
    alone does NOT descend at lr 5e-3 or 1e-2 (40 steps: loss 0.023 -> 0.025 / 0.064, joint error 0.10 -> 0.27 / 0.47 rad):
    its feature planes are box-filtered noise with a correlation length of 5 texels (0.04 canonical units), about what 0.1
    rad moves the arm, so the photometric gradient is noise and Adam walks every joint at random. A trained field is
    smooth; with the feature planes averaged over 16 x 16 texels (x 4 to keep their magnitude; the part-probability planes
    untouched) the referee descends at lr 5e-3: loss 0.034 -> 0.0070, joint error 0.100 -> 0.061 rad in 25 steps. Reached on the
    GPU (two runs): frame loss 0.0277 -> 0.0116 / 0.0082, joint error 0.100 -> 0.053 / 0.051 rad."""
    from enarf_gan_amd import ops
    from enarf_gan_amd.models.fit import PoseCorrection, fit_pose
    torch.manual_seed(0)                               # the ray sampler's noise comes from torch's device generator
    sc = Scene(32, 1)
    s = sc.raw
    m = _model(sc)
    feat = torch.nn.functional.avg_pool2d(s["tri_plane"][:1, :96], FIT["pool"])
    feat = torch.nn.functional.interpolate(feat, size=s["tri_plane"].shape[-2:], mode="bilinear", align_corners=False) * FIT["gain"]
    with torch.no_grad():
        m.tri_plane.copy_(torch.cat([feat, s["tri_plane"][:1, 96:]], dim=1))
    pose, bl, z_rend, inv_K = (s[k].cuda() for k in ("pose_to_camera", "bone_length", "z_rend", "inv_intrinsics"))
    turn = PoseCorrection(1, s["parents"]).cuda()
    with torch.no_grad():
        turn.rotation[0, FIT["joint"]] = torch.tensor([0.0, 0.0, FIT["angle"]])
        start = turn(pose)

    def frame(p):
        with torch.no_grad():
            c, a, _ = m.render_entire_img(p, inv_K, None, z_rend, bl, render_size=32, Nc=FIT["Nc"], Nf=FIT["Nf"])
        return (c + (-1.0) * (1 - a))[None], a[None]

    def frame_loss(p):
        c, a = frame(p)
        lc, lm = ops.photometric_loss(None, c.reshape(1, 3, -1), a.reshape(1, -1), target.reshape(1, 3, -1), target_mask.reshape(1, -1))
        return float(lc + lm)

    target, target_mask = frame(pose)
    assert float(target_mask.max()) > 0.5
    j = FIT["joint"]
    loss0, err0 = frame_loss(start), _rotation_angle(pose[0, j, :3, :3], start[0, j, :3, :3])
    fitted, history = fit_pose(m, target, target_mask, start, bl, (None, z_rend), inv_K, steps=FIT["steps"], lr=FIT["lr"],
                               n_rays=FIT["n_rays"], Nc=FIT["Nc"], Nf=FIT["Nf"])
    assert history.is_cuda and history.shape == (FIT["steps"],) and bool(torch.isfinite(history).all())
    loss1, err1 = frame_loss(fitted), _rotation_angle(pose[0, j, :3, :3], fitted[0, j, :3, :3])
    print(f"fit_pose: frame loss {loss0:.6g} -> {loss1:.6g}, joint {j} rotation error {err0:.4f} -> {err1:.4f} rad, "
          f"sampled loss {float(history[0]):.6g} -> {float(history[-1]):.6g}")
    assert abs(err0 - FIT["angle"]) < 1e-3
    assert loss1 < loss0 and err1 < err0
    assert all(p.requires_grad for p in m.parameters())


def test_train_step_posable_moves_the_field_and_the_poses():
    """One step of the single-scene training loop with pose refinement: both the field's parameters and the correction's
    residuals receive a finite gradient and move; train_step's own path is untouched."""
    from enarf_gan_amd import ops
    from enarf_gan_amd.models.dso import train_step_posable
    from enarf_gan_amd.models.fit import PoseCorrection
    from enarf_gan_amd.models.generator import DSONARFGenerator
    from test_host_cpu import Cfg
    sc = Scene(32, 2)
    s = sc.raw
    gen = DSONARFGenerator(Cfg(use_triplane=True, ray_batchsize=128, nerf_params=_nerf_cfg(Nc=24, Nf=32, mlp_mode="f32")), 32, 24,
                           s["parents"], 23)
    gen.register_canonical_pose(s["canonical_pose"])
    with torch.no_grad():
        gen.nerf.tri_plane.copy_(s["tri_plane"][:1])
    gen = gen.cuda()
    g = torch.Generator().manual_seed(1)
    mask = torch.zeros(2, 32, 32)
    mask[:, 6:26, 10:22] = 1
    batch = {"img": torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, "mask": mask, "pose_3d": s["pose_to_camera"],
             "frame_time": torch.tensor([0.1, 0.7]), "bone_length": s["bone_length"],
             "intrinsics": torch.inverse(s["inv_intrinsics"]), "frame_idx": torch.tensor([3, 1])}
    batch = {k: v.cuda() for k, v in batch.items()}
    corr = PoseCorrection(5, s["parents"]).cuda()
    opt, popt = torch.optim.SGD(gen.parameters(), lr=1e-3), torch.optim.SGD(corr.parameters(), lr=1e-3)
    before = gen.nerf.tri_plane.detach().clone()
    lc, lm = train_step_posable(gen, ops.photometric_loss, batch, opt, -1.0, corr, popt)
    assert lc.is_cuda and bool(torch.isfinite(lc)) and bool(torch.isfinite(lm))
    assert bool(torch.isfinite(corr.rotation.grad).all()) and float(corr.rotation.grad[[3, 1]].abs().max()) > 0
    assert not bool(corr.rotation.grad[[0, 2, 4]].any()) and float(corr.rotation.detach()[[3, 1]].abs().max()) > 0
    assert not torch.equal(before, gen.nerf.tri_plane.detach())
