"""GPU tests of libenarf_seg.so and the interface over it: the part that owns a sample point (seg_label_kernel) and the
semantic map of a march (seg_composite_kernel) against tests/seg_reference.py, whose docstring holds the ambiguity rule.

Bounds: validity bits are compared bit for bit (the contract of the parity tests); weights, colours and masses within
1e-4 (the project's parity bound: part weights, palette entries and compositing weights all have scale <= 1); labels and
part maps are equal wherever the referee's decision is not within the ambiguity margin, and such cases are capped.
Scenes are Scene(16, B): 256 rays x (48 + 64) samples an image on 256^2 planes."""
import functools

import numpy as np
import pytest
import torch

import seg_reference as R
from _helpers import DeviceScene, Scene

pytestmark = pytest.mark.gpu
TOL = 1e-4
Nc, Nf = 48, 64
CASES = {"b1": (1, "center_fixed", {}), "b2": (2, "center_fixed", {}), "p24": (1, "center+head", {}),
         "clamp": (1, "center_fixed", {"clamp_mask": True}), "uniform": (1, "center_fixed", {"uniform_part_weight": True})}


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(B, ol):
    sc = Scene(16, B, ol, 20)
    return sc, DeviceScene(sc)


@functools.lru_cache(maxsize=None)
def _case(name):
    """one march of the case's scene with its taps, the kernel's labels of its fine samples, and the referee's"""
    from enarf_gan_amd import ops
    B, ol, flags = CASES[name]
    sc, ds = _scene(B, ol)
    coord = sc.raw["image_coord"]
    out = ds.render(coord, Nc, Nf, None, seed=1, debug=True, **flags)
    t = out.taps
    got = ops.part_labels_on_rays(coord.to(ds.dev), ds.inv_K, t["depth_min"], t["depth_max"], t["bins"], ds.parts, ds.cpose,
                                  ds.tri, return_valid_bits=True, **flags)
    pts = R.ray_points(coord, sc.raw["inv_intrinsics"], t["depth_min"].cpu(), t["depth_max"].cpu(), t["bins"].cpu())
    ref = R.labels(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], **flags)
    return sc, ds, out, got, pts, ref


def _check_labels(got, ref, what, cap=True):
    """kernel (label, top, second) as flat numpy arrays against a labels_from_weights dict"""
    label, top, second = (np.asarray(x).reshape(ref["label"].shape) for x in got)
    e_top, e_sec = np.abs(top - ref["top"]).max(), np.abs(second - ref["second"]).max()
    multi, amb = int((ref["n_valid"] > 1).sum()), int(ref["ambiguous"].sum())
    clear = ~ref["ambiguous"]
    wrong = int((label != ref["label"])[clear].sum())
    print(f"{what}: top err {e_top:.2e}, second err {e_sec:.2e}, {amb} ambiguous of {multi} samples with >= 2 valid parts, "
          f"{wrong} wrong labels on the unambiguous ones")
    assert e_top <= TOL and e_sec <= TOL, (what, e_top, e_sec)
    assert wrong == 0, what
    if cap:
        assert amb <= R.MAX_AMBIGUOUS_SAMPLES * multi, (what, amb, multi)


# ------------------------------------------------------------------------------------- labels on the fine samples of a march
@pytest.mark.parametrize("name", list(CASES))
def test_labels_on_the_fine_samples_of_a_march(name):
    sc, ds, out, (label, top, second, bits), pts, ref = _case(name)
    B = sc.B
    assert label.shape == (B, 256, Nf) and label.dtype == torch.int32 and bits.dtype == torch.int32
    ours = _np(bits).view(np.uint32).reshape(B, -1)
    assert np.array_equal(ours, R.bits(ref["valid"])), "validity bits against the referee"
    flags = CASES[name][2]
    _, _, qbits = ds.query(pts, need_valid=True, need_color=False, **flags)
    assert np.array_equal(ours, _np(qbits).view(np.uint32)), "validity bits against query_fwd at the same points"
    assert int((ref["n_valid"] > 1).sum()) > 1000 and int((ref["label"] >= 0).sum()) > 3000
    if name == "uniform":        # one constant weight: the lowest valid part everywhere, no exclusions
        assert np.array_equal(_np(label).reshape(B, -1), R.lowest_set_bit(ours))
        assert np.array_equal(_np(label).reshape(B, -1), ref["label"])
        w = np.float32(1.0) / np.float32(sc.P)
        assert np.array_equal(_np(top).reshape(B, -1), np.where(ours != 0, w, np.float32(0)))
        assert np.array_equal(_np(second).reshape(B, -1), np.where(ref["n_valid"] > 1, w, np.float32(-1)))
        return
    _check_labels((_np(label), _np(top), _np(second)), ref, name)
    assert len(np.unique(ref["label"])) >= 8


# ------------------------------------------------------------------------------------------------------- explicit points
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000])
def test_explicit_points_tails_and_both_layouts(M):
    from enarf_gan_amd import ops
    sc, ds = _scene(2, "center_fixed")
    g = torch.Generator().manual_seed(M)
    centres = sc.pose_scaled[:, torch.randint(0, sc.P, (M,), generator=g), :3, 3].permute(0, 2, 1)        # (2, 3, M)
    pts = (centres + torch.randn(2, 3, M, generator=g) * 0.4).contiguous()
    ref = R.labels(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"])
    dev = pts.to(ds.dev)
    a = ops.part_labels(dev, ds.parts, ds.cpose, ds.tri, return_valid_bits=True)
    assert [tuple(t.shape) for t in a] == [(2, M)] * 4
    assert np.array_equal(_np(a[3]).view(np.uint32), R.bits(ref["valid"]))
    _check_labels([_np(t) for t in a[:3]], ref, f"M={M}", cap=False)
    last = dev.permute(0, 2, 1).contiguous()                                                              # (2, M, 3)
    b = ops.part_labels(last, ds.parts, ds.cpose, ds.tri, points_last=True, return_valid_bits=True)
    c = ops.part_labels(dev.permute(0, 2, 1), ds.parts, ds.cpose, ds.tri, points_last=True, return_valid_bits=True)   # a view
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    # (M, 3): one image
    one = ops.part_labels(last[1], ds.parts[1:], ds.cpose, ds.tri[1:], points_last=True, return_valid_bits=True)
    for x, y in zip(a, one):
        assert y.shape == (1, M) and torch.equal(x[1:], y)


def test_no_points_and_points_outside_every_cube():
    from enarf_gan_amd import ops
    sc, ds = _scene(1, "center_fixed")
    empty = ops.part_labels(torch.zeros(1, 3, 0, device=ds.dev), ds.parts, ds.cpose, ds.tri, return_valid_bits=True)
    assert [tuple(t.shape) for t in empty] == [(1, 0)] * 4 and empty[0].dtype == torch.int32
    assert ops.part_labels(torch.zeros(0, 3, device=ds.dev), ds.parts, ds.cpose, ds.tri, points_last=True)[0].shape == (1, 0)
    g = torch.Generator().manual_seed(0)
    far = torch.randn(1, 3, 300, generator=g)
    far = far / far.norm(dim=1, keepdim=True) * 50.0 + sc.pose_scaled[0, 0, :3, 3][None, :, None]
    label, top, second, bits = ops.part_labels(far.to(ds.dev), ds.parts, ds.cpose, ds.tri, return_valid_bits=True)
    assert bool((label == -1).all()) and bool((top == 0).all()) and bool((second == -1).all()) and bool((bits == 0).all())


def test_points_on_cube_faces_against_the_referee_and_the_query_kernel():
    """Points whose local or canonical coordinates sit on, or a few ulp either side of, a cube face (built as
    test_gpu_parity builds them), so that validity is decided by the last bit: bits against the referee and query_fwd,
    labels and weights against the referee and against query_fwd(debug=True)'s dbg_weight."""
    from enarf_gan_amd import ops
    from test_gpu_parity import _cube_face_points
    sc, ds = _scene(1, "center_fixed")
    pts = _cube_face_points(sc, per=2000, seed=5)
    ref = R.labels(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"])
    local, canonical = R.O.to_local_and_canonical(pts, sc.pose_scaled, sc.scale, sc.cpose)
    on_face = ((canonical.abs().amax(dim=2) - 1).abs() < 1e-6) | ((local.abs().amax(dim=2) - 1).abs() < 1e-6)
    assert int((on_face & ref["valid"]).sum()) > 100 and int((on_face & ~ref["valid"]).sum()) > 100
    label, top, second, bits = ops.part_labels(pts.to(ds.dev), ds.parts, ds.cpose, ds.tri, return_valid_bits=True)
    ours = _np(bits).view(np.uint32)
    assert np.array_equal(ours, R.bits(ref["valid"]))
    _check_labels((_np(label), _np(top), _np(second)), ref, "faces vs referee", cap=False)
    _, _, qbits, _, dw = ds.query(pts, debug=True)
    assert np.array_equal(ours, _np(qbits).view(np.uint32))
    _check_labels((_np(label), _np(top), _np(second)), R.labels_from_weights(ref["valid"], _np(dw).astype(np.float64)),
                  "faces vs query_fwd's weights", cap=False)


# ------------------------------------------------------------------------------------------------------------- composite
def _check_composite(got, ref, what, cap):
    color, part_map, part_mass = (_np(t) for t in got)
    e_c, e_m = np.abs(color - ref["color"]).max(), np.abs(part_mass - ref["part_mass"]).max()
    clear = ~ref["ambiguous"]
    wrong = int((part_map != ref["part_map"])[clear].sum())
    rays, amb = int(ref["labelled"].sum()), int(ref["ambiguous"].sum())
    print(f"{what}: colour err {e_c:.2e}, mass err {e_m:.2e}, {amb} ambiguous of {rays} labelled rays, {wrong} wrong")
    assert e_c <= TOL and e_m <= TOL and wrong == 0, (what, e_c, e_m, wrong)
    if cap:
        assert rays > 50 and amb <= R.MAX_AMBIGUOUS_RAYS * rays, (what, amb, rays)


@pytest.mark.parametrize("name", ["b1", "b2"])
def test_composite_of_a_march_matches_the_referee(name):
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.rendering import semantic_palette
    sc, ds, out, (label, _, _, _), _, ref = _case(name)
    pal = semantic_palette(sc.P)
    got = ops.semantic_composite(label, out.fine_weights, pal.to(ds.dev))
    assert got[0].shape == (sc.B, 3, 256) and got[1].shape == (sc.B, 256) and got[1].dtype == torch.int32
    want = R.composite(_np(label), _np(out.fine_weights), pal, ref["ambiguous"].reshape(sc.B, 256, Nf))
    _check_composite(got, want, name, cap=True)
    assert len(np.unique(want["part_map"])) >= 5
    again = ops.semantic_composite(label, out.fine_weights, pal.to(ds.dev))
    assert all(torch.equal(x, y) for x, y in zip(got, again)), "two runs give identical bits"
    if name == "b1":             # the rays a one-image march drops: zero weights -> no part, no mass, no colour
        dropped = out.taps["ray_validity"][0] == 0
        assert 10 < int(dropped.sum()) < 250
        assert bool((out.fine_weights[0, 0][dropped] == 0).all())
        assert bool((got[1][0][dropped] == -1).all()) and bool((got[2][0][dropped] == 0).all())
        assert bool((got[0][0][:, dropped] == 0).all())


@pytest.mark.parametrize("nf", [2, 64, 65, 128])
def test_composite_sample_counts_and_edge_rays(nf):
    """Nf = 2 (one interval), 64 / 65 (the last weighted sample in lane 62 / 63, the closing one in the second slot) and
    128 (two samples a lane); 37 rays x 2 images (not a multiple of the 4 rays of a workgroup); up to 24 distinct labels a
    ray; unlabelled samples, labels outside [0, P), a ray of zero weights and a ray without labels."""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.rendering import semantic_palette
    g = torch.Generator().manual_seed(nf)
    B, n, P = 2, 37, 24
    labels = torch.randint(-1, P, (B, n, nf), generator=g, dtype=torch.int32)
    labels[0, 3] = torch.randint(0, 3, (nf,), generator=g, dtype=torch.int32)           # few parts, large masses
    labels[1, 5, ::2] = 99                                                                # not a part: counts as -1
    w = torch.rand(B, 1, n, nf - 1, generator=g) / nf
    w[0, 0, 7] = 0.0                                                                      # labelled, weightless
    labels[1, 9] = -1                                                                     # weights, no label
    pal = semantic_palette(P)
    got = ops.semantic_composite(labels.cuda(), w.cuda(), pal.cuda())
    want = R.composite(labels.numpy(), w.numpy(), pal)
    _check_composite(got, want, f"Nf={nf}", cap=False)
    for b, r in ((0, 7), (1, 9)):
        assert int(got[1][b, r]) == -1 and float(got[2][b, r]) == 0 and bool((got[0][b, :, r] == 0).all())
    again = ops.semantic_composite(labels.cuda(), w.cuda(), pal.cuda())
    assert all(torch.equal(x, y) for x, y in zip(got, again))


# ------------------------------------------------------------------------------------------------------ public interface
def _model(sc):
    from test_gpu_api import _model as make
    return make(sc, Nc, Nf)


def test_render_entire_img_semantic_map_is_the_composite_of_its_own_taps():
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.rendering import _parts_from_part_poses, semantic_palette
    sc, ds = _scene(1, "center_fixed")
    s = sc.raw
    m = _model(sc)
    args = (s["pose_to_camera"].cuda(), s["inv_intrinsics"].cuda(), None, s["z_rend"].cuda(), s["bone_length"].cuda())
    torch.manual_seed(5)
    color, mask, disp = m.render_entire_img(*args, render_size=16, Nc=Nc, Nf=Nf)
    torch.manual_seed(5)
    sem, smask, sdisp = m.render_entire_img(*args, render_size=16, Nc=Nc, Nf=Nf, semantic_map=True)
    assert sem.shape == (3, 16, 16) and torch.equal(smask, mask) and torch.equal(sdisp, disp)
    assert not torch.equal(sem, color)
    buf = m.buffers_tensors
    assert buf["part_map"].shape == (1, 256) and buf["part_map"].dtype == torch.int32
    assert buf["part_mass"].shape == (1, 256) and buf["part_labels"].shape == (1, 256, Nf)
    pose_parts, bl = m.transform_pose(args[0], args[4])
    idx = torch.arange(256)
    coord = torch.stack([idx % 16 + 0.5, torch.div(idx, 16, rounding_mode="floor") + 0.5, torch.ones(256)])[None].cuda()
    labels, _, _ = ops.part_labels_on_rays(coord, args[1], buf["depth_min"], buf["depth_max"], buf["bins"],
                                           _parts_from_part_poses(m, pose_parts, bl), m.canonical_pose, m.tri_plane.detach())
    assert torch.equal(labels, buf["part_labels"])
    c, pm, mass = ops.semantic_composite(labels, buf["fine_weights"], semantic_palette(sc.P).cuda())
    assert torch.equal(c.reshape(3, 16, 16), sem) and torch.equal(pm, buf["part_map"]) and torch.equal(mass, buf["part_mass"])
    assert int((pm >= 0).sum()) > 50 and len(pm.unique()) >= 5
    # the mass of the dominant part is at most the ray's mask, and a ray with a part has a mask
    assert bool((mass <= smask.reshape(1, -1) + 1e-5).all())
    with torch.enable_grad(), pytest.raises(NotImplementedError):
        m.render_entire_img(*args, render_size=16, Nc=Nc, Nf=Nf, semantic_map=True, no_grad=False)


def test_render_part_map_shapes_and_dtypes():
    from enarf_gan_amd.models.generator import TriNARFGenerator
    from test_host_cpu import Cfg, _nerf_cfg
    sc = Scene(16, 2, "center_fixed", 256)
    s = sc.raw
    gen = TriNARFGenerator(Cfg(z_dim=256, background_ratio=0.7, crop_background=True, pretrained_background=False,
                               nerf_params=_nerf_cfg(constant_triplane=False, Nc=Nc, Nf=Nf)), 16, 24, s["parents"], 23,
                           black_background=True)
    gen.register_canonical_pose(s["canonical_pose"])
    gen.nerf.load_state_dict({f"mlp.{k}": v for k, v in s["mlp"].items()}, strict=False)
    gen = gen.cuda().eval()
    tri_plane = s["tri_plane"].cuda()
    gen.nerf.tri_plane_gen = lambda z_, enc, truncation_psi=1: tri_plane
    z = torch.cat([torch.randn(2, 512, generator=torch.Generator().manual_seed(0)), s["z_rend"]], dim=1).cuda()
    image, part_map, mask = gen.render_part_map(s["pose_to_camera"].cuda(), s["bone_length"].cuda(), z, s["inv_intrinsics"].cuda())
    assert image.shape == (2, 3, 16, 16) and image.dtype == torch.float32
    assert part_map.shape == (2, 16, 16) and part_map.dtype == torch.int32
    assert mask.shape == (2, 16, 16) and mask.dtype == torch.float32
    assert int(part_map.min()) >= -1 and int(part_map.max()) < 23 and int((part_map >= 0).sum()) > 100
    assert bool(((part_map < 0) | (mask > 0)).all()) and float(image.abs().max()) <= 1 + 1e-5
    assert not image.requires_grad


def test_extract_mesh_returns_one_label_per_vertex():
    from enarf_gan_amd.libraries.NARF.mesh_rendering import density_volume, extract_mesh, point_part_labels
    sc, ds = _scene(1, "center_fixed")
    s = sc.raw
    m = _model(sc)
    voxel = 0.125
    center = torch.tensor([0.02, -0.03, 1.0]).reshape(1, 3, 1)
    center[0, :, 0] += sc.pose_parts[0, :, :3, 3].mean(0) - torch.tensor([0.0, 0.0, 1.0])
    mi = {"z": None, "z_rend": s["z_rend"].cuda(), "bone_length": sc.bl_parts.cuda(), "truncation_psi": 1}
    pose = sc.pose_parts.cuda()
    th = float(density_volume(m, pose, center, voxel, mi).max()) * 0.3
    verts, tris = extract_mesh(m, pose, center, voxel, th, mi)
    v2, t2, labels = extract_mesh(m, pose, center, voxel, th, mi, return_part_labels=True)
    assert torch.equal(v2, verts) and torch.equal(t2, tris) and len(tris) > 0
    assert labels.shape == (len(verts),) and labels.dtype == torch.int32
    again = point_part_labels(m, pose, verts, mi, points_last=True)
    assert torch.equal(again[0][0], labels)
    ref = R.labels((verts.cpu() * 3.0).t()[None].contiguous(), sc.pose_scaled, sc.scale, sc.cpose, s["tri_plane"])
    _check_labels([_np(t) for t in again], ref, "mesh vertices", cap=False)
    assert float((labels >= 0).float().mean()) > 0.5
    # the same through the model's entry points (joint poses in)
    margs = (s["pose_to_camera"].cuda(), None, s["z_rend"].cuda(), s["bone_length"].cuda())
    mv, mt = m.extract_mesh(*margs, voxel_size=voxel, mesh_th=th)
    mv2, mt2, ml = m.extract_mesh(*margs, voxel_size=voxel, mesh_th=th, return_part_labels=True)
    assert torch.equal(mv, mv2) and torch.equal(mt, mt2) and ml.shape == (len(mv),)
    mine = m.part_labels(mv, margs[0], None, margs[3], points_last=True)
    assert torch.equal(mine[0][0], ml)
