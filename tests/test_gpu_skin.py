"""GPU tests of libenarf_skin.so and the interface over it: the skin weights of vertices (skin_weights_kernel<4>, <8>) and
linear-blend posing (skin_pose_kernel<4>, <8>) against tests/skin_reference.py, whose docstring holds the ambiguity rule.

Bounds. Validity bits and the fallback part of an unowned vertex are compared bit for bit (the contract of the parity
tests). On unambiguous vertices the kept raw weights (normalised weight x the referee's kept sum S) are within 1e-4 (the
project's parity bound; raw weights have scale <= 1), the normalised weights and kept_mass within 2e-4 / S; the kept set may
differ only on ambiguous vertices, which are capped at 1 % of the vertices with more than K valid parts. Posed coordinates
equal the float64 referee rounded to fp32 or lie one fp32 step from it (fp64 arithmetic on both sides, one rounding at the
end: the bound geom_buffers_kernel is held to). Scenes are Scene(16, 1): 256^2 planes, 23 or 24 parts."""
import functools

import numpy as np
import pytest
import torch

import geom_reference as GR
import seg_reference as SR
import skin_reference as SK
from _helpers import DeviceScene, Scene

pytestmark = pytest.mark.gpu
TOL = 1e-4
CASES = {"center_fixed": ("center_fixed", {}), "center+head": ("center+head", {}),
         "clamp_mask": ("center_fixed", {"clamp_mask": True}), "uniform_part_weight": ("center_fixed", {"uniform_part_weight": True})}


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(ol):
    sc = Scene(16, 1, ol, 20)
    return sc, DeviceScene(sc)


@functools.lru_cache(maxsize=None)
def _referee(name, K):
    ol, flags = CASES[name]
    sc, _ = _scene(ol)
    pts = SK.scene_points(sc)
    return pts, SK.weights(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], K, **flags)


def _weights(ds, pts, K, **kw):
    """ops.skin_weights on (1, 3, N) points of the scaled camera space (coordinate_scale 1: the points are scaled already)"""
    from enarf_gan_amd import ops
    return ops.skin_weights(pts[0].t().contiguous().to(ds.dev), ds.parts, ds.cpose, ds.tri, max_influences=K,
                            coordinate_scale=1.0, return_valid_bits=True, **kw)


def _far_points(sc, n=300):
    """(1, 3, n) points 50 units from the first part: outside every cube"""
    far = torch.randn(1, 3, n, generator=torch.Generator().manual_seed(0))
    return (far / far.norm(dim=1, keepdim=True) * 50.0 + sc.pose_scaled[0, 0, :3, 3][None, :, None]).contiguous()


def _check_weights(got, ref, P, K, what, cap):
    joints, weights, mass, bits = (_np(t) for t in got)
    N = len(ref["n_valid"])
    assert joints.shape == (N, K) and joints.dtype == np.int32 and weights.shape == (N, K) and mass.shape == (N,)
    assert np.array_equal(bits.view(np.uint32), SR.bits(torch.from_numpy(ref["valid"])[None])[0]), f"{what}: validity bits"
    un = ref["unowned"]
    assert np.array_equal(joints[un, 0], ref["fallback"][un]) and (joints[un, 1:] == -1).all(), f"{what}: fallback parts"
    assert (weights[un, 0] == 1).all() and (weights[un, 1:] == 0).all() and (mass[un] == 0).all()
    assert ((joints >= 0).sum(axis=1) == np.where(un, 1, np.minimum(ref["n_valid"], K))).all(), f"{what}: used slots"
    assert (weights[joints < 0] == 0).all()
    clear = ~ref["ambiguous"] & ~un
    S = ref["kept_sum"][clear]
    d_got, d_ref = SK.dense(joints, weights, P)[clear], SK.dense(ref["joints"], ref["weights"], P)[clear]
    same_set = ((d_got > 0) == (d_ref > 0)).all(axis=1)
    e_norm = np.abs(d_got - d_ref).max(axis=1)
    e_raw = e_norm * S
    e_mass = np.abs(mass[clear] - ref["kept_mass"][clear])
    many, amb = int((ref["n_valid"] > K).sum()), int(ref["ambiguous"].sum())
    top = lambda a: float(a.max()) if a.size else 0.0                      # V = 1 may leave no unambiguous owned vertex
    print(f"{what}: raw weight err {top(e_raw):.2e}, normalised err {top(e_norm):.2e} (S >= {float(S.min()) if S.size else 0:.3f}), "
          f"kept_mass err {top(e_mass):.2e}, {amb} ambiguous of {many} with more than K valid parts, {int(un.sum())} unowned, "
          f"{int((~same_set).sum())} kept sets differ on the unambiguous ones")
    assert same_set.all(), what
    assert (e_raw <= TOL).all() and (e_norm <= 2 * TOL / S).all() and (e_mass <= 2 * TOL / S).all(), what
    if cap:
        assert amb <= SK.MAX_AMBIGUOUS * many, (what, amb, many)
    return many


# ------------------------------------------------------------------------------------------------ weights on scene points
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_weights_on_scene_points_match_the_referee(name, K):
    ol, flags = CASES[name]
    sc, ds = _scene(ol)
    pts, ref = _referee(name, K)
    got = _weights(ds, pts, K, **flags)
    _, _, qbits = ds.query(pts, need_valid=True, need_color=False, **flags)
    assert np.array_equal(_np(got[3]).view(np.uint32), _np(qbits).view(np.uint32)[0]), "validity bits against query_fwd"
    assert int(ref["unowned"].sum()) == 34 and ref["kept_sum"][~ref["unowned"]].min() >= (0.126 if not flags.get("uniform_part_weight") else 0)
    if name == "uniform_part_weight":
        # one constant weight, exact ties everywhere: the tie rule alone decides, so the kept parts are the K lowest valid
        # parts exactly; n w and w / (n w) are exact in fp64, so the weights are fl32(1 / n) and the mass fl32(K / n)
        joints, weights, mass, _ = (_np(t) for t in got)
        own = ~ref["unowned"]
        assert np.array_equal(joints[own], ref["joints"][own])
        n = np.minimum(ref["n_valid"], K)[own]
        assert np.array_equal(weights[own], np.where(ref["joints"][own] >= 0, (1.0 / n).astype(np.float32)[:, None], np.float32(0)))
        assert np.array_equal(mass[own], (n / ref["n_valid"][own]).astype(np.float32))
        un = ref["unowned"]
        assert np.array_equal(joints[un, 0], ref["fallback"][un]) and (weights[un, 0] == 1).all() and (mass[un] == 0).all()
        assert int((ref["n_valid"] > K).sum()) > 1000
        return
    many = _check_weights(got, ref, sc.P, K, f"{name} K={K}", cap=True)
    assert many > 1000, "the scene exercises the cut-off"
    if (name, K) == ("center_fixed", 4):
        assert many == 2982


# --------------------------------------------------------------------------------------------- weights on explicit vertices
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000])
def test_weights_on_explicit_vertices_tails_and_both_layouts(V, K):
    from enarf_gan_amd import ops
    sc, ds = _scene("center_fixed")
    g = torch.Generator().manual_seed(V)
    centres = sc.pose_scaled[0, torch.randint(0, sc.P, (V,), generator=g), :3, 3].t()                 # (3, V)
    pts = (centres + torch.randn(3, V, generator=g) * 0.4)[None].contiguous()
    ref = SK.weights(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], K)
    a = _weights(ds, pts, K)
    _check_weights(a, ref, sc.P, K, f"V={V} K={K}", cap=False)
    soa = pts[0].contiguous().to(ds.dev)                                                               # (3, V), read as a view
    b = ops.skin_weights(soa.t(), ds.parts, ds.cpose, ds.tri, max_influences=K, return_valid_bits=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # camera units: the kernel's own multiplication by coordinate_scale is the fp32 product the host makes
    cam = (torch.randn(V, 3, generator=g) * 0.3).to(ds.dev)
    c = ops.skin_weights(cam, ds.parts, ds.cpose, ds.tri, max_influences=K, coordinate_scale=3.0, return_valid_bits=True)
    d = ops.skin_weights(cam * 3.0, ds.parts, ds.cpose, ds.tri, max_influences=K, return_valid_bits=True)
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    without = ops.skin_weights(cam, ds.parts, ds.cpose, ds.tri, max_influences=K, coordinate_scale=3.0)
    assert len(without) == 3 and all(torch.equal(x, y) for x, y in zip(without, c))


@pytest.mark.parametrize("K", [4, 8])
def test_weights_on_cube_faces_and_far_outside_every_cube(K):
    """points whose local or canonical coordinates sit on, or a few ulp either side of, a cube face (built as
    test_gpu_parity builds them), points far outside every cube (each follows its nearest part), and no points"""
    from enarf_gan_amd import ops
    from test_gpu_parity import _cube_face_points
    sc, ds = _scene("center_fixed")
    pts = _cube_face_points(sc, per=2000, seed=5)
    ref = SK.weights(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], K)
    local, canonical = SK.O.to_local_and_canonical(pts, sc.pose_scaled, sc.scale, sc.cpose)
    on_face = ((canonical.abs().amax(dim=2) - 1).abs() < 1e-6) | ((local.abs().amax(dim=2) - 1).abs() < 1e-6)
    valid = torch.from_numpy(ref["valid"])[None]
    assert int((on_face & valid).sum()) > 100 and int((on_face & ~valid).sum()) > 100
    _check_weights(_weights(ds, pts, K), ref, sc.P, K, f"faces K={K}", cap=False)
    far = _far_points(sc)
    fref = SK.weights(far, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], K)
    assert fref["unowned"].all() and len(np.unique(fref["fallback"])) >= 3
    joints, weights, mass, bits = _weights(ds, far, K)
    assert np.array_equal(_np(joints)[:, 0], fref["fallback"]) and bool((joints[:, 1:] == -1).all())
    assert bool((weights[:, 0] == 1).all()) and bool((weights[:, 1:] == 0).all()) and bool((mass == 0).all()) and bool((bits == 0).all())
    empty = ops.skin_weights(torch.zeros(0, 3, device=ds.dev), ds.parts, ds.cpose, ds.tri, max_influences=K, return_valid_bits=True)
    assert [tuple(t.shape) for t in empty] == [(0, K), (0, K), (0,), (0,)] and empty[0].dtype == torch.int32


@pytest.mark.parametrize("K", [4, 8])
def test_skin_and_seg_agree_on_membership(K):
    """skin_weights_kernel and seg_label_kernel walk the parts through the one definition in csrc/enarf_parts.h: on the same
    300 points (a full 256-lane block and a tail: scene points, points on and a few ulp off the cube faces, points outside
    every cube) their validity bits are equal, the strongest influence is the label (both let the lowest index win a tie),
    and a point no part contains has label -1 and kept mass 0"""
    from enarf_gan_amd import ops
    from test_gpu_parity import _cube_face_points
    sc, ds = _scene("center_fixed")
    scene, faces = SK.scene_points(sc), _cube_face_points(sc, per=2000, seed=5)
    pick = lambda p, n: p[0, :, torch.linspace(0, p.shape[2] - 1, n).long()]
    v = torch.cat([pick(scene, 180), pick(faces, 80), _far_points(sc)[0, :, :40]], dim=1).t().contiguous().to(ds.dev)
    assert v.shape == (300, 3)
    for flags in ({}, {"uniform_part_weight": True}):
        joints, _, mass, bits = ops.skin_weights(v, ds.parts, ds.cpose, ds.tri, max_influences=K, coordinate_scale=1.0,
                                                 return_valid_bits=True, **flags)
        label, _, _, seg_bits = ops.part_labels(v, ds.parts, ds.cpose, ds.tri, points_last=True, return_valid_bits=True, **flags)
        label, seg_bits = label.reshape(-1), seg_bits.reshape(-1)
        assert torch.equal(bits, seg_bits), flags
        owned = bits != 0
        assert int(owned.sum()) >= 100 and int((~owned).sum()) >= 40, "both kinds of point are present"
        assert torch.equal(joints[owned, 0], label[owned]), flags
        assert bool((label[~owned] == -1).all()) and bool((mass[~owned] == 0).all()), flags


@pytest.mark.parametrize("K", [4, 8])
def test_six_coincident_parts_bit_for_bit(K):
    """six coincident part frames over identical mask planes: six equal raw weights, so the tie rule alone orders them.
    4 w, 6 w and their quotients are exact or correctly rounded in fp64, so every output is known to the bit"""
    from enarf_gan_amd import ops
    from test_skin_cpu import _coincident
    pose, scale, cpose, tri = _coincident()
    parts = torch.zeros(1, 6, 16)
    parts[0, :, :9] = torch.eye(3).reshape(9)
    parts[0, :, 12] = scale[0]
    g = torch.Generator().manual_seed(3)
    v = (torch.rand(300, 3, generator=g) * 1.8 - 0.9).cuda()
    joints, weights, mass, bits = ops.skin_weights(v, parts.cuda(), cpose.cuda(), tri.cuda(), max_influences=K, return_valid_bits=True)
    assert bool((bits == 63).all())
    if K == 4:
        assert np.array_equal(_np(joints), np.tile(np.arange(4, dtype=np.int32), (300, 1)))
        assert bool((weights == 0.25).all()) and np.array_equal(_np(mass), np.full(300, np.float32(4 / 6)))
    else:
        assert np.array_equal(_np(joints), np.tile(np.array([0, 1, 2, 3, 4, 5, -1, -1], np.int32), (300, 1)))
        assert np.array_equal(_np(weights), np.tile(np.array([np.float32(1 / 6)] * 6 + [0, 0], np.float32), (300, 1)))
        assert bool((mass == 1).all())
    ref = SK.weights(v.cpu().t()[None].contiguous(), pose, scale, cpose, tri, K)
    assert np.array_equal(_np(joints), ref["joints"]) and np.abs(_np(weights) - ref["weights"]).max() < 1e-7


# ---------------------------------------------------------------------------------------------------------------- posing
def _pose_case(V, P, F, K, seed):
    """random rest and target records (rotations, translations and bone lengths all differ), vertices, joints with unused
    slots and fp32 weights that sum to 1"""
    from test_skin_cpu import _frames
    rng = np.random.default_rng(seed)
    cs = 3.0
    rest = SK.records(_frames(rng, P, 0.4).astype(np.float32)[None], (rng.random((1, P)) + 0.5).astype(np.float32),
                      (rng.random(P) + 0.5).astype(np.float32), cs)
    tgt = SK.records(_frames(rng, F * P, 0.4).astype(np.float32).reshape(F, P, 4, 4), (rng.random((F, P)) + 0.5).astype(np.float32),
                     (rng.random(P) + 0.5).astype(np.float32), cs)
    v = (rng.standard_normal((V, 3)) * 0.5).astype(np.float32)
    joints = np.stack([rng.permutation(P)[:K] for _ in range(V)]).astype(np.int32)
    w = (rng.random((V, K)) + 0.05).astype(np.float32)
    drop = rng.random((V, K)) < 0.3
    drop[:, 0] = False
    joints[drop], w[drop] = -1, 0
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    return v, joints, w, rest, tgt, cs


def _check_posed(got, ref, what):
    """posed vertices against the float64 referee: the referee rounded to fp32, or one fp32 step from it -> the worst step"""
    steps = GR.ulps_from(_np(got), ref)
    assert steps.max() <= 1, (what, float(steps.max()))
    return float(steps.max())


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000])
def test_posing_matches_the_referee_to_one_fp32_step(V, K):
    from enarf_gan_amd import _skin_lib, ops
    worst = 0.0
    for P in (23, 24):
        for F in (1, 2, _skin_lib.FRAMES_PER_GROUP + 1):
            v, joints, w, rest, tgt, cs = _pose_case(V, P, F, K, seed=1000 * V + 10 * P + F)
            dev = [torch.from_numpy(x).cuda() for x in (v, joints, w, rest, tgt)]
            got = ops.skin_pose(*dev, coordinate_scale=cs)
            assert got.shape == (F, V, 3) and got.dtype == torch.float32
            ref = SK.pose(v, joints, w, rest, tgt, cs)
            assert (np.abs(ref - v).max(axis=(1, 2)) > 0.1).all(), "the target poses move the mesh"
            worst = max(worst, _check_posed(got, ref, (P, F)))
            assert torch.equal(got, ops.skin_pose(*dev, coordinate_scale=cs)), "two runs give identical bits"
            soa = dev[0].t().contiguous().t()                              # a (3, V) buffer read as (V, 3)
            assert torch.equal(got, ops.skin_pose(soa, *dev[1:], coordinate_scale=cs))
    print(f"V={V} K={K}: at most {worst:.0f} fp32 step from the referee")


@pytest.mark.parametrize("K", [4, 8])
def test_posing_writes_into_a_slice_and_repeats_bit_for_bit(K):
    from enarf_gan_amd import _skin_lib, ops
    V, P, F = 333, 24, _skin_lib.FRAMES_PER_GROUP + 3
    v, joints, w, rest, tgt, cs = _pose_case(V, P, F, K, seed=K)
    dev = [torch.from_numpy(x).cuda() for x in (v, joints, w, rest, tgt)]
    want = ops.skin_pose(*dev, coordinate_scale=cs)
    assert GR.ulps_from(_np(want), SK.pose(v, joints, w, rest, tgt, cs)).max() <= 1
    big = torch.full((F + 2, V, 3), float("nan"), device="cuda")
    back = ops.skin_pose(*dev, coordinate_scale=cs, out=big[1:F + 1])
    assert back.data_ptr() == big[1].data_ptr() and torch.equal(big[1:F + 1], want)
    assert bool(big[0].isnan().all()) and bool(big[F + 1].isnan().all())
    wide = torch.full((F, 2 * V, 3), float("nan"), device="cuda")          # frames V vertices long, 2 V apart
    ops.skin_pose(*dev, coordinate_scale=cs, out=wide[:, :V])
    assert torch.equal(wide[:, :V], want) and bool(wide[:, V:].isnan().all())
    # the rest pose as the target gives the vertices back within one step; no frames and no vertices launch nothing
    same = ops.skin_pose(*dev[:4], dev[3], coordinate_scale=cs)
    assert GR.ulps_from(_np(same), SK.pose(v, joints, w, rest, rest, cs)).max() <= 1 and np.abs(_np(same)[0] - v).max() < 1e-6
    assert ops.skin_pose(*dev[:4], dev[4][:0], coordinate_scale=cs).shape == (0, V, 3)
    assert ops.skin_pose(dev[0][:0], dev[1][:0], dev[2][:0], dev[3], dev[4], coordinate_scale=cs).shape == (F, 0, 3)
    with pytest.raises(ValueError):
        ops.skin_pose(*dev, coordinate_scale=cs, out=torch.empty(F, V, 4, device="cuda")[:, :, :3])


# -------------------------------------------------------------------------------------------------------------- interface
def _key_poses(s):
    from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle
    first = s["pose_to_camera"][:1]
    return torch.cat([first, rotate_pose_by_angle(first, torch.tensor([0.7]))]).double().cuda()


@functools.lru_cache(maxsize=None)
def _rig(K=4):
    from test_gpu_paint import _model
    gen, s, z, pose, bl, Kmat, mesh = _model()                              # voxel_size 0.05: a 41^3 lattice
    return gen.extract_rigged_mesh(pose, z, bl, **mesh, max_influences=K, return_colors=True, return_part_labels=True)


def test_rigged_mesh_interface():
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import skin_mesh
    from enarf_gan_amd.libraries.NeRF.rendering import _parts_from_part_poses
    from test_gpu_paint import _model
    gen, s, z, pose, bl, Kmat, mesh = _model()
    nerf, rig = gen.nerf, _rig()
    v, t, labels, colors = gen.extract_mesh(pose, z, bl, **mesh, return_part_labels=True, return_colors=True)
    V, P = len(v), nerf.num_bone
    assert V > 100 and torch.equal(rig.vertices, v) and torch.equal(rig.triangles, t)
    assert torch.equal(rig.labels, labels) and torch.equal(rig.colors, colors)
    assert rig.joints.shape == (V, 4) and rig.joints.dtype == torch.int32 and rig.weights.shape == (V, 4) and rig.kept_mass.shape == (V,)
    assert rig.rest_pose.shape == (1, P, 4, 4) and rig.rest_bone_length.shape == (1, P, 1)
    assert float((rig.weights.sum(dim=1) - 1).abs().max()) < 1e-6 and int(rig.joints.max()) < P
    # the strongest influence is the part that owns the vertex, and a vertex some part contains has a positive kept mass
    top = nerf.part_labels(v, pose, gen._latent_parts(z)[0], bl, truncation_psi=0.4, points_last=True)
    owned = labels >= 0
    agree = (rig.joints[:, 0] == labels)[owned].float().mean()
    assert float(agree) > 0.99 and bool((rig.kept_mass[owned] > 0).all()) and bool((rig.kept_mass[~owned] == 0).all())
    assert torch.equal(top[0][0], labels)
    rig8 = _rig(8)
    assert rig8.joints.shape == (V, 8) and bool((rig8.kept_mass >= rig.kept_mass).all())
    # skin_mesh is ops.skin_pose on the records of the same frames
    poses32 = ops.interpolate_pose(_key_poses(s), s["parents"], 4, False, return_f32=True)[1]
    pose_parts, bl_parts = nerf.transform_pose(poses32, (bl * 1.25).expand(4, -1, -1))
    posed = skin_mesh(nerf, rig, pose_parts, bl_parts)
    rest = _parts_from_part_poses(nerf, rig.rest_pose, rig.rest_bone_length)
    parts = _parts_from_part_poses(nerf, pose_parts, bl_parts)
    assert posed.shape == (4, V, 3)
    assert torch.equal(posed, ops.skin_pose(v, rig.joints, rig.weights, rest, parts, coordinate_scale=float(nerf.coordinate_scale)))
    ref = SK.pose(_np(v), _np(rig.joints), _np(rig.weights), _np(rest), _np(parts), float(nerf.coordinate_scale))
    assert GR.ulps_from(_np(posed), ref).max() <= 1
    # the rest pose with the rest bone lengths gives the mesh back
    back = skin_mesh(nerf, rig, rig.rest_pose, rig.rest_bone_length)
    assert float((back[0] - v).abs().max()) < 1e-6
    assert float((posed[3] - v).abs().max()) > 0.01


def test_mesh_animation_frames_are_single_renders():
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import rasterize_mesh, skin_mesh
    from test_gpu_paint import _model
    gen, s, z, pose, bl, Kmat, mesh = _model()
    nerf, rig = gen.nerf, _rig()
    keys, num, R = _key_poses(s), 4, 96
    frames, poses = gen.render_mesh_animation(rig, keys, bl, Kmat, num=num, loop=False, render_size=R, frames_per_batch=1)
    assert frames.shape == (num, R, R, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    assert torch.equal(poses, ops.interpolate_pose(keys, s["parents"], num, False)) and poses.dtype == torch.float64
    chunked, _ = gen.render_mesh_animation(rig, keys, bl, Kmat, num=num, loop=False, render_size=R, frames_per_batch=3)
    assert torch.equal(chunked, frames), "the bytes do not depend on frames_per_batch"
    pose_parts, bl_parts = nerf.transform_pose(poses.float(), bl.expand(num, -1, -1))
    posed = skin_mesh(nerf, rig, pose_parts, bl_parts)
    for i in range(num):
        f = rasterize_mesh(posed[i], rig.triangles, Kmat, gen.size, R)
        want = ops.shade_fragments(f.pix_to_face, f.bary, f.normals, posed[i], rig.triangles, vertex_colors=rig.colors).image
        assert torch.equal(frames[i], want), f"frame {i}"
    assert not torch.equal(frames[0], frames[3]) and int((frames[0] != 255).sum()) > 50          # the mesh is drawn, and moves
    parts, _ = gen.render_mesh_animation(rig, keys, bl, Kmat, num=2, loop=False, color="parts", lit=False, render_size=R)
    white, _ = gen.render_mesh_animation(rig, keys, bl, Kmat, num=2, loop=False, color=None, render_size=R)
    assert parts.shape == (2, R, R, 3) and not torch.equal(parts[0], frames[0])
    assert torch.equal(white[0], rasterize_mesh(posed[0], rig.triangles, Kmat, gen.size, R).image)
    with pytest.raises(ValueError):
        gen.render_mesh_animation(rig, keys, bl, Kmat, num=2, loop=False, color="texture")
