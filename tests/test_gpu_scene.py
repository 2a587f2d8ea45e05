"""GPU tests of libenarf_scene.so and the interface over it: scene_composite_kernel against the float64 numpy restatement
of its contract (tests/scene_reference.py) on the shared cases of tests/scene_cases.py, determinism and `want` subsets on
poisoned outputs, and the entry points above it (rendering.render_scene, TriNARFGenerator.render_scene and
render_scene_animation) against single-avatar renders.

The bound of every comparison of a kernel output with the referee is per entry: |got - fp32(ref)| <= one fp32 step at the
magnitude of the entry's sum of absolute terms (colours are signed: an ulp of the result would punish cancellation). The
kernel's sums are fp64 sums of at most 512 terms, whose error (512 x 2^-53 of that magnitude, plus the relative error of
exp of an fp64 prefix sum, ~ 2^-53 x the optical depth) is orders below 2^-24 of it; what remains is the one rounding to
fp32 on each side. t, source, instance and skipped are compared for equality."""
import functools

import numpy as np
import pytest
import torch

import scene_cases as SC
import scene_reference as SR

pytestmark = pytest.mark.gpu

FIELDS = ("color", "mask", "disparity", "instance_mass", "instance", "skipped", "t", "source", "weight")
ROUNDED = ("color", "mask", "disparity", "instance_mass", "weight")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def _case(K, Nf, n, F):
    """the shared inputs of a shape, the render_scale it is run at, and the referee's outputs (computed once)"""
    inputs = SC.case(K, Nf, n, F)
    scale = 2.0 if F == 2 else 1.0
    return inputs, scale, SR.composite(*inputs, render_scale=scale)


def _composite(inputs, scale, want=FIELDS, **kw):
    from enarf_gan_amd import ops
    out = ops.scene_composite(*(None if a is None else _dev(a) for a in inputs), render_scale=scale, want=want, **kw)
    torch.cuda.synchronize()
    assert out._fields == FIELDS
    return {k: None if getattr(out, k) is None else getattr(out, k).cpu().numpy() for k in FIELDS}


def _check(got, ref, what):
    """the fields of `got` that are there (every field of FIELDS unless the call's `want` left some out) against the referee"""
    there = lambda k: got.get(k) is not None
    worst = {k: SR.excess(got[k], ref[k], ref["abs"][k]) for k in ROUNDED if there(k)}
    off = {k: int((got[k].astype(np.float64) != ref[k]).sum()) for k in SR.EXACT_OUTPUTS if there(k)}
    print(f"{what}: " + ", ".join(f"{k} {w.max():.2f} steps" for k, w in worst.items()) + "; unequal: "
          + ", ".join(f"{k} {v}" for k, v in off.items()))
    assert all(got[k].dtype == np.int32 for k in ("instance", "skipped", "source") if there(k))
    for k, v in off.items():
        assert v == 0, (what, k)
    for k, w in worst.items():
        assert w.max() <= 1, (what, k)


# ------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("K,Nf,n,F", SC.SHAPES)
def test_cases_match_the_referee(K, Nf, n, F):
    """the seven shapes of tests/scene_cases.py; with n = 67 every frame carries the planted rays (interleaved and disjoint
    ranges, tied lists, repeated depths, a last-ulp inversion, zero density, an opaque first segment, invalid avatars, a
    NaN depth, a negative density, a zero depth), frame 1 five rays further on"""
    inputs, scale, ref = _case(K, Nf, n, F)
    got = _composite(inputs, scale)
    _check(got, ref, f"K {K} Nf {Nf} n {n} F {F}")
    assert (got["mask"] >= 0).all() and (got["mask"] <= 1).all() and (got["instance"] < K).all()
    kinds = set()
    for f in range(F):
        for r in range(n):
            kind = SC.kind_of(r, f, n)
            kinds.add(kind)
            assert got["skipped"][f, r] == (SC.SKIPPED_BIT[kind](K) if kind in SC.SKIPPED_BIT else 0), (f, r, kind)
            if kind in ("all_invalid", "dropped"):
                assert got["mask"][f, r] == 0 and got["disparity"][f, r] == 0 and not got["color"][f, :, r].any()
                assert got["instance"][f, r] == -1 and (got["source"][f, r] == -1).all() and np.isinf(got["t"][f, r]).all()
                assert not got["weight"][f, r].any() and not got["instance_mass"][f, :, r].any()
            if kind == "zero_density":
                assert got["mask"][f, r] == 0 and got["instance"][f, r] == -1 and np.isfinite(got["t"][f, r]).all()
            if kind == "opaque_start":
                assert got["weight"][f, r, 0] == 1 and not got["weight"][f, r, 1:].any() and got["mask"][f, r] == 1
            if kind == "inversion":
                assert (np.diff(got["t"][f, r]) >= 0).all() and (got["weight"][f, r] >= 0).all()
    assert n == 1 or kinds == set(SC.PLANTED) | {"random_validity"}


def test_one_frame_without_its_axis_and_no_rays():
    """(K, n, Nf) inputs are one frame and the outputs lose the axis too; no validity bytes means every avatar is screened;
    n = 0 and F = 0 return empty tensors"""
    from enarf_gan_amd import ops
    (depth, density, color, valid), scale, ref = _case(3, 5, 67, 1)
    framed = _composite((depth, density, color, valid), scale)
    flat = _composite((depth[0], density[0], color[0], valid[0]), scale)
    for k in FIELDS:
        assert flat[k].shape == framed[k].shape[1:] and flat[k].tobytes() == framed[k].tobytes(), k
    open_ = _composite((depth, density, color, None), scale)
    _check(open_, SR.composite(depth, density, color, None, render_scale=scale), "no validity bytes")
    assert (open_["skipped"] != framed["skipped"]).any()                 # the dropped ray's zeros are screened now
    for F, n in ((1, 0), (0, 4)):
        out = ops.scene_composite(torch.zeros(F, 2, n, 4).cuda(), torch.zeros(F, 2, n, 4).cuda(), torch.zeros(F, 2, 3, n, 4).cuda(),
                                  want=FIELDS)
        assert out.color.shape == (F, 3, n) and out.instance.shape == (F, n) and out.t.shape == (F, n, 8) and out.mask.is_cuda


def test_two_calls_are_bit_identical_and_want_writes_nothing_else():
    from enarf_gan_amd import ops
    inputs, scale, _ = _case(5, 13, 67, 2)
    a, b = _composite(inputs, scale), _composite(inputs, scale)
    for k in FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k
    dev = [_dev(x) for x in inputs]
    F, K, n, Nf = inputs[0].shape
    shapes = dict(color=(F, 3, n), mask=(F, n), disparity=(F, n), instance_mass=(F, K, n), instance=(F, n), skipped=(F, n),
                  t=(F, n, K * Nf), source=(F, n, K * Nf), weight=(F, n, K * Nf))
    ints = ("instance", "skipped", "source")
    for want in (("mask",), ("color", "instance"), ("t", "source"), ("weight", "skipped", "instance_mass"), ("disparity",)):
        # every output is given, poisoned, in one allocation with a guard band on both sides of each; only `want` may change
        sizes = {k: int(np.prod(shapes[k])) * 4 for k in FIELDS}
        arena = torch.full((sum(sizes.values()) + 64 * (len(FIELDS) + 1),), 0xA5, dtype=torch.uint8, device="cuda")
        views, at = {}, 64
        for k in FIELDS:
            views[k] = arena[at:at + sizes[k]].view(torch.int32 if k in ints else torch.float32).view(shapes[k])
            at += sizes[k] + 64
        out = ops.scene_composite(*dev, render_scale=scale, want=want, out={k: views[k] for k in want})
        torch.cuda.synchronize()
        assert all((getattr(out, k) is None) == (k not in want) for k in FIELDS)
        before = arena.cpu().numpy().copy()
        for k in want:
            assert getattr(out, k).data_ptr() == views[k].data_ptr()
            assert views[k].cpu().numpy().tobytes() == a[k].tobytes(), (want, k)
            views[k].view(-1).view(torch.uint8).fill_(0xA5)
        torch.cuda.synchronize()
        assert (arena.cpu().numpy() == 0xA5).all() and (before != 0xA5).any(), want


# ------------------------------------------------------------------------------------------------- render_scene
S, NC, NF = 32, 16, 16


@functools.lru_cache(maxsize=None)
def _narf():
    """the synthetic scene at 32 x 32 rays with its renderer (Nc 16, Nf 16, fp32 MLP): (model, scene, part frames
    (1, P, 4, 4), model_input of one avatar, image_coord, inv_intrinsics)"""
    from _helpers import Scene
    from enarf_gan_amd.models.narf import TriPlaneNARF
    from test_host_cpu import _nerf_cfg
    sc = Scene(S, 1, "center_fixed", 256)
    s = sc.raw
    m = TriPlaneNARF(_nerf_cfg(origin_location=sc.ol, Nc=NC, Nf=NF, mlp_mode="f32"), 256, 24, parent=s["parents"], num_bone_param=23)
    m.register_canonical_pose(s["canonical_pose"])
    m.load_state_dict({f"mlp.{k}": v for k, v in s["mlp"].items()}, strict=False)
    m = m.cuda().eval()
    mi = {"z": None, "z_rend": s["z_rend"].cuda(), "bone_length": sc.bl_parts.cuda(), "tri_plane_feature": s["tri_plane"].cuda()}
    return m, sc, sc.pose_parts.cuda(), mi, s["image_coord"].cuda(), s["inv_intrinsics"].cuda()


def _moved(pose_parts, x=0.0, z=0.0):
    """the part frames translated rigidly in camera space (metres)"""
    out = pose_parts.clone()
    out[:, :, 0, 3] += x
    out[:, :, 2, 3] += z
    return out


def _single(m, coord, pose, K_inv, mi, seed):
    from enarf_gan_amd.libraries.NeRF.rendering import render
    with torch.no_grad():
        return render(m, coord, pose, K_inv, Nc=NC, Nf=NF, model_input=mi, seed=seed)


def _pair(mi):
    """model_input of two avatars of the same identity (one shared tri-plane)"""
    return {**mi, "z_rend": mi["z_rend"].repeat(2, 1), "bone_length": mi["bone_length"].repeat(2, 1, 1)}


def test_one_avatar_is_render():
    """K = 1: the scene composed from the march's taps is the march's own image on the same seed, to the forward parity
    bound (1e-4 of each output's scale, tests/test_gpu_parity.py)"""
    from _helpers import assert_close
    from enarf_gan_amd.libraries.NeRF.rendering import render_scene
    m, sc, pose, mi, coord, K_inv = _narf()
    c0, m0, d0 = _single(m, coord, pose, K_inv, mi, 5)
    c1, m1, d1 = render_scene(m, coord, pose, K_inv, Nc=NC, Nf=NF, model_input=mi, seed=5)
    assert c1.shape == (1, 3, S * S) and m1.shape == (1, S * S) and d1.shape == (1, S * S) and float(m0.max()) > 0.5
    for ours, ref, what in ((c1, c0, "colour"), (m1, m0, "mask"), (d1, d0, "disparity")):
        print(f"render_scene K = 1, {what}: worst entry {assert_close(ours.cpu(), ref.cpu(), what, 1e-4):.3e} of the scale")
    side = m.buffers_tensors
    assert side["instance_mass"].shape == (1, 1, S * S) and side["avatar_masks"].shape == (1, 1, S * S)
    assert_close(side["avatar_masks"][0].cpu(), m0.cpu(), "the avatar's own mask", 1e-4)
    assert_close(side["instance_mass"][0].cpu(), m0.cpu(), "instance mass of the one avatar", 1e-4)
    assert not side["skipped"].any() and side["instance"].dtype == torch.int32
    sure = (m0 - 0.5).abs() > 1e-3
    assert torch.equal(side["instance"][sure], torch.where(m0 >= 0.5, 0, -1).int()[sure])


def test_avatars_side_by_side_are_the_sum_of_their_renders():
    """two avatars moved back and apart so that no pixel sees both, marched one a batch: the scene is the sum of the two
    single renders to the parity bound, and the instance map names each on its own support"""
    from _helpers import assert_close
    from enarf_gan_amd.libraries.NeRF.rendering import render_scene
    m, sc, pose, mi, coord, K_inv = _narf()
    root_x = float(pose[0, 0, 0, 3])
    left, right = _moved(pose, -1.3 - root_x, 3.0), _moved(pose, 1.3 - root_x, 3.0)
    (ca, ma, da), (cb, mb, db) = _single(m, coord, left, K_inv, mi, 6), _single(m, coord, right, K_inv, mi, 6)
    assert int((ma > 0).sum()) > 20 and int((mb > 0).sum()) > 20 and not ((ma > 0) & (mb > 0)).any()
    c, mk, d = render_scene(m, coord, torch.cat([left, right]), K_inv, Nc=NC, Nf=NF, model_input=_pair(mi), seed=6,
                            avatars_per_batch=1)
    for ours, ref, what in ((c, ca + cb, "colour"), (mk, ma + mb, "mask"), (d, da + db, "disparity")):
        print(f"two avatars apart, {what}: worst entry {assert_close(ours.cpu(), ref.cpu(), what, 1e-4):.3e} of the scale")
    side = m.buffers_tensors
    assert_close(side["avatar_masks"][0].cpu(), torch.cat([ma, mb]).cpu(), "the avatars' own masks", 1e-4)
    assert not side["skipped"].any()
    want = torch.where(ma >= 0.5, 0, torch.where(mb >= 0.5, 1, -1)).int()
    sure = ((ma - 0.5).abs() > 1e-3) & ((mb - 0.5).abs() > 1e-3)
    assert int((want == 0).sum()) > 5 and int((want == 1).sum()) > 5 and torch.equal(side["instance"][sure], want[sure])
    both = render_scene(m, coord, torch.cat([left, right]), K_inv, Nc=NC, Nf=NF, model_input=_pair(mi), seed=6)
    # one renderer batch of two draws other samples (16 a ray here): the same silhouettes, not the same values
    assert both[0].shape == c.shape and int(((both[1] > 0.5) & (mk > 0.5)).sum()) > 0.5 * int((mk > 0.5).sum())
    with pytest.raises(ValueError, match="avatars_per_batch"):
        render_scene(m, coord, torch.cat([left, right]), K_inv, Nc=NC, Nf=NF, model_input=_pair(mi), avatars_per_batch=0)


def test_the_nearer_avatar_covers_the_farther():
    """two avatars on the same pixels, one 1.5 m behind the other (their depth ranges are apart), marched one a batch:
    where the nearer one's own mask is above 0.99 at most 0.01 of the light of the farther one gets through, so the
    scene's colour is the nearer one's own within 0.01 of the colour scale plus the parity bound, and the pixel is its"""
    from enarf_gan_amd.libraries.NeRF.rendering import render_scene
    m, sc, pose, mi, coord, K_inv = _narf()
    far = _moved(pose, 0.0, 1.5)
    (cn, mn, _), (cf, mf, _) = _single(m, coord, pose, K_inv, mi, 7), _single(m, coord, far, K_inv, mi, 7)
    solid = mn[0] > 0.99
    assert int(solid.sum()) > 10 and int((solid & (mf[0] > 0.5)).sum()) > 5
    for order, near_index in ((torch.cat([far, pose]), 1), (torch.cat([pose, far]), 0)):
        c, mk, _ = render_scene(m, coord, order, K_inv, Nc=NC, Nf=NF, model_input=_pair(mi), seed=7, avatars_per_batch=1)
        scale = max(float(cn.abs().max()), float(cf.abs().max()))
        gap = float((c[0] - cn[0])[:, solid].abs().max())
        print(f"nearer avatar as avatar {near_index}: worst colour gap on its solid pixels {gap / scale:.3e} of the scale")
        assert gap <= (0.01 + 1e-4) * scale
        assert (m.buffers_tensors["instance"][0][solid] == near_index).all()
        assert float((mk[0] - mn[0])[solid].min()) >= -1e-4                    # the scene is at least as opaque there


# ------------------------------------------------------------------------------------------------- the generator
def test_generator_scene_and_its_animation():
    """TriNARFGenerator.render_scene at size 32 with K = 2: shapes and dtypes, the image is render_scene's colour over the
    background as forward() composes it, and render_scene_animation with frames_per_batch = 1 gives, byte for byte, the
    frames of render_scene (one avatar a batch) on the interpolated poses; the sampler's seeds come from torch's
    generator, reseeded before each route"""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle
    from enarf_gan_amd.libraries.NeRF.rendering import render_scene, semantic_palette
    from test_gpu_anim import _generator
    gen, s, z = _generator(S, 24, 32)
    nerf, psi = gen.nerf, 0.4
    first = s["pose_to_camera"][:1]
    second = first.clone()
    second[:, :, 0, 3] += 0.4
    second[:, :, 2, 3] += 0.3
    pose = torch.cat([first, second]).cuda()
    z2 = torch.cat([z, torch.randn(1, z.shape[1], generator=torch.Generator().manual_seed(3)).cuda()])
    bl = s["bone_length"][:1].cuda().repeat(2, 1, 1)
    K = s["intrinsics"][:1].cuda()
    K_inv = torch.linalg.inv_ex(K.float()).inverse
    image, mask, instance, colours = gen.render_scene(pose, bl, z2, K_inv, truncation_psi=psi, return_instances=True, seed=9)
    assert image.shape == (1, 3, S, S) and image.dtype == torch.float32 and mask.shape == (1, S, S) and mask.dtype == torch.float32
    assert instance.shape == (1, S, S) and instance.dtype == torch.int32 and colours.shape == (1, 3, S, S)
    assert set(instance.unique().tolist()) == {-1, 0, 1} and image.is_cuda and float(mask.max()) > 0.9
    palette = semantic_palette(2, "cuda")
    for k in (0, 1):
        assert torch.equal(colours[0][:, instance[0] == k].t(), palette[k].expand(int((instance[0] == k).sum()), 3))
    assert (colours[0][:, instance[0] < 0] == 1).all()
    two = gen.render_scene(pose, bl, z2, K_inv, truncation_psi=psi, seed=9)
    assert len(two) == 2 and torch.equal(two[0], image) and torch.equal(two[1], mask)
    z_nerf, z_render, _ = gen._latent_parts(z2)
    parts, pack = ops.prepare(pose, bl, nerf.canonical_bone_length, z_render, nerf.mlp.as_dict(), nerf.parent_id,
                              nerf.origin_location, nerf.coordinate_scale)
    _, pixels = gen.ray_sampler(S, S, 1, device="cuda")
    mi = {"z": z_nerf, "z_rend": z_render, "bone_length": bl, "truncation_psi": psi}
    c, mk, _ = render_scene(nerf, pixels, pose.new_empty(2, nerf.num_bone, 4, 4), K_inv, Nc=24, Nf=32, model_input=mi, seed=9,
                            _parts=parts, _pack=pack)
    assert torch.equal(mask, mk.reshape(1, S, S))
    assert torch.equal(image, c.reshape(1, 3, S, S) + (1 - mk.reshape(1, 1, S, S)) * -1)          # a black background: -1
    given = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(1)).cuda()
    over = gen.render_scene(pose, bl, z2, K_inv, truncation_psi=psi, background=given, seed=9)[0]
    assert torch.equal(over, c.reshape(1, 3, S, S) + (1 - mk.reshape(1, 1, S, S)) * given)
    for bad in ("second", given[:, :, :8], None):
        with pytest.raises(ValueError, match="background"):
            gen.render_scene(pose, bl, z2, K_inv, background=bad)
    with pytest.raises(AssertionError):
        gen.render_scene(pose, bl, z, K_inv)

    num = 3
    keys = torch.stack([torch.cat([p[None], rotate_pose_by_angle(p[None], torch.tensor([0.7]))]) for p in pose.cpu()]).double().cuda()
    torch.manual_seed(5)
    frames, masks, instances, poses = gen.render_scene_animation(keys, bl, K, z2, num=num, loop=False, truncation_psi=psi,
                                                                 frames_per_batch=1)
    assert frames.shape == (num, S, S, 3) and frames.dtype == torch.uint8 and masks.shape == (num, S, S) and masks.dtype == torch.uint8
    assert instances.shape == (num, S, S) and instances.dtype == torch.int32 and poses.shape == (2, num, 24, 4, 4)
    assert poses.dtype == torch.float64 and frames.is_cuda and masks.is_cuda and instances.is_cuda and poses.is_cuda
    for k in (0, 1):
        assert torch.equal(poses[k], ops.interpolate_pose(keys[k], s["parents"], num, False))
    torch.manual_seed(5)
    for f in range(num):
        person, alpha, backdrop = gen.render_scene(poses[:, f].float(), bl, z2, K_inv, truncation_psi=psi, avatars_per_batch=1,
                                                   return_bg=True)
        want_frame, want_mask = ops.compose_frames(person, alpha, backdrop)
        assert torch.equal(frames[f], want_frame[0]) and torch.equal(masks[f], want_mask[0]), f"frame {f}"
        assert torch.equal(instances[f], nerf.buffers_tensors["instance"].reshape(S, S)), f"instances of frame {f}"
    assert not torch.equal(frames[0], frames[2])
    torch.manual_seed(5)
    chunked = gen.render_scene_animation(list(keys), bl, K, z2, num=num, loop=False, truncation_psi=psi, frames_per_batch=2)
    assert chunked[0].shape == frames.shape and chunked[2].shape == instances.shape and torch.equal(chunked[3], poses)
    with pytest.raises(AssertionError):
        gen.render_scene_animation(keys, bl, K, z, num=num)
