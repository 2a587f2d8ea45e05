"""GPU tests of the animation path (libenarf_anim.so): the pose kernel against the numpy referee of its contract
(tests/anim_reference.py) and the reference's recorded outputs (tests/golden/pose_interp.npz) under the tolerance rule of
DESIGN.md §3.11, the frame composition byte for byte against its fp32 restatement, and TriNARFGenerator.render_animation
against the generator's own forward().

The rule: for each input, d is the largest absolute difference between the referee's float64 and longdouble runs on that
input; the kernel's fp64 output must lie within 16 d of the float64 run (and so within 32 d of the reference's recording,
which the CPU suite holds within 16 d of it)."""
import numpy as np
import pytest
import torch

import anim_reference as A

pytestmark = pytest.mark.gpu

PARENTS = A.SMPL_PARENTS


def _interp(keys, parents, num, loop, orbit=None, f32=True, bone=True):
    from enarf_gan_amd import _anim_lib
    dev = torch.device("cuda")
    out = _anim_lib.interpolate_pose(torch.from_numpy(np.array(keys)).to(dev), parents, num, loop,
                                     None if orbit is None else torch.from_numpy(np.array(orbit)).to(dev),
                                     want_f32=f32, want_bone_length=bone)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _check(what, got, keys, parents, num, loop, f64, d, orbit=None):
    """the rule, the fp32 copy bit for bit, the bone lengths to one fp32 ulp; returns the ratio |kernel - referee| / d"""
    p64, p32, bone = got
    J = keys.shape[1]
    assert p64.shape == (num, J, 4, 4) and p64.dtype == np.float64 and p32.dtype == np.float32 and bone.shape == (num, J - 1, 1)
    err = float(np.abs(p64 - f64).max())
    print(f"{what}: |kernel - referee| {err:.3e}, d {d:.3e}, ratio {err / d:.2f}")
    assert np.isfinite(p64).all() and err <= A.FACTOR * d, (what, err, d)
    assert np.array_equal(p32.view(np.uint32), p64.astype(np.float32).view(np.uint32)), f"{what}: the fp32 copy is not the fp64 output rounded once"
    want = A.bone_length(f64, parents).astype(np.float32)
    assert (np.abs(bone - want) <= np.spacing(want)).all(), f"{what}: bone_length"
    return err / d


@pytest.mark.parametrize("n", range(7))
def test_pose_kernel_matches_referee_and_golden(n):
    keys, num, loop, recorded, f64, d = A.golden_case(n)
    got = _interp(keys, PARENTS, num, loop)
    _check(f"case {n} (K {keys.shape[0]}, num {num}, loop {loop})", got, keys, PARENTS, num, loop, f64, d)
    assert np.abs(got[0] - recorded).max() <= 2 * A.FACTOR * d
    if not loop:                                   # the last frame of an open sequence is the last key pose
        assert np.abs(got[0][-1] - keys[-1]).max() <= A.FACTOR * d


def test_pose_kernel_with_orbit():
    """angles 0, pi / 2 and arbitrary ones: the referee followed by the float64 rotate_pose"""
    rng = np.random.default_rng(5)
    for n in (0, 1):
        keys, num, loop = A.golden_case(n)[:3]
        orbit = np.r_[0.0, np.pi / 2, 2.2173, rng.uniform(-7, 7, num - 3)]
        f64, d = A.gap(keys, PARENTS, num, loop, orbit)
        plain = A.golden_case(n)[4]
        assert np.abs(f64[1] - plain[1]).max() > 0.1           # the quarter turn moved frame 1
        got = _interp(keys, PARENTS, num, loop, orbit)
        _check(f"orbit, case {n}", got, keys, PARENTS, num, loop, f64, d)
        assert np.abs(got[0][0] - plain[0]).max() <= A.FACTOR * d      # angle 0 leaves frame 0 where it was


def test_pose_kernel_chain_of_64_and_single_joint():
    """a chain-shaped skeleton of 64 joints (a full wavefront, kinematic depth 63) and a skeleton of one joint, d recomputed"""
    rng = np.random.default_rng(11)
    chain = np.arange(-1, 63)
    for J, parents, K, num, loop in ((64, chain, 2, 4, True), (64, chain, 3, 4, False), (1, np.array([-1]), 3, 6, True)):
        keys = A.random_key_poses(rng, K, J=J, parents=parents)
        f64, d = A.gap(keys, parents, num, loop)
        got = _interp(keys, parents, num, loop)
        _check(f"J {J}, K {K}, num {num}, loop {loop}", got, keys, parents, num, loop, f64, d)


def test_pose_kernel_identical_keys_and_a_single_frame():
    """identical key poses (zero relative rotation) reproduce the key pose; num = 1 with loop is the first key pose"""
    keys = np.repeat(A.golden_case(0)[0][1:2], 3, axis=0)
    for num, loop in ((6, True), (4, False)):
        f64, d = A.gap(keys, PARENTS, num, loop)
        got = _interp(keys, PARENTS, num, loop)
        _check(f"identical keys, loop {loop}", got, keys, PARENTS, num, loop, f64, d)
        assert np.abs(got[0] - keys[0]).max() <= A.FACTOR * d
    one = A.golden_case(4)[0]                                      # K = 1
    f64, d = A.gap(one, PARENTS, 1, True)
    got = _interp(one, PARENTS, 1, True)
    _check("num 1", got, one, PARENTS, 1, True, f64, d)
    assert np.abs(got[0][0] - one[0]).max() <= A.FACTOR * d


def test_pose_kernel_null_outputs_are_not_written():
    """null optional outputs are left alone and nothing is written past frame num: buffers one frame longer, full of a
    sentinel, through the C ABI itself"""
    import ctypes as C
    from enarf_gan_amd import _anim_lib
    keys, num, loop, _, f64, d = A.golden_case(0)
    lib = _anim_lib.load()
    dev = torch.device("cuda")
    key = torch.from_numpy(np.array(keys)).to(dev)
    orbit = torch.zeros(num + 1, dtype=torch.float64, device=dev)
    bufs = {"p64": torch.full((num + 1, 24, 4, 4), -7.0, dtype=torch.float64, device=dev),
            "p32": torch.full((num + 1, 24, 4, 4), -7.0, dtype=torch.float32, device=dev),
            "bone": torch.full((num + 1, 23, 1), -7.0, dtype=torch.float32, device=dev)}
    par = (C.c_int32 * 24)(*[int(v) for v in PARENTS])
    stream = torch.cuda.current_stream().cuda_stream

    def call(p32, bone, angles=None):
        _anim_lib.check(lib.enarf_anim_interpolate_pose(key.data_ptr(), par, 3, 24, num, int(loop), angles, bufs["p64"].data_ptr(),
                                                        p32, bone, stream), "enarf_anim_interpolate_pose")
        torch.cuda.synchronize()
    call(None, None)
    assert (bufs["p32"] == -7).all() and (bufs["bone"] == -7).all() and (bufs["p64"][num] == -7).all()
    assert np.abs(bufs["p64"][:num].cpu().numpy() - f64).max() <= A.FACTOR * d
    first = bufs["p64"][:num].clone()
    call(bufs["p32"].data_ptr(), None, orbit.data_ptr())               # an orbit of zeros turns nothing
    assert (bufs["bone"] == -7).all() and (bufs["p32"][num] == -7).all() and (bufs["p64"][num] == -7).all()
    assert torch.equal(bufs["p32"][:num], bufs["p64"][:num].float())
    assert np.abs((bufs["p64"][:num] - first).cpu().numpy()).max() <= A.FACTOR * d
    call(None, bufs["bone"].data_ptr())
    assert (bufs["bone"][num] == -7).all() and (bufs["bone"][:num] > 0).all() and torch.equal(bufs["p64"][:num], first)
    # what the host refuses, it refuses before any launch
    for K_, J_, num_, loop_ in ((3, 24, 10, 1), (3, 24, 9, 0), (1, 24, 4, 0), (3, 65, 12, 1), (0, 24, 12, 1), (3, 24, 0, 1)):
        assert lib.enarf_anim_interpolate_pose(key.data_ptr(), par, K_, J_, num_, loop_, None, bufs["p64"].data_ptr(), None, None,
                                               stream) == -1
    bad = (C.c_int32 * 24)(*([-1] + [5] * 23))
    assert lib.enarf_anim_interpolate_pose(key.data_ptr(), bad, 3, 24, 12, 1, None, bufs["p64"].data_ptr(), None, None, stream) == -1
    torch.cuda.synchronize()
    assert torch.equal(bufs["p64"][:num], first) and (bufs["p64"][num] == -7).all()


def test_two_runs_give_identical_bits():
    keys, num, loop = A.golden_case(6)[:3]
    orbit = np.linspace(0, 2 * np.pi, num, endpoint=False)
    a, b = _interp(keys, PARENTS, num, loop, orbit), _interp(keys, PARENTS, num, loop, orbit)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    rng = np.random.default_rng(2)
    color, mask = rng.uniform(-1.2, 1.2, (3, 3, 49)).astype(np.float32), rng.uniform(0, 1, (3, 49)).astype(np.float32)
    a, b = _compose(color, mask, 0.25), _compose(color, mask, 0.25)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------- frames
def _compose(color, mask, bg, masks=True):
    from enarf_gan_amd import ops
    dev = torch.device("cuda")
    bg = torch.from_numpy(bg).to(dev) if isinstance(bg, np.ndarray) else bg
    out = ops.compose_frames(torch.from_numpy(color).to(dev), torch.from_numpy(mask).to(dev), bg, return_masks=masks)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) if masks else out.cpu().numpy()


@pytest.mark.parametrize("background", ["scalar", "shared", "per_frame"])
@pytest.mark.parametrize("F,S", [(3, 5), (3, 16), (1, 2), (1, 1)])
def test_compose_matches_restatement_byte_for_byte(F, S, background):
    """n = 25 (a tail, and groups of four that straddle two frames), 256, 4 (no tail) and 1 (tail only)"""
    rng = np.random.default_rng(100 * F + S)
    n = S * S
    color = rng.uniform(-1.3, 1.3, (F, 3, n)).astype(np.float32)
    mask = rng.uniform(-0.1, 1.1, (F, n)).astype(np.float32)
    mask[rng.uniform(size=mask.shape) < 0.2] = 0.0
    mask[rng.uniform(size=mask.shape) < 0.2] = 1.0
    bg = {"scalar": -1.0, "shared": rng.uniform(-1.2, 1.2, (1, 3, S, S)).astype(np.float32),
          "per_frame": rng.uniform(-1.2, 1.2, (F, 3, S, S)).astype(np.float32)}[background]
    frames, masks = _compose(color.reshape(F, 3, S, S), mask.reshape(F, S, S), bg)
    want_frames, want_masks = A.compose_frames(color, mask, bg)
    assert frames.shape == (F, S, S, 3) and frames.dtype == np.uint8 and masks.shape == (F, S, S) and masks.dtype == np.uint8
    assert np.array_equal(frames, want_frames) and np.array_equal(masks, want_masks)
    assert np.array_equal(_compose(color, mask, bg, masks=False), want_frames)          # the masks output absent
    if n > 4:
        assert len(np.unique(want_frames)) > 10 and 0 in want_frames and 255 in want_frames


def _around(x, steps=2):
    """x and its fp32 neighbours up to `steps` ulps either side"""
    out = [x]
    lo = hi = x
    for _ in range(steps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.stack(out, axis=-1).reshape(-1)


def test_compose_on_decisions():
    """colours for which v 127.5 + 127.5 lands exactly on an integer and an ulp either side, values outside [-1, 1], masks
    of exactly 0 and 1 and around every k / 255, infinities and NaNs; S = 37 is odd, so four-pixel groups straddle the
    two frames and a tail is left"""
    S = 37
    n = S * S
    k = np.arange(256, dtype=np.float32)
    c = _around(((k - np.float32(127.5)) / np.float32(127.5)).astype(np.float32))          # 1280 colours
    m = _around((k / np.float32(255)).astype(np.float32))                                    # 1280 mask values
    special = np.array([-1.5, 1.5, -1.0, 1.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30, 1e-40], np.float32)
    rng = np.random.default_rng(9)
    color = rng.uniform(-1, 1, (2, 3, n)).astype(np.float32)
    mask = np.ones((2, n), np.float32)
    for ch in range(3):                           # frame 0: mask 1, so v = c; each channel its own order
        color[0, ch, :len(c)] = np.roll(c, 7 * ch)
        color[0, ch, len(c):len(c) + len(special)] = np.roll(special, ch)
    mask[1, :len(m)] = m                          # frame 1: the mask on its decisions, colour and background random
    mask[1, len(m):len(m) + len(special)] = special
    mask[1, len(m) + len(special):] = rng.choice(np.array([0.0, 1.0, 0.5], np.float32), n - len(m) - len(special))
    with np.errstate(invalid="ignore", over="ignore"):
        w = color[0] * np.float32(127.5) + np.float32(127.5)
        on, frac = w == np.round(w), w - np.floor(w)
    assert on.sum() > 300 and ((frac > 0.9999) & (w < 255)).sum() > 100 and ((frac > 0) & (frac < 1e-4)).sum() > 100
    for bg in (-1.0, 0.3, rng.uniform(-1, 1, (1, 3, S, S)).astype(np.float32)):
        if isinstance(bg, np.ndarray):
            bg[0, 0, 0, :3] = [np.nan, np.inf, -np.inf]
        frames, masks = _compose(color, mask, bg)
        want_frames, want_masks = A.compose_frames(color, mask, bg)
        assert np.array_equal(frames, want_frames) and np.array_equal(masks, want_masks)
    nan_at = len(c) + 8                                                                           # special[8]
    assert np.isnan(color[0, 0, nan_at]) and want_frames.reshape(2, n, 3)[0, nan_at, 0] == 0      # a NaN gives 0
    assert want_masks.reshape(2, n)[1, len(m) + 8] == 0 and want_masks.reshape(2, n)[1, len(m) + 6] == 255


# ------------------------------------------------------------------------------------------------- render_animation
def _generator(S, Nc, Nf):
    """the tiny generator of test_gpu_api.test_gan_generator_forward_matches_oracle: a fixed tri-plane stands in for the
    synthesis network, one copy per image of the batch it is asked for"""
    from _helpers import Scene
    from enarf_gan_amd.models.generator import TriNARFGenerator
    from test_host_cpu import Cfg, _nerf_cfg
    sc = Scene(S, 1, "center_fixed", 256)
    s = sc.raw
    gen = TriNARFGenerator(Cfg(z_dim=256, background_ratio=0.7, crop_background=True, pretrained_background=False,
                               nerf_params=_nerf_cfg(Nc=Nc, Nf=Nf, constant_triplane=False)), S, 24, s["parents"], 23,
                           black_background=True)
    gen.register_canonical_pose(s["canonical_pose"])
    gen.nerf.load_state_dict({f"mlp.{k}": v for k, v in s["mlp"].items()}, strict=False)
    gen = gen.cuda().eval()
    tri = s["tri_plane"][:1].cuda()
    gen.nerf.tri_plane_gen = lambda z_, enc, truncation_psi=1: tri.repeat(z_.shape[0], 1, 1, 1)
    z = torch.cat([torch.randn(1, 512, generator=torch.Generator().manual_seed(0)), s["z_rend"][:1]], dim=1).cuda()
    return gen, s, z


def test_render_animation_chunks_match_forward_on_the_same_chunks():
    """K = 2, num = 4, frames_per_batch = 3: one full chunk and one short one. The frames equal, byte for byte,
    compose_frames of what gen(...) returns for the poses render_animation returned, with the same z and truncation_psi,
    every frame having its own copy of the tri-plane there (z repeated per frame): the shared tri-plane route gives the
    bits of the per-frame route. gen(...) is called on the frames of a chunk together, because a renderer batch shares
    its near / far planes (reduced over the batch) and numbers its rays batch-wide for the importance samples; the
    sampler's seeds are drawn from torch's generator, reseeded before each route."""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle
    S, num, per, psi = 32, 4, 3, 0.4
    gen, s, z = _generator(S, 24, 32)
    first = s["pose_to_camera"][:1]
    keys = torch.cat([first, rotate_pose_by_angle(first, torch.tensor([0.7]))]).double().cuda()
    bone_length, K = s["bone_length"][:1].cuda(), s["intrinsics"][:1].cuda()
    orbit = torch.linspace(0, 0.5, num, dtype=torch.float64).cuda()
    torch.manual_seed(11)
    frames, masks, poses = gen.render_animation(keys, bone_length, K, z, num=num, loop=True, orbit=orbit, truncation_psi=psi,
                                                frames_per_batch=per)
    assert frames.shape == (num, S, S, 3) and frames.dtype == torch.uint8 and masks.shape == (num, S, S) and masks.dtype == torch.uint8
    assert poses.shape == (num, 24, 4, 4) and poses.dtype == torch.float64 and frames.is_cuda and masks.is_cuda and poses.is_cuda
    want_poses, want32 = ops.interpolate_pose(keys, s["parents"], num, True, orbit, return_f32=True)
    assert torch.equal(poses, want_poses)
    K_inv = torch.linalg.inv_ex(K.float()).inverse
    torch.manual_seed(11)
    with torch.no_grad():
        for a in range(0, num, per):
            c = min(a + per, num) - a
            person, alpha, bg = gen(want32[a:a + c], None, bone_length.expand(c, -1, -1), z.expand(c, -1), K_inv.expand(c, -1, -1),
                                    truncation_psi=psi, return_bg=True)
            assert bg == -1 and gen.nerf.buffers_tensors["tri_plane_feature"].shape[0] == c
            want_frames, want_masks = ops.compose_frames(person, alpha, bg)
            for f in range(c):
                assert torch.equal(frames[a + f], want_frames[f]), f"frame {a + f}"
                assert torch.equal(masks[a + f], want_masks[f]), f"mask of frame {a + f}"
    assert int(masks.max()) > 50 and len(torch.unique(frames)) > 20
    assert not torch.equal(frames[0], frames[3])
    with pytest.raises(AssertionError):            # one identity at a time
        gen.render_animation(keys, bone_length, K, z.expand(2, -1), num=num)
    with pytest.raises(AssertionError):
        gen.render_animation(keys, bone_length.expand(2, -1, -1), K, z, num=num)


def test_render_animation_one_frame_per_batch_matches_single_frame_calls():
    """frames_per_batch = 1: every frame is a renderer batch of its own, so the frames equal, byte for byte, compose_frames
    of what one gen(...) call per frame returns for the same z, truncation_psi and the poses render_animation returned
    (the sampler's seeds are drawn from torch's generator in frame order, reseeded before each route). With more frames
    a batch the bytes depend on the grouping, as the docstring says: the near / far planes are reduced over the batch."""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle
    S, num, psi = 32, 4, 0.4
    gen, s, z = _generator(S, 24, 32)
    first = s["pose_to_camera"][:1]
    keys = torch.cat([first, rotate_pose_by_angle(first, torch.tensor([0.7]))]).double().cuda()
    bone_length, K = s["bone_length"][:1].cuda(), s["intrinsics"][:1].cuda()
    torch.manual_seed(5)
    frames, masks, poses = gen.render_animation(keys, bone_length, K, z, num=num, loop=False, truncation_psi=psi,
                                                frames_per_batch=1)
    K_inv = torch.linalg.inv_ex(K.float()).inverse
    torch.manual_seed(5)
    with torch.no_grad():
        for f in range(num):
            person, alpha, bg = gen(poses[f:f + 1].float(), None, bone_length, z, K_inv, truncation_psi=psi, return_bg=True)
            want_frames, want_masks = ops.compose_frames(person, alpha, bg)
            assert torch.equal(frames[f], want_frames[0]), f"frame {f}"
            assert torch.equal(masks[f], want_masks[0]), f"mask of frame {f}"
    assert int(masks.max()) > 50 and not torch.equal(frames[0], frames[3])


def test_compose_into_unaligned_slices_and_from_unaligned_inputs():
    """`out` slices that start at a byte address that is no multiple of 4 (S = 5, from frame 1 of a larger buffer) go
    through a copy: the bytes are the restatement's and the frames around the slice keep their sentinel. Inputs that are
    not 16-byte aligned with n % 4 == 0 take the kernel's pixel-by-pixel loads: the same bytes."""
    from enarf_gan_amd import ops
    dev = torch.device("cuda")
    rng = np.random.default_rng(31)
    F, S = 2, 5
    n = S * S
    color, mask = rng.uniform(-1.2, 1.2, (F, 3, n)).astype(np.float32), rng.uniform(0, 1, (F, n)).astype(np.float32)
    bg = rng.uniform(-1, 1, (1, 3, S, S)).astype(np.float32)
    want_frames, want_masks = A.compose_frames(color, mask, bg)
    frames = torch.full((F + 2, S, S, 3), 77, dtype=torch.uint8, device=dev)
    masks = torch.full((F + 2, S, S), 77, dtype=torch.uint8, device=dev)
    assert frames[1:F + 1].data_ptr() % 4 and masks[1:F + 1].data_ptr() % 4
    got = ops.compose_frames(torch.from_numpy(color).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(bg).to(dev),
                             out=(frames[1:F + 1], masks[1:F + 1]))
    torch.cuda.synchronize()
    assert got[0].data_ptr() == frames[1:].data_ptr() and got[1].data_ptr() == masks[1:].data_ptr()
    assert np.array_equal(frames[1:F + 1].cpu().numpy(), want_frames) and np.array_equal(masks[1:F + 1].cpu().numpy(), want_masks)
    for t in (frames, masks):
        assert (t[0] == 77).all() and (t[F + 1] == 77).all()
    only = torch.full((F + 2, S, S, 3), 77, dtype=torch.uint8, device=dev)
    ops.compose_frames(torch.from_numpy(color).to(dev), torch.from_numpy(mask).to(dev), -1.0, return_masks=False, out=(only[1:F + 1], None))
    assert np.array_equal(only[1:F + 1].cpu().numpy(), A.compose_frames(color, mask, -1.0)[0]) and (only[0] == 77).all() and (only[F + 1] == 77).all()
    # n % 4 == 0 with inputs one float off a 16-byte boundary
    F, S = 3, 4
    n = S * S
    color, mask = rng.uniform(-1.2, 1.2, (F, 3, n)).astype(np.float32), rng.uniform(0, 1, (F, n)).astype(np.float32)
    bg = rng.uniform(-1, 1, (F, 3, n)).astype(np.float32)

    def off(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device=dev)
        view = buf[1:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    want_frames, want_masks = A.compose_frames(color, mask, bg)
    for c_, m_, b_ in ((off(color), off(mask), off(bg)), (torch.from_numpy(color).to(dev), off(mask), torch.from_numpy(bg).to(dev))):
        got = ops.compose_frames(c_, m_, b_)
        assert np.array_equal(got[0].cpu().numpy(), want_frames) and np.array_equal(got[1].cpu().numpy(), want_masks)
