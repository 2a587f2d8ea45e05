"""CPU checks of the animation path (libenarf_anim.so's host side): the numpy referee (tests/anim_reference.py) against the
reference's recorded interpolate_pose outputs under the tolerance rule of DESIGN.md §3.11, every argument error of
interpolate_pose / compose_frames before any device call, and the plain-torch turntable helpers of
libraries/NARF/pose_utils.py against the reference's recorded values."""
import numpy as np
import pytest
import torch

import anim_reference as A

PARENTS = A.SMPL_PARENTS


@pytest.mark.parametrize("n", range(7))
def test_referee_matches_the_reference_recording(n):
    """|referee - recording| <= 16 d, d the referee's own float64-against-longdouble difference on the same input"""
    assert A.num_golden_cases() == 7
    keys, num, loop, recorded, f64, d = A.golden_case(n)
    err = float(np.abs(f64 - recorded).max())
    print(f"case {n}: K {keys.shape[0]} num {num} loop {loop}: |referee - reference| {err:.3e}, d {d:.3e}, ratio {err / d:.2f}")
    assert recorded.shape == (num, 24, 4, 4) and 0 < d < 1e-13
    assert err <= A.FACTOR * d
    bottom = np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (num, 24, 4))
    assert np.array_equal(f64[:, :, 3], bottom)


def test_recorded_cases_are_the_listed_ones_and_stay_off_the_half_turn():
    g = A.load_golden()
    assert [tuple(int(v) for v in c) for c in g["cases"]] == [(3, 12, 1), (3, 12, 0), (2, 7, 0), (5, 8, 0), (1, 5, 1),
                                                               (2, 2, 0), (4, 100, 1)]
    assert np.array_equal(g["parents"], PARENTS)
    largest = 0.0
    for n in range(7):
        keys, num, loop = A.golden_case(n)[:3]
        K = keys.shape[0]
        for k in range(K if loop else K - 1):
            for j in range(24):
                loc = [keys[m, j] if j == 0 else A.inv_rigid(keys[m, PARENTS[j]]) @ keys[m, j] for m in (k, (k + 1) % K)]
                cos = (np.trace(loc[0][:3, :3].T @ loc[1][:3, :3]) - 1) / 2
                largest = max(largest, float(np.arccos(np.clip(cos, -1, 1))))
    assert 2.5 < largest < np.pi - 0.05           # large rotations are in, the half turn (no unique short arc) is not


def test_referee_and_binding_raise_where_the_reference_raised():
    from enarf_gan_amd.libraries.NARF.pose_utils import interpolate_pose
    g = A.load_golden()
    assert [tuple(int(v) for v in c) for c in g["raises"]] == [(3, 10, 1), (3, 9, 0)] and list(g["raised"]) == ["ValueError"] * 2
    keys = np.repeat(A.golden_case(0)[0][:1], 3, axis=0)
    for K, num, loop in g["raises"]:
        with pytest.raises(ValueError):
            A.interpolate_pose(keys, PARENTS, int(num), bool(loop))
        with pytest.raises(ValueError):
            interpolate_pose(keys, PARENTS, int(num), bool(loop))


@pytest.fixture
def no_device(monkeypatch):
    """fails the test if the library is loaded or a device call is made"""
    from enarf_gan_amd import _anim_lib

    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_anim_lib, "load", refuse)
    monkeypatch.setattr(torch.cuda, "current_device", refuse)
    monkeypatch.setattr(torch.cuda, "current_stream", refuse)


def test_interpolate_pose_checks_its_arguments_before_any_device_call(no_device):
    from enarf_gan_amd import ops
    from enarf_gan_amd._loader import EnarfHipError
    from enarf_gan_amd.libraries.NARF.pose_utils import interpolate_pose
    keys = A.golden_case(0)[0]                                   # (3, 24, 4, 4)
    chain = list(range(-1, 64))                                  # 65 joints
    bad = [
        (keys, PARENTS, 10, True, None),                         # num not a multiple of K
        (keys, PARENTS, 9, False, None),                         # num not a multiple of K - 1
        (keys[:1], PARENTS, 4, False, None),                     # K < 2 without loop
        (keys[:2], PARENTS, 1, False, None),                     # num < 2 without loop
        (keys, PARENTS, 0, True, None),
        (np.zeros((2, 65, 4, 4)), chain, 4, True, None),         # J > 64
        (keys, PARENTS[:23], 12, True, None),                    # one parent short
        (keys, np.r_[0, PARENTS[1:]], 12, True, None),           # no root in front
        (keys, np.r_[PARENTS[:5], 7, PARENTS[6:]], 12, True, None),   # a parent after its joint
        (keys[:, :, :3], PARENTS, 12, True, None),               # not 4 x 4
        (keys, PARENTS, 12, True, np.zeros(11)),                 # orbit of the wrong length
    ]
    for pose, parents, num, loop, orbit in bad:
        for form in (pose, torch.from_numpy(np.array(pose))):
            with pytest.raises(ValueError):
                interpolate_pose(form, parents, num, loop, orbit)
        with pytest.raises(ValueError):
            ops.interpolate_pose(torch.from_numpy(np.array(pose)), parents, num, loop,
                                 None if orbit is None else torch.from_numpy(orbit))
    with pytest.raises(ValueError):
        interpolate_pose(keys.astype(np.int64), PARENTS, 12, True)
    cpu = torch.from_numpy(np.array(keys))
    for call in (lambda: interpolate_pose(cpu, PARENTS, 12, True), lambda: ops.interpolate_pose(cpu, PARENTS, 12, True),
                 lambda: interpolate_pose(cpu.float(), PARENTS, 12, False, orbit=[0.0] * 12),
                 lambda: ops.interpolate_pose(cpu, PARENTS, 12, True, return_bone_length=True)):
        with pytest.raises(EnarfHipError, match="no CPU fallback"):
            call()


def test_compose_frames_checks_its_arguments_before_any_device_call(no_device):
    from enarf_gan_amd import ops
    from enarf_gan_amd._loader import EnarfHipError
    color, mask = torch.zeros(2, 3, 16), torch.zeros(2, 16)
    bad = [
        (torch.zeros(2, 4, 16), mask, -1.0),                     # not three channels
        (torch.zeros(2, 3, 15), torch.zeros(2, 15), -1.0),       # 15 pixels are no square
        (color, torch.zeros(2, 9), -1.0),                        # mask of another size
        (color, torch.zeros(3, 16), -1.0),                       # mask of another batch
        (color, mask, torch.zeros(3, 3, 4, 4)),                  # background of another batch
        (color, mask, torch.zeros(1, 3, 5, 5)),                  # background of another size
        (torch.zeros(2, 16), mask, -1.0),
    ]
    for c, m, bg in bad:
        with pytest.raises(ValueError):
            ops.compose_frames(c, m, bg)
    with pytest.raises((TypeError, ValueError)):
        ops.compose_frames(color, mask, "black")
    for c, m, bg in ((color, mask, -1.0), (color.reshape(2, 3, 4, 4), mask.reshape(2, 4, 4), torch.zeros(1, 3, 4, 4)),
                     (color, mask, torch.zeros(2, 3, 16))):
        with pytest.raises(EnarfHipError, match="no CPU fallback"):
            ops.compose_frames(c, m, bg)


# ------------------------------------------------------------------------------------------------- the torch helpers
# Every entry of a helper's result is two products and up to three sums of values of magnitude <= `scale` (the largest
# joint translation plus the largest vertex coordinate), behind an fp32 cos / sin, a 24-term mean and a subtraction: fewer
# than 32 roundings of half an fp32 ulp of a value <= scale each. The same bound holds for the reference's own fp32 run.
def _bound(scale):
    return 16 * np.finfo(np.float32).eps * scale


def test_rotation_matrix_and_rotate_pose_match_the_reference_recording():
    from enarf_gan_amd.libraries.NARF import pose_utils as U
    g = A.load_golden()
    pose, angle = torch.from_numpy(g["helper_pose"]), torch.from_numpy(g["helper_angle"])
    assert pose.dtype == torch.float32 and pose.shape == (3, 24, 4, 4) and list(angle[:2]) == [0.0, np.float32(np.pi / 2)]
    R = U.rotation_matrix(angle)
    want = A.rotation_matrix(g["helper_angle"].astype(np.float64))
    assert R.shape == (3, 4, 4) and R.dtype == torch.float32
    assert np.abs(R.numpy() - want).max() <= np.finfo(np.float32).eps          # cos / sin of an fp32 angle: within an ulp of 1
    assert np.abs(g["helper_rotation_matrix"] - want).max() <= np.finfo(np.float32).eps
    assert np.array_equal(R.numpy() == 0, want == 0) and np.array_equal(R.numpy()[:, 1, 1], np.ones(3, np.float32))
    scale = float(np.abs(g["helper_pose"][:, :, :3, 3]).max()) + 1
    want = A.rotate_pose(g["helper_pose"].astype(np.float64), A.rotation_matrix(g["helper_angle"].astype(np.float64)))
    eps = np.finfo(np.float32).eps
    for got in (U.rotate_pose_by_angle(pose, angle), U.rotate_pose(pose, U.rotation_matrix(angle))):
        assert got.dtype == torch.float32 and got.shape == pose.shape
        assert np.abs(got.numpy() - want).max() <= _bound(scale)
        # the rotation block has no mean in it: rows 0 and 2 are c a -+ s b of entries |a|, |b| <= 1 (cos and sin within
        # half an ulp of 1 each, two products, one sum: under 3 eps); row 1 and the bottom row come through exactly
        assert np.abs(got.numpy()[:, :, :3, :3] - want[:, :, :3, :3]).max() <= 3 * eps
        assert torch.equal(got[:, :, 1, :3], pose[:, :, 1, :3]) and torch.equal(got[:, :, 3], pose[:, :, 3])
        assert torch.equal(got[0, :, :3, :3], pose[0, :, :3, :3])                # angle 0 turns nothing
    assert np.abs(g["helper_rotate_pose_by_angle"] - want).max() <= _bound(scale)
    assert np.abs(U.rotate_pose_by_angle(pose, angle).numpy() - g["helper_rotate_pose_by_angle"]).max() <= 2 * _bound(scale)
    # a float64 pose stays float64 (the reference's zeros are hard-coded to fp32 and promote; the values agree)
    got64 = U.rotate_pose_by_angle(pose.double(), angle.double())
    assert got64.dtype == torch.float64 and np.abs(got64.numpy() - want).max() <= 1e-12


def test_rotate_pose_randomly_draws_one_angle_per_pose():
    from enarf_gan_amd.libraries.NARF import pose_utils as U
    pose = torch.from_numpy(A.load_golden()["helper_pose"])
    torch.manual_seed(3)
    got = U.rotate_pose_randomly(pose)
    torch.manual_seed(3)
    angle = pose.new_empty((3,)).uniform_(0, 2 * np.pi)
    assert torch.equal(got, U.rotate_pose_by_angle(pose, angle)) and len(set(angle.tolist())) == 3
    assert float(angle.min()) >= 0 and float(angle.max()) < 2 * np.pi + 1e-6


def test_rotate_mesh_by_angle_matches_the_reference_recording():
    from enarf_gan_amd.libraries.NARF import pose_utils as U
    g = A.load_golden()
    pose, angle = torch.from_numpy(g["helper_pose"][:1]), torch.from_numpy(g["helper_angle"][2:])
    verts, faces = torch.from_numpy(g["helper_vertices"]), torch.from_numpy(g["helper_faces"])
    colours = torch.zeros(37, 3)
    out = U.rotate_mesh_by_angle(pose, (verts, faces, colours), angle)
    assert len(out) == 3 and out[0].shape == (37, 3)
    for copy, given in ((out[1], faces), (out[2], colours)):                     # deep copies, as in the reference
        assert torch.equal(copy, given) and copy.data_ptr() != given.data_ptr()
    assert torch.equal(verts, torch.from_numpy(g["helper_vertices"]))          # the input mesh is left as it was
    want = A.rotate_mesh(g["helper_pose"][:1].astype(np.float64), g["helper_vertices"], g["helper_angle"][2:])
    scale = float(np.abs(g["helper_pose"][0, :, :3, 3]).max() + np.abs(g["helper_vertices"]).max())
    assert np.abs(out[0].numpy() - want).max() <= _bound(scale)
    assert np.abs(g["helper_rotate_mesh_by_angle"] - want).max() <= _bound(scale)
