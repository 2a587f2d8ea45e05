"""GPU tests of the pose prior's bone masks (libenarf_pose.so): bit-for-bit agreement with the float64 numpy
restatement of the contract (tests/bone_mask_reference.py), the edge cases, the reference's recorded outputs
(tests/golden/bone_mask.npz), determinism, bounds, HumanPoseDataset against the reference's items, and the bone-guided
loss on drawn masks."""
import ctypes as C

import numpy as np
import pytest
import torch

import bone_mask_reference as R
import pose_golden as PG
from enarf_gan_amd import synth

pytestmark = pytest.mark.gpu

ALL = ("mask", "disparity", "part_disparity", "keypoint_mask", "pose_2d")


def _poses(B, S, seed):
    poses = synth.random_pose(B, seed=seed)[0].numpy().astype(np.float64)
    poses[:, :, :3, 3] += np.random.RandomState(seed).normal(0, 1e-3, poses[:, :, :3, 3].shape)
    K = np.broadcast_to(synth.intrinsics(S)[0][0].numpy().astype(np.float64), (B, 3, 3)).copy()
    K[:, 0, 2] += 0.37                               # a principal point off the pixel grid
    return poses, K


def _draw(poses, K, S, t, outputs=ALL):
    from enarf_gan_amd.dataset.utils_3d import bone_masks
    out = bone_masks(torch.from_numpy(np.ascontiguousarray(poses)).cuda(), torch.from_numpy(np.ascontiguousarray(K)).cuda(),
                     S, t, outputs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    """identical bits, NaN payloads aside (numpy's 0/0 on the host and the device's differ in sign)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return ((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all()


def _check_bits(got, ref, frames, what):
    for name in got:
        assert _same_bits(got[name][frames], ref[name]), f"{what}: {name} differs from the restatement"


@pytest.mark.parametrize("t", [0.5, 1.5])
@pytest.mark.parametrize("B,S", [(1, 64), (12, 64), (32, 64), (1, 128), (12, 128), (32, 128), (1, 512), (12, 512),
                                 (32, 512)])
def test_kernel_matches_restatement_bit_for_bit(B, S, t):
    poses, K = _poses(B, S, seed=100 + B)
    got = _draw(poses, K, S, t)
    # the restatement costs ~1 s a frame at 512: check the first and last frames there, every frame below
    frames = [0, B - 1] if S == 512 else list(range(B))
    ref = R.batch(poses[frames], K[frames], S, t)
    _check_bits(got, ref, frames, f"B={B} S={S} t={t}")
    assert got["mask"].mean() > 0.002
    mask_only = _draw(poses, K, S, t, ("mask",))
    assert np.array_equal(mask_only["mask"], got["mask"])


def _edge_poses(S):
    """off-screen and behind-camera joints, a joint at z = 0, every keypoint box across each border, all bones of zero
    length, a size of 1"""
    g = PG.load()
    out = []
    base, K = _poses(1, S, seed=7)
    f, c = K[0, 0, 0], K[0, 0, 2]
    for offset in (-1.5, -0.5, -0.2, 0.0, 0.3):         # keypoints across the top / left border, on it, inside it
        p = base[0].copy()
        for j in range(24):
            z = p[j, 2, 3]
            px = [offset, S - 1 - offset, 0.4 * S, 0.6 * S][j % 4]
            py = [0.3 * S, 0.7 * S, offset, S - 1 - offset][j % 4]
            p[j, 0, 3], p[j, 1, 3] = (px - c) * z / f, (py - c) * z / f
        out.append(p)
    p = base[0].copy()
    p[10, 2, 3], p[11, 2, 3], p[4, 2, 3] = -0.5, -2.0, 0.0            # behind the camera, and on its plane
    p[15, :3, 3] = (50.0, -40.0, 1.0)                                 # far off screen
    out.append(p)
    p = base[0].copy()
    p[:, :3, 3] = p[0, :3, 3]                                         # every bone of zero length
    out.append(p)
    if S == 64:
        out.append(g["float64_64_t0.5_poses"][PG.EDGE_FRAME])
    return np.stack(out), np.broadcast_to(K[0], (len(out), 3, 3)).copy()


@pytest.mark.parametrize("t", [0.5, 1.5])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_edge_cases_match_restatement(S, t):
    poses, K = _edge_poses(S)
    got = _draw(poses, K, S, t)
    ref = R.batch(poses, K, S, t)
    _check_bits(got, ref, slice(None), f"edge S={S} t={t}")
    if S == 64:
        km = got["keypoint_mask"]
        assert km[1].sum() > 0 and km[6].sum() > 0 and got["mask"][6].sum() == 0   # zero-length bones draw no mask
        assert np.isnan(got["pose_2d"][5, 4]).all() and np.isnan(got["disparity"][5]).all()   # a joint at z = 0


def test_kernel_matches_reference_goldens():
    from enarf_gan_amd.dataset.dataset import HumanPoseDataset, SMPLProperty
    from enarf_gan_amd.dataset.utils_3d import create_mask
    g = PG.load()
    hpp = SMPLProperty()
    for name, poses, Ks, S, t, gold in PG.cases(g):
        fp64 = name.startswith("float64")
        got = _draw(poses.astype(np.float64), Ks.astype(np.float64), S, t)
        assert np.array_equal(got["keypoint_mask"], gold["keypoint_mask"]), name
        for b in range(len(poses)):
            diff = got["mask"][b] != gold["mask"][b]
            if fp64:
                assert not diff.any(), (name, b)
                assert np.array_equal(got["disparity"][b], gold["disparity"][b]), (name, b)
            else:
                assert diff.sum() <= 2 and (R.margin(poses[b], Ks[b], S, t)[diff] < 1e-6).all(), (name, b)
                gd = gold["disparity"][b].astype(np.float64)
                rel = np.abs(got["disparity"][b] - gd) / np.maximum(np.abs(gd), 1e-30)
                assert rel.max() <= (1e-4 if (S == 64 and b == PG.EDGE_FRAME) else 1e-6), (name, b, rel.max())
        # the reference's own entry point, fed the reference's (possibly fp32) image coordinates
        jpi = np.concatenate([gold["joint_pos"][0].T, np.ones((1, 24))])[None].astype(poses.dtype)
        jmc_, jpi_ = HumanPoseDataset.add_blank_part(None, poses[:1], jpi)
        disp, mask, part, key = create_mask(hpp, jmc_, jpi_, S, thickness=t)
        assert disp.dtype == np.float32 and part.shape == (19, S, S) and key.shape == (24, S, S)
        assert np.array_equal(mask, gold["mask"][0]) and np.array_equal(key, gold["keypoint_mask"][0]), name
        gd = gold["disparity"][0].astype(np.float64)
        assert (np.abs(disp - gd) <= (0 if fp64 else 1e-6) * np.abs(gd)).all(), name
        if S == 64 and t == 0.5:
            gp = g[f"{name}_part_disparity"].astype(np.float64)
            assert (np.abs(part - gp) <= (0 if fp64 else 1e-6) * np.abs(gp)).all(), name


def test_two_runs_give_identical_bits():
    poses, K = _poses(12, 128, seed=3)
    a, b = _draw(poses, K, 128, 0.5), _draw(poses, K, 128, 0.5)
    for k in ALL:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_null_outputs_are_not_written():
    """each subset of the optional outputs matches the restatement; buffers one frame longer than B keep the sentinel
    in that frame, and B = 0 writes nothing"""
    from enarf_gan_amd import _pose_lib
    B, S, t = 3, 64, 1.5
    poses, K = _poses(B, S, seed=21)
    ref = R.batch(poses, K, S, t)
    for subset in (("mask", "disparity"), ("mask", "part_disparity"), ("mask", "keypoint_mask"), ("mask", "pose_2d")):
        got = _draw(poses, K, S, t, subset)
        assert set(got) == set(subset)
        for k in subset:
            assert _same_bits(got[k], ref[k]), (subset, k)
    lib = _pose_lib.load()
    dev = torch.device("cuda")
    shapes = {"mask": (S, S), "disparity": (S, S), "part_disparity": (19, S, S), "keypoint_mask": (24, S, S),
              "pose_2d": (24, 2)}
    bufs = {k: torch.full((B + 1, *s), -7.0, dtype=torch.float64 if k == "pose_2d" else torch.float32, device=dev)
            for k, s in shapes.items()}
    P, KK = torch.from_numpy(poses).to(dev), torch.from_numpy(K).to(dev)
    for n in (B, 0):
        passed = ("mask", "keypoint_mask") if n else ALL
        ptrs = [bufs[k].data_ptr() if k in passed else None for k in ALL]
        _pose_lib.check(lib.enarf_pose_bone_masks(P.data_ptr(), KK.data_ptr(), None, n, S, t, *ptrs,
                                                  torch.cuda.current_stream().cuda_stream), "enarf_pose_bone_masks")
        torch.cuda.synchronize()
    for k in ALL:
        assert (bufs[k][B] == -7).all(), f"{k}: written past frame B"
        if k in ("mask", "keypoint_mask"):
            assert _same_bits(bufs[k][:B].cpu().numpy(), ref[k]), k
        else:
            assert (bufs[k][:B] == -7).all(), f"{k}: written although it was not passed"


@pytest.mark.parametrize("cache", ["cache32", "cache64"])
def test_dataset_batches_reproduce_reference_items(tmp_path, cache):
    from enarf_gan_amd.dataset.dataset import HumanPoseDataset
    g = PG.load()
    PG.write_cache(g, cache, str(tmp_path))
    ds = HumanPoseDataset(size=64, data_root=str(tmp_path), num_repeat_in_epoch=3)
    items = PG.items(g, cache)
    if cache == "cache64":
        assert np.array_equal(ds.canonical_pose, g["cache64_canonical"])
    whole = next(ds.batches(len(ds), shuffle=False, drop_last=False))
    torch.cuda.synchronize()
    for i, want in items.items():
        for src, got in (("batch", {k: v[i] for k, v in whole.items()}), ("item", ds[i])):
            got = {k: v.cpu().numpy() for k, v in got.items()}
            assert set(got) == set(want), (src, sorted(got), sorted(want))
            for k in want:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (cache, src, k)
            assert np.array_equal(got["intrinsics"], want["intrinsics"]) and np.array_equal(got["pose_to_world"],
                                                                                            want["pose_to_world"])
            if cache == "cache32":
                assert np.array_equal(got["pose_to_camera"], want["pose_to_camera"])
            else:             # extrinsic @ pose: the host's matmul, rounded to fp32
                assert (np.abs(got["pose_to_camera"] - want["pose_to_camera"])
                        <= np.spacing(np.abs(want["pose_to_camera"]))).all()
            assert (np.abs(got["bone_length"] - want["bone_length"]) <= np.spacing(want["bone_length"])).all()
            tol = 1e-6 if cache == "cache32" else 1e-12
            assert np.allclose(got["pose_2d"], want["pose_2d"], rtol=tol, atol=0), (cache, src)
            diff = got["bone_mask"] != want["bone_mask"]
            f = i % 5
            margin = R.margin(ds.pose_to_camera[f], ds.intrinsics[f], 64, 0.5)
            assert diff.sum() <= 2 and (margin[diff] < 1e-6).all(), (cache, src, i)
            assert want["bone_mask"].sum() > 20
    # shuffled batches: each row is the frame its index names
    order = ds.batch_order(4, generator=torch.Generator().manual_seed(3))
    for idx, batch in zip(order, ds.batches(4, generator=torch.Generator().manual_seed(3))):
        assert batch["bone_mask"].shape == (4, 64, 64)
        for r, i in enumerate(idx):
            assert torch.equal(batch["bone_mask"][r], whole["bone_mask"][i % 5])
            assert torch.equal(batch["pose_to_camera"][r], whole["pose_to_camera"][i % 5])


def test_nerf_patch_loss_on_drawn_masks(tmp_path):
    from enarf_gan_amd.dataset.dataset import HumanPoseDataset
    from enarf_gan_amd.models.loss import nerf_patch_loss
    g = PG.load()
    PG.write_cache(g, "cache64", str(tmp_path))
    ds = HumanPoseDataset(size=64, data_root=str(tmp_path), num_repeat_in_epoch=1)
    batch = next(ds.batches(5, shuffle=False))
    items = PG.items(g, "cache64")
    idx = sorted(i for i in items if i < 5)
    drawn = batch["bone_mask"][idx].unsqueeze(1)
    golden = torch.from_numpy(np.stack([items[i]["bone_mask"] for i in idx])).unsqueeze(1).cuda()
    fake = torch.rand(len(idx), 1, 64, 64, generator=torch.Generator().manual_seed(0)).cuda()
    assert torch.equal(drawn, golden)
    assert torch.equal(nerf_patch_loss(fake, drawn), nerf_patch_loss(fake, golden))
