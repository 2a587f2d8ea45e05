"""CPU checks of the pose prior's bone masks (libenarf_pose.so, include/enarf_pose.h): the numpy restatement of the
contract (tests/bone_mask_reference.py) against the reference's recorded outputs, the hard-coded SMPL tables, the
library's ABI and kernel inventory, the argument checks, the pose-only cache reader and the batch order."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import bone_mask_reference as R
import libraries as L
import pose_golden as PG

ROOT = L.ROOT
SRC = os.path.join(ROOT, "enarf-gan_amd", "csrc", "enarf_pose.hip")

# ------------------------------------------------------------------------------------------------- the restatement
def test_restatement_reproduces_reference_goldens():
    g = PG.load()
    n = 0
    for name, poses, Ks, S, t, gold in PG.cases(g):
        out = R.batch(poses, Ks, S, t)
        fp64 = name.startswith("float64")
        assert np.array_equal(out["keypoint_mask"], gold["keypoint_mask"]), name
        for b in range(len(poses)):
            diff = out["mask"][b] != gold["mask"][b]
            if fp64:
                assert not diff.any(), (name, b)
            else:                 # the reference rounds ab and |ab|^2 to fp32: a differing pixel lies on a boundary
                assert diff.sum() <= 2 and (R.margin(poses[b], Ks[b], S, t)[diff] < 1e-6).all(), (name, b)
            d, gd = out["disparity"][b].astype(np.float64), gold["disparity"][b].astype(np.float64)
            if fp64:
                assert np.array_equal(d, gd), (name, b)
                assert np.array_equal(out["pose_2d"][b], gold["joint_pos"][b]), (name, b)
            else:
                rel = np.abs(d - gd) / np.maximum(np.abs(gd), 1e-30)
                # the edge frame's behind-camera bone cancels in s z_a + (1 - s) z_b, which the reference forms from
                # fp32 projections: its relative error grows there, elsewhere it stays at fp32 rounding
                bound = 1e-4 if (S == 64 and b == PG.EDGE_FRAME) else 1e-6
                assert rel.max() <= bound, (name, b, rel.max())
            n += 1
    assert n == 2 * (4 + 3) * 2
    part = R.masks(g["float64_64_t0.5_poses"][0], g["float64_64_t0.5_K"][0], 64, 0.5)["part_disparity"]
    assert np.array_equal(part, g["float64_64_t0.5_part_disparity"])
    part32 = R.masks(g["float32_64_t0.5_poses"][0], g["float32_64_t0.5_K"][0], 64, 0.5)["part_disparity"]
    gp = g["float32_64_t0.5_part_disparity"].astype(np.float64)
    assert (np.abs(part32 - gp) <= 1e-6 * np.abs(gp)).all()


def test_edge_frame_hits_every_border_and_the_wrap():
    g = PG.load()
    name, poses, Ks, S, t, gold = next(c for c in PG.cases(g) if c[0] == "float64_64_t1.5")
    km = gold["keypoint_mask"][PG.EDGE_FRAME]
    # joints 20 (left) and 22 (top) cross the top / left borders: their boxes wrap away; 21 (right) and 23 (bottom) clip
    assert km[20].sum() == 0 and km[22].sum() == 0
    assert km[21].sum() > 0 and km[21][:, -1].any() and km[23].sum() > 0 and km[23][-1].any()
    assert km[15].sum() == 0                                  # far off screen
    assert poses[PG.EDGE_FRAME, 10, 2, 3] < 0                 # behind the camera


def test_smpl_tables_equal_recorded_ones():
    from enarf_gan_amd.dataset.dataset import SMPLProperty
    from enarf_gan_amd.dataset.utils_3d import BLANK_IDX
    g = PG.load()
    hpp = SMPLProperty()
    assert hpp.prev_seq == g["prev_seq"].tolist() == R.PREV_SEQ
    assert hpp.is_blank.tolist() == g["is_blank"].tolist() == R.IS_BLANK
    assert hpp.valid_keypoints == g["valid_keypoints"].tolist() == R.VALID_KEYPOINTS
    assert BLANK_IDX == g["blank_idx"].tolist() == R.BLANK_IDX
    assert R.PART_IDS == g["part_ids"].tolist() and len(R.PART_IDS) == 19
    assert [R.PART_IDS[k] for k in R.BONE_GROUP] == g["bone_group_ids"].tolist()
    # the kernel's hard-coded tables
    src = open(SRC).read()

    def table(name):
        m = re.search(name + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", src)
        return [int(v) for v in m.group(1).split(",")]
    assert table("kBoneA") == R.BONE_A and table("kBoneB") == R.BONE_B
    assert table("kBoneGroup") == R.BONE_GROUP and table("kKeyJoint") == R.KEY_JOINT


# ------------------------------------------------------------------------------------------------- the library
def test_header_symbols_exported_and_bound():
    """what is specific to this library; tests/test_libraries_cpu.py holds the checks every library gets"""
    from enarf_gan_amd import _pose_lib
    assert L.declared("pose") == ["enarf_pose_abi_version", "enarf_pose_bone_masks", "enarf_pose_last_error"]
    assert _pose_lib.ABI_VERSION == 1


def test_sources_read_no_environment_and_hold_no_assembly():
    for path in (SRC, os.path.join(ROOT, "include", "enarf_pose.h")):
        src = open(path).read()
        assert "getenv" not in src and "asm" not in src, path
    for path in ("_pose_lib.py", os.path.join("dataset", "dataset.py"), os.path.join("dataset", "utils_3d.py")):
        src = open(os.path.join(ROOT, "enarf-gan_amd", path)).read()
        assert "os.environ" not in src and "getenv" not in src, path


def test_argument_checks_need_no_device():
    from enarf_gan_amd import _pose_lib
    L.library("pose")
    lib = _pose_lib.load()
    f = lib.enarf_pose_bone_masks

    def call(pose=1, K=1, jpos=None, B=2, S=64, t=0.5, mask=1):
        return f(pose, K, jpos, B, S, t, mask, None, None, None, None, None)
    assert call(B=-1) == -1 and b"batch -1" in lib.enarf_pose_last_error()
    assert call(B=1 << 31) == -1
    assert call(S=0) == -1 and b"size 0" in lib.enarf_pose_last_error()
    assert call(S=4097) == -1
    assert call(t=float("nan")) == -1 and b"thickness" in lib.enarf_pose_last_error()
    assert call(t=float("inf")) == -1
    assert call(pose=None) == -1 and b"null" in lib.enarf_pose_last_error()
    assert call(mask=None) == -1
    assert call(K=None) == -1
    assert call(B=0) == 0                                     # nothing to draw: no launch
    assert call(B=0, pose=None, K=None, mask=None) == 0


def test_host_layer_has_no_cpu_fallback():
    from enarf_gan_amd._lib import EnarfHipError
    from enarf_gan_amd.dataset.dataset import SMPLProperty
    from enarf_gan_amd.dataset.utils_3d import bone_masks, create_mask
    pose = torch.zeros(1, 24, 4, 4)
    with pytest.raises(EnarfHipError):
        bone_masks(pose, torch.eye(3)[None], 64)
    with pytest.raises(EnarfHipError):
        bone_masks(pose.numpy(), torch.eye(3)[None], 64)

    class Other:
        prev_seq, is_blank, valid_keypoints = [-1, 0], np.array([0, 0]), [0, 1]
    with pytest.raises(NotImplementedError):
        create_mask(Other(), np.zeros((1, 28, 4, 4)), np.zeros((1, 3, 28)), 64)
    if not torch.cuda.is_available():
        with pytest.raises(EnarfHipError):
            create_mask(SMPLProperty(), np.zeros((1, 28, 4, 4)), np.zeros((1, 3, 28)), 64)


# ------------------------------------------------------------------------------------------------- host layer
def test_read_pose_cache_without_images(tmp_path):
    from enarf_gan_amd import formats
    g = PG.load()
    d = PG.write_cache(g, "cache64", str(tmp_path))
    c = formats.read_pose_cache(str(tmp_path / "cache.pickle"))
    assert np.array_equal(c.pose_to_world, d["smpl_pose"]) and np.array_equal(c.intrinsics, d["camera_intrinsic"])
    assert np.array_equal(c.camera_rotation, d["camera_rotation"])
    assert np.array_equal(c.canonical_pose, g["cache64_canonical"])
    items = PG.items(g, "cache64")
    for i, it in items.items():
        assert np.array_equal(c.pose_to_camera[i % 5].astype(np.float32), it["pose_to_camera"])
    d32 = PG.write_cache(g, "cache32", str(tmp_path))
    os.remove(tmp_path / "canonical.npy")
    c32 = formats.read_pose_cache(str(tmp_path / "cache.pickle"))
    assert c32.camera_rotation is None and c32.canonical_pose is None
    assert np.array_equal(c32.pose_to_camera, d32["smpl_pose"])
    with pytest.raises(ValueError):
        formats.read_cache(str(tmp_path / "cache.pickle"))          # the image cache reader still wants 'img'


def test_read_pose_cache_refuses_other_globals(tmp_path):
    from enarf_gan_amd import formats

    class Evil:
        def __reduce__(self):
            return (print, ("this must not run",))
    with open(tmp_path / "cache.pickle", "wb") as f:
        pickle.dump({"camera_intrinsic": np.eye(3)[None], "smpl_pose": np.zeros((1, 24, 4, 4)), "x": Evil()}, f)
    with pytest.raises(formats.UnsafePickleError):
        formats.read_pose_cache(str(tmp_path / "cache.pickle"))


class _Index(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


@pytest.mark.parametrize("batch_size,shuffle,drop_last", [(4, True, True), (3, True, False), (4, False, True)])
def test_batch_order_equals_dataloader(tmp_path, batch_size, shuffle, drop_last):
    from enarf_gan_amd.dataset.dataset import HumanPoseDataset
    PG.write_cache(PG.load(), "cache32", str(tmp_path))
    ds = HumanPoseDataset(size=64, data_root=str(tmp_path), num_repeat_in_epoch=3)
    assert len(ds) == 15 and ds.num_bone == 24 and ds.num_bone_param == 23 and len(ds.parents) == 24
    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    for _ in range(2):                                    # two epochs from the same generator
        want = [b.tolist() for b in torch.utils.data.DataLoader(_Index(len(ds)), batch_size, shuffle=shuffle,
                                                                 drop_last=drop_last, generator=g1)]
        assert ds.batch_order(batch_size, shuffle, drop_last, generator=g2) == want
    assert torch.equal(g1.get_state(), g2.get_state())


def test_getitem_refuses_dataloader_workers(tmp_path, monkeypatch):
    from enarf_gan_amd.dataset.dataset import HumanPoseDataset
    PG.write_cache(PG.load(), "cache32", str(tmp_path))
    ds = HumanPoseDataset(size=64, data_root=str(tmp_path))
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="batches"):
        ds[0]
