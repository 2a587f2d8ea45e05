#!/usr/bin/env python3
"""Generate tests/golden/bone_mask.npz by running the REFERENCE's own dataset/utils_3d.py and dataset/dataset.py on
the CPU, the way make_golden.py does: the reference checkout is put on sys.path and its modules are imported
unmodified. dataset.py imports blosc, which this path never calls: a placeholder module stands in for it.

  python tests/golden/make_golden_bone_mask.py --reference PATH_TO_REFERENCE_CHECKOUT

Recorded, on seeded synth.random_pose poses and synth.intrinsics cameras:
  * create_mask(hpp, add_blank_part(pose_to_image_coord(...))) for fp32 and fp64 caches, S = 64 and 128, thickness
    0.5 and 1.5: masks and keypoint masks as packed bits, disparities as fp32; part disparities for one frame at 64;
  * an edge pose: a joint behind the camera, one far off screen, keypoints across all four borders;
  * the SMPLProperty tables and create_mask's part grouping;
  * HumanPoseDataset items from two small pose-only cache.pickle files the script writes (fp32 without a camera, fp64
    with camera_rotation / camera_translation and a canonical.npy).
The GPU tests read only the .npz.
"""
import argparse
import os
import pickle
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from enarf_gan_amd import synth  # noqa: E402

N_RANDOM = 3
SIZES = (64, 128)
THICKNESS = (0.5, 1.5)


def edge_pose(size):
    """a random pose whose joints 20-23 sit across the left, right, top and bottom borders, 15 far off screen and 10
    behind the camera (z < 0)"""
    pose = synth.random_pose(1, seed=77)[0][0].numpy().astype(np.float64)
    K = synth.intrinsics(size)[0][0].numpy().astype(np.float64)
    f, c = K[0, 0], K[0, 2]
    for j, (px, py) in {20: (-0.3, 0.4 * size), 21: (size - 0.7, 0.5 * size), 22: (0.45 * size, -0.2),
                        23: (0.55 * size, size - 0.6), 15: (-3.0 * size, -2.0 * size)}.items():
        z = pose[j, 2, 3]
        pose[j, 0, 3] = (px - c) * z / f
        pose[j, 1, 3] = (py - c) * z / f
    pose[10, 2, 3] = -0.5
    return pose


def frames(dtype, size):
    poses = synth.random_pose(N_RANDOM, seed=1234)[0].numpy().astype(np.float64)
    if dtype == np.float64:        # genuinely fp64 values, not widened fp32 ones
        rs = np.random.RandomState(5)
        poses[:, :, :3, 3] += rs.normal(0, 1e-3, size=poses[:, :, :3, 3].shape)
    if size == 64:
        poses = np.concatenate([poses, edge_pose(size)[None]])
    K = np.broadcast_to(synth.intrinsics(size)[0][0].numpy().astype(np.float64), (len(poses), 3, 3))
    return poses.astype(dtype), np.ascontiguousarray(K).astype(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    blosc = types.ModuleType("blosc")                   # imported by dataset.py, never called on this path
    sys.modules["blosc"] = blosc
    from dataset import dataset as ref_dataset
    from dataset import utils_3d as ref_utils

    hpp = ref_dataset.SMPLProperty()
    add_blank_part = ref_dataset.HumanPoseDataset.add_blank_part
    out = {"prev_seq": np.array(hpp.prev_seq), "is_blank": np.array(hpp.is_blank),
           "valid_keypoints": np.array(hpp.valid_keypoints),
           "bone_group_ids": np.array([hpp.prev_seq[i] if hpp.is_blank[i] else i for i in hpp.prev_seq if i >= 0]),
           "blank_idx": np.array(add_blank_part(None, np.arange(24)[None, :, None, None] * np.ones((1, 24, 4, 4)),
                                                np.zeros((1, 3, 24)))[0][0, :, 0, 0].astype(np.int64))}
    out["part_ids"] = np.array(sorted(set(out["bone_group_ids"].tolist())))
    cases = []
    for dtype in (np.float32, np.float64):
        for size in SIZES:
            poses, Ks = frames(dtype, size)
            for t in THICKNESS:
                name = f"{np.dtype(dtype).name}_{size}_t{t}"
                cases.append(name)
                rec = {"disparity": [], "mask": [], "keypoint_mask": [], "joint_pos": []}
                for b in range(len(poses)):
                    jpi = ref_utils.pose_to_image_coord(poses[b], Ks[b])
                    jmc_, jpi_ = add_blank_part(None, poses[b][None], jpi)
                    disp, mask, part, key = ref_utils.create_mask(hpp, jmc_, jpi_, size, thickness=t)
                    rec["disparity"].append(disp)
                    rec["mask"].append(mask)
                    rec["keypoint_mask"].append(key)
                    rec["joint_pos"].append(jpi[0, :2].T)
                    if size == 64 and t == 0.5 and b == 0:
                        out[f"{name}_part_disparity"] = part
                out[f"{name}_poses"], out[f"{name}_K"] = poses, Ks
                out[f"{name}_disparity"] = np.stack(rec["disparity"])
                out[f"{name}_joint_pos"] = np.stack(rec["joint_pos"])
                for k in ("mask", "keypoint_mask"):
                    m = np.stack(rec[k])
                    assert set(np.unique(m)) <= {0.0, 1.0}
                    out[f"{name}_{k}_bits"], out[f"{name}_{k}_shape"] = np.packbits(m.astype(bool)), np.array(m.shape)
    out["cases"] = np.array(cases)

    # HumanPoseDataset on two pose-only caches
    rs = np.random.RandomState(9)
    n = 5
    pose_w = synth.random_pose(n, seed=4321)[0].numpy()
    K = synth.intrinsics(64, n)[0].numpy()
    caches = {"cache32": {"camera_intrinsic": K.astype(np.float32), "smpl_pose": pose_w.astype(np.float32)}}
    rot = np.stack([synth._axis_angle_to_matrix(rs.normal(0, 0.05, 3)) for _ in range(n)])
    caches["cache64"] = {"camera_intrinsic": K.astype(np.float64),
                         "smpl_pose": pose_w.astype(np.float64) + rs.normal(0, 1e-3, (n, 24, 4, 4)) * (np.arange(4) == 3),
                         "camera_rotation": rot, "camera_translation": rs.normal(0, 0.05, (n, 3, 1))}
    canonical = synth.random_pose(1, seed=3)[0].numpy()[0].astype(np.float32)
    items = [0, 3, 7, 11]                                          # indices past N wrap (i % N)
    for cname, d in caches.items():
        for k, v in d.items():
            out[f"{cname}__{k}"] = v
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "cache.pickle"), "wb") as f:
                pickle.dump(d, f)
            if cname == "cache64":
                np.save(os.path.join(tmp, "canonical.npy"), canonical)
            ds = ref_dataset.HumanPoseDataset(size=64, data_root=tmp, num_repeat_in_epoch=3)
            assert len(ds) == 3 * n
            for i in items:
                it = ds[i]
                for k, v in it.items():
                    v = np.asarray(v)
                    if k == "bone_mask":
                        out[f"{cname}_item{i}_bone_mask_bits"] = np.packbits(v.astype(bool))
                        assert set(np.unique(v)) <= {0.0, 1.0} and v.dtype == np.float32
                    else:
                        out[f"{cname}_item{i}_{k}"] = v
            if cname == "cache64":
                out["cache64_canonical"] = ds.canonical_pose
    out["dataset_items"] = np.array(items)
    path = os.path.join(HERE, "bone_mask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
