#!/usr/bin/env python3
"""Generate tests/golden/pose_interp.npz by running the REFERENCE's own libraries/NARF/pose_utils.py on the CPU, the way
make_golden_bone_mask.py does: the reference checkout is put on sys.path and its module is imported unmodified (it needs
scipy, for Slerp).

  python tests/golden/make_golden_pose_interp.py --reference PATH_TO_REFERENCE_CHECKOUT

Recorded (inputs and outputs only):
  * interpolate_pose on rigid key poses built by forward kinematics from random local rotations over the SMPL tree
    (tests/anim_reference.random_key_poses; every consecutive pair's relative angle is below pi - 0.05, where the short
    arc is unique): (K, num, loop) = (3, 12, yes), (3, 12, no), (2, 7, no), (5, 8, no), (1, 5, yes), (2, 2, no) and
    (4, 100, yes) with large rotations;
  * that it raises ValueError for (3, 10, loop) and (3, 9, no loop);
  * rotation_matrix, rotate_pose_by_angle and rotate_mesh_by_angle on fp32 tensors.
The tests read only the .npz.
"""
import argparse
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

# tests/anim_reference.py by path: tests/ itself stays off sys.path, its libraries.py would hide the reference's package
_spec = importlib.util.spec_from_file_location("anim_reference", os.path.join(os.path.dirname(HERE), "anim_reference.py"))
A = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(A)

# (K, num, loop, spread of the random local rotation vectors)
CASES = [(3, 12, True, 0.6), (3, 12, False, 0.6), (2, 7, False, 0.6), (5, 8, False, 0.6), (1, 5, True, 0.6),
         (2, 2, False, 0.6), (4, 100, True, 2.0)]
RAISES = [(3, 10, True), (3, 9, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from libraries.NARF import pose_utils as ref

    rng = np.random.default_rng(20240607)
    out = {"parents": A.SMPL_PARENTS.astype(np.int32), "cases": np.array([[K, num, int(loop)] for K, num, loop, _ in CASES])}
    for n, (K, num, loop, spread) in enumerate(CASES):
        keys = A.random_key_poses(rng, K, spread=spread)
        out[f"case{n}_keys"] = keys
        out[f"case{n}_out"] = ref.interpolate_pose(keys, A.SMPL_PARENTS, num, loop)
        assert out[f"case{n}_out"].shape == (num, 24, 4, 4) and out[f"case{n}_out"].dtype == np.float64
    raised = []
    for K, num, loop in RAISES:
        try:
            ref.interpolate_pose(A.random_key_poses(rng, K), A.SMPL_PARENTS, num, loop)
            raised.append("")
        except Exception as e:      # noqa: BLE001
            raised.append(type(e).__name__)
    out["raises"], out["raised"] = np.array([[K, num, int(loop)] for K, num, loop in RAISES]), np.array(raised)

    pose = torch.from_numpy(np.stack([A.random_key_poses(rng, 1)[0] for _ in range(3)]).astype(np.float32))
    angle = torch.tensor([0.0, np.pi / 2, 2.2173], dtype=torch.float32)
    verts = torch.from_numpy(rng.normal(size=(37, 3)).astype(np.float32))
    faces = torch.from_numpy(rng.integers(0, 37, size=(20, 3)))
    out["helper_pose"], out["helper_angle"] = pose.numpy(), angle.numpy()
    out["helper_rotation_matrix"] = ref.rotation_matrix(angle).numpy()
    out["helper_rotate_pose_by_angle"] = ref.rotate_pose_by_angle(pose, angle).numpy()
    out["helper_vertices"], out["helper_faces"] = verts.numpy(), faces.numpy()
    mesh = ref.rotate_mesh_by_angle(pose[:1], (verts, faces), angle[2:])
    assert len(mesh) == 2 and torch.equal(mesh[1], faces)
    out["helper_rotate_mesh_by_angle"] = mesh[0].numpy()
    path = os.path.join(HERE, "pose_interp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
