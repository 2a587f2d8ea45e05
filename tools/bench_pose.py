#!/usr/bin/env python3
"""Bone masks of the pose prior (libenarf_pose.so) against the CPU they replace.

Device time per batch, from events around 20 calls after a warm-up (median of 5 such runs), for B = 32 at 128 with the
mask only, B = 12 at 512 with the mask only and B = 12 at 512 with every output. Beside them, the CPU baseline: the
float64 numpy restatement of the same contract (tests/bone_mask_reference.py; numpy's elementwise kernels run on one
thread) per frame on the host. Poses: synth.random_pose, cameras: synth.intrinsics. Prints one line per case."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bone_mask_reference as R  # noqa: E402
from enarf_gan_amd import synth  # noqa: E402
from enarf_gan_amd.dataset.utils_3d import bone_masks  # noqa: E402

ALL = ("mask", "disparity", "part_disparity", "keypoint_mask", "pose_2d")
CASES = [(32, 128, ("mask",)), (12, 512, ("mask",)), (12, 512, ALL)]
CALLS, RUNS = 20, 5


def inputs(B, S):
    pose = synth.random_pose(B, seed=5)[0].double().cuda()
    K = synth.intrinsics(S, B)[0].double().cuda()
    return pose, K


for B, S, outputs in CASES:
    pose, K = inputs(B, S)
    for _ in range(3):
        bone_masks(pose, K, S, 0.5, outputs)
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            bone_masks(pose, K, S, 0.5, outputs)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / CALLS)
    ms = sorted(times)[RUNS // 2]
    frac = float(bone_masks(pose, K, S, 0.5)["mask"].mean())
    print(f"device: B = {B}, S = {S}, outputs = {'+'.join(outputs)}: {ms * 1e3:.1f} us per batch "
          f"({ms * 1e3 / B:.2f} us per frame), mask cover {frac * 100:.1f} %", flush=True)

for S, reps in ((128, 5), (512, 2)):
    pose, K = (t.cpu().numpy() for t in inputs(1, S))
    R.masks(pose[0], K[0], S, 0.5)
    t0 = time.perf_counter()
    for _ in range(reps):
        R.masks(pose[0], K[0], S, 0.5)
    per = (time.perf_counter() - t0) / reps
    print(f"CPU baseline (numpy restatement, one thread, every output): S = {S}: {per * 1e3:.1f} ms per frame",
          flush=True)
