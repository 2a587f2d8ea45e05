#!/usr/bin/env python3
"""The paper's 3-D metric for an ENARF-GAN snapshot: the mean squared error between the generator's disparity and the
ground-truth inverse depth of a depth cache (the reference's evaluation/compute_depth.py), with the running sums kept on
the device (models/evaluate.inverse_depth_error: ops.DepthError, two launches per batch, one host read at the end).

  python tools/eval_depth.py --snapshot snapshot_latest.pth --depth-cache NARF_GAN_depth_cache/cache.pickle \\
      --canonical neutral_canonical.npy --num-sample 10000
  python tools/eval_depth.py ... --disparity-npy disparity.npy      # the cache's maps, unpacked elsewhere: (N, S, S) fp32

The depth cache holds "camera_intrinsic" (N, 3, 3), "smpl_pose" (N, 24, 4, 4) and "disparity", N blosc-packed (S, S)
inverse-depth maps with 0 on background (preprocess_depth.py). The maps are read through formats.unpack_image, which
needs the third-party `blosc` package; where it is missing this tool says so and `--disparity-npy` takes the same maps as
one unpacked array. Samples are drawn in a shuffled order from --seed, a latent per sample from the same seed. Prints one
JSON line: inv_depth_mse (the reference's number), inv_depth_mse_fg (over the ground truth's foreground), iou of the
silhouettes, and the counts. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from enarf_gan_amd import formats, synth  # noqa: E402
from enarf_gan_amd.models.evaluate import inverse_depth_error  # noqa: E402
from enarf_gan_amd.models.generator import TriNARFGenerator  # noqa: E402


def read_disparity(cache_path, npy_path, count):
    """(N, S, S) fp32 ground-truth inverse depth, from --disparity-npy or the cache's packed entries"""
    if npy_path:
        maps = np.load(npy_path, allow_pickle=False)
    else:
        packed = formats._load_arrays(cache_path).get("disparity")
        if packed is None:
            raise SystemExit(f"{cache_path}: no 'disparity' entries: not a depth cache")
        try:
            maps = np.stack([formats.unpack_image(p) for p in packed])
        except ImportError as e:
            raise SystemExit(f"the cache's disparity maps are blosc-packed and blosc is not installed ({e}); unpack them "
                             "where it is and pass the (N, S, S) array with --disparity-npy") from None
    maps = np.asarray(maps, np.float32)
    if maps.ndim != 3 or maps.shape[1] != maps.shape[2] or len(maps) != count:
        raise SystemExit(f"ground-truth disparity {maps.shape}: expected ({count}, S, S)")
    return maps


def batches(poses, intrinsics, bone_length, disparity, order, batch_size):
    """the reference loader's dicts (SurrealPoseDepthDataset: the pose in camera space is the pose in world space)"""
    for a in range(0, len(order), batch_size):
        idx = order[a:a + batch_size]
        pose = torch.from_numpy(poses[idx].astype(np.float32))
        yield {"pose_3d": pose, "pose_3d_world": pose, "bone_length": torch.from_numpy(bone_length[idx].astype(np.float32)),
               "intrinsics": torch.from_numpy(intrinsics[idx].astype(np.float32)), "img": torch.from_numpy(disparity[idx])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--snapshot", required=True)
    ap.add_argument("--depth-cache", required=True, help="cache.pickle of the depth data set")
    ap.add_argument("--disparity-npy", default=None, help="the cache's disparity maps as one unpacked (N, S, S) array")
    ap.add_argument("--canonical", required=True, help="canonical pose, .npy (24, 4, 4)")
    ap.add_argument("--num-sample", type=int, default=10000)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--truncation-psi", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--black-background", action="store_true", help="a snapshot trained without a background generator")
    ap.add_argument("--z-dim", type=int, default=256)
    ap.add_argument("--nc", type=int, default=48)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--origin-location", default="center_fixed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_depth.py runs the generator on the GPU; none is available (nothing was evaluated)")

    cache = formats.read_pose_cache(args.depth_cache)
    disparity = read_disparity(args.depth_cache, args.disparity_npy, len(cache.intrinsics))
    if args.num_sample > len(disparity):
        raise SystemExit(f"--num-sample {args.num_sample} exceeds the cache's {len(disparity)} samples")
    size = disparity.shape[-1]
    joints = cache.pose_to_camera[..., :3, 3]
    bone_length = np.linalg.norm(joints[:, 1:] - joints[:, np.asarray(synth.SMPL_PARENTS)[1:]], axis=-1)[..., None]

    dev = torch.device("cuda")
    cfg = synth.AttrDict(z_dim=args.z_dim, background_ratio=0.7, crop_background=True, pretrained_background=False,
                         nerf_params=synth.nerf_config(Nc=args.nc, Nf=args.nf, origin_location=args.origin_location,
                                                       constant_triplane=False))
    gen = TriNARFGenerator(cfg, size, 24, synth.SMPL_PARENTS, 23, black_background=args.black_background)
    gen.register_canonical_pose(np.load(args.canonical))
    report = formats.load_generator_snapshot(args.snapshot, gen)
    print(f"snapshot: {len(report.loaded)} tensors loaded, {len(report.missing)} missing, {len(report.ignored)} ignored",
          file=sys.stderr)
    gen = gen.to(dev)

    rng = torch.Generator().manual_seed(args.seed)
    order = torch.randperm(len(disparity), generator=rng).numpy()[:args.num_sample]
    latents = torch.Generator(device=dev).manual_seed(args.seed)
    result = inverse_depth_error(gen, batches(cache.pose_to_camera, cache.intrinsics, bone_length, disparity, order,
                                              args.batch_size), args.num_sample, args.truncation_psi, generator=latents)
    print(json.dumps({"snapshot": args.snapshot, "num_sample": args.num_sample, "truncation_psi": args.truncation_psi,
                      "size": size, **result}))


if __name__ == "__main__":
    main()
