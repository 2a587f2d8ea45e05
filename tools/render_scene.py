#!/usr/bin/env python3
"""Several identities of an ENARF-GAN snapshot in one picture, composed on the device: TriNARFGenerator.render_scene (the
avatars marched on the same rays, one scene_composite launch that integrates their media over the merged samples, so
that limbs in front of and behind another body come out right) and one copy of the finished image to the host.

  python tools/render_scene.py --snapshot snapshot_latest.pth --sample-data sample_data.pickle --canonical canonical.npy \\
      --entries 0,7,19 --shift 0.5 --out group.png                  # three people side by side, one PNG (PIL)
  python tools/render_scene.py ... --out group.npy                   # the (S, S, 3) uint8 image as an array
  python tools/render_scene.py ... --instances --out group.png       # also group_instances.png / .npy: who owns each pixel
  python tools/render_scene.py ... --keys "0,7;3,12" --num 48 --out frames/   # the group in motion (render_scene_animation)

The poses, the camera and the bone lengths are entries of a sample_data.pickle (formats.read_sample_data; the camera
of the first entry); `--canonical` is the canonical pose (24, 4, 4) the model was trained with. The generator is built
as tools/animate.py builds it and the snapshot's weights are loaded into it. Avatar k gets the latent of seed `--seed` +
k and is moved `--shift` (k - (K - 1) / 2) metres along the camera's x axis, so that entries recorded one at a time
stand next to each other. `--instances` writes the instance map in the colours of semantic_palette(K) over white (with
.npy: the int32 map itself, -1 where no avatar reaches `--threshold`). `--keys` takes one comma-separated list of key
entries an avatar, the lists separated by semicolons, and renders `--num` frames; `num` must be a multiple of the number
of keys (with --no-loop: of the number of keys minus one)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from enarf_gan_amd import formats, ops, synth  # noqa: E402
from enarf_gan_amd.models.generator import TriNARFGenerator  # noqa: E402


def shifted(poses, shift, k, K):
    """joint-to-camera poses (..., 24, 4, 4) moved shift (k - (K - 1) / 2) along x"""
    out = poses.clone()
    out[..., 0, 3] += shift * (k - (K - 1) / 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--snapshot", required=True)
    ap.add_argument("--sample-data", required=True)
    ap.add_argument("--canonical", required=True, help="canonical pose, .npy (24, 4, 4)")
    ap.add_argument("--entries", default="0,1", help="comma-separated entries of the sample data, one an avatar")
    ap.add_argument("--keys", default=None, help="animation: key entries of each avatar, 'a,b;c,d' (overrides --entries)")
    ap.add_argument("--num", type=int, default=48, help="animation: frames")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--frames-per-batch", type=int, default=8)
    ap.add_argument("--shift", type=float, default=0.5, help="metres between neighbouring avatars along the camera's x axis")
    ap.add_argument("--seed", type=int, default=0, help="seed of the first avatar's latent; avatar k takes seed + k")
    ap.add_argument("--truncation-psi", type=float, default=0.4)
    ap.add_argument("--avatars-per-batch", type=int, default=None)
    ap.add_argument("--threshold", type=float, default=0.5, help="mask below which a pixel belongs to no avatar")
    ap.add_argument("--black-background", action="store_true")
    ap.add_argument("--instances", action="store_true", help="also write the instance map")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--z-dim", type=int, default=256)
    ap.add_argument("--nc", type=int, default=48)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--origin-location", default="center_fixed")
    ap.add_argument("--out", required=True, help="a .png or .npy path; with --keys a directory for PNGs or a .npy path")
    args = ap.parse_args()

    dev = torch.device("cuda")
    data = formats.read_sample_data(args.sample_data)
    groups = [[int(e) for e in g.split(",")] for g in args.keys.split(";")] if args.keys else [[int(e)] for e in args.entries.split(",")]
    K = len(groups)
    cfg = synth.AttrDict(z_dim=args.z_dim, background_ratio=0.7, crop_background=True, pretrained_background=False,
                         nerf_params=synth.nerf_config(Nc=args.nc, Nf=args.nf, origin_location=args.origin_location,
                                                       constant_triplane=False))
    gen = TriNARFGenerator(cfg, args.size, 24, synth.SMPL_PARENTS, 23, black_background=args.black_background)
    gen.register_canonical_pose(np.load(args.canonical))
    report = formats.load_generator_snapshot(args.snapshot, gen)
    print(f"snapshot: {len(report.loaded)} tensors loaded, {len(report.missing)} missing, {len(report.ignored)} ignored"
          + (f", iteration {report.iteration}" if report.iteration is not None else ""), file=sys.stderr)
    gen = gen.to(dev).eval()

    first = [g[0] for g in groups]
    bone_length = torch.from_numpy(data.bone_length[first].astype(np.float32)).to(dev)
    intrinsics = torch.from_numpy(data.intrinsics[first[0]].astype(np.float32)).to(dev)
    shares = 3 if args.black_background else 4
    z = torch.cat([torch.randn(1, args.z_dim * shares, generator=torch.Generator().manual_seed(args.seed + k)) for k in range(K)]).to(dev)
    stem = args.out[:-4] if args.out.endswith((".npy", ".png")) else args.out.rstrip("/")
    if args.keys:
        keys = [shifted(torch.from_numpy(data.pose_3d[g].astype(np.float64)), args.shift, k, K).to(dev) for k, g in enumerate(groups)]
        frames, _, instances, _ = gen.render_scene_animation(keys, bone_length, intrinsics, z, num=args.num, loop=not args.no_loop,
                                                             truncation_psi=args.truncation_psi,
                                                             frames_per_batch=args.frames_per_batch, threshold=args.threshold)
        painted = ops.compose_frames(gen._instance_image(instances, K), torch.ones_like(instances, dtype=torch.float32), 0.0,
                                     return_masks=False) if args.instances else None
    else:
        pose = torch.cat([shifted(torch.from_numpy(data.pose_3d[g].astype(np.float32)), args.shift, k, K) for k, g in enumerate(groups)]).to(dev)
        K_inv = torch.linalg.inv_ex(intrinsics.reshape(-1, 3, 3)[:1]).inverse
        image, mask, instances, colours = gen.render_scene(pose, bone_length, z, K_inv, truncation_psi=args.truncation_psi,
                                                           return_instances=True, avatars_per_batch=args.avatars_per_batch,
                                                           threshold=args.threshold)
        frames = ops.compose_frames(image, torch.ones_like(mask), 0.0, return_masks=False)          # the image is composed already
        painted = ops.compose_frames(colours, torch.ones_like(mask), 0.0, return_masks=False) if args.instances else None
    frames = frames.cpu().numpy()                                       # the device-to-host copies
    instances = instances.cpu().numpy() if args.instances else None
    painted = painted.cpu().numpy() if args.instances else None
    if args.out.endswith(".npy"):
        np.save(args.out, frames if args.keys else frames[0])
        if args.instances:
            np.save(stem + "_instances.npy", instances if args.keys else instances[0])
        print(args.out, frames.shape, file=sys.stderr)
        return
    from PIL import Image
    if not args.keys:
        Image.fromarray(frames[0]).save(args.out)
        if args.instances:
            Image.fromarray(painted[0]).save(stem + "_instances.png")
        print(f"{args.out}: {K} avatars, {frames.shape[1]} x {frames.shape[2]}", file=sys.stderr)
        return
    os.makedirs(args.out, exist_ok=True)
    for i, frame in enumerate(frames):
        Image.fromarray(frame).save(os.path.join(args.out, f"frame_{i:04d}.png"))
        if args.instances:
            Image.fromarray(painted[i]).save(os.path.join(args.out, f"instances_{i:04d}.png"))
    print(f"{args.out}: {len(frames)} PNGs of {frames.shape[1]} x {frames.shape[2]}, {K} avatars", file=sys.stderr)


if __name__ == "__main__":
    main()
