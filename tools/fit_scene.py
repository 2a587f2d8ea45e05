#!/usr/bin/env python3
"""Fit the poses of several identities of an ENARF-GAN snapshot to one picture with all of them in it (models/fit.fit_scene:
Adam on per-joint rotation residuals and a root translation an avatar, through render_scene_posable and the photometric
loss; the avatars are composed depth-correctly and the gradient of the composite is the HIP kernel's,
ops.scene_composite_bwd, as the pose gradient of every avatar's query is ops.query_pose_bwd).

  python tools/fit_scene.py --snapshot snapshot_latest.pth --sample-data sample_data.pickle --canonical canonical.npy \\
      --entries 0,7 --shift 0.5 --target group.npy --steps 200 --lr 5e-3 --out fitted_poses.npy

The starting poses, the camera (of the first entry) and the bone lengths are the entries --entries of a
sample_data.pickle (formats.read_sample_data), avatar k moved `--shift` (k - (K - 1) / 2) metres along the camera's x
axis and given the latent of seed `--seed` + k, as tools/render_scene.py places and draws them; `--canonical` is the
canonical pose (24, 4, 4) the model was trained with. The target is a .npy image of the model's size: (S, S, 3) or
(3, S, S), uint8 (0..255) or floating point in [-1, 1]; its foreground mask is `--mask` ((S, S), non-zero = a person) or,
without one, every pixel that differs from the background colour --background. `--instances` is an (S, S) integer map of
the avatar that owns each pixel (-1 for none, as tools/render_scene.py --instances writes it): with it the instance
masses are supervised too, weighted by --instance-weight. Writes the fitted poses (K, 24, 4, 4) fp32 to --out and prints
one JSON line with the loss of the first and the last step. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from enarf_gan_amd import formats, synth  # noqa: E402
from enarf_gan_amd.models.fit import fit_scene  # noqa: E402
from enarf_gan_amd.models.generator import TriNARFGenerator  # noqa: E402
from fit_pose import read_target  # noqa: E402
from render_scene import shifted  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--snapshot", required=True)
    ap.add_argument("--sample-data", required=True)
    ap.add_argument("--canonical", required=True, help="canonical pose, .npy (24, 4, 4)")
    ap.add_argument("--entries", default="0,1", help="comma-separated entries of the sample data, one an avatar")
    ap.add_argument("--shift", type=float, default=0.5, help="metres between neighbouring avatars along the camera's x axis")
    ap.add_argument("--target", required=True, help="the picture, .npy")
    ap.add_argument("--mask", default=None, help="its foreground mask, .npy (S, S)")
    ap.add_argument("--instances", default=None, help="the avatar that owns each pixel, .npy (S, S) integers, -1 for none")
    ap.add_argument("--instance-weight", type=float, default=1.0)
    ap.add_argument("--background", type=float, default=-1.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0, help="seed of the first avatar's latent; avatar k takes seed + k")
    ap.add_argument("--truncation-psi", type=float, default=0.4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--z-dim", type=int, default=256)
    ap.add_argument("--nc", type=int, default=48)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--origin-location", default="center_fixed")
    ap.add_argument("--out", required=True, help="the fitted poses, .npy (K, 24, 4, 4)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_scene.py renders on the GPU; none is available (nothing was fitted)")

    dev = torch.device("cuda")
    data = formats.read_sample_data(args.sample_data)
    entries = [int(e) for e in args.entries.split(",")]
    K = len(entries)
    cfg = synth.AttrDict(z_dim=args.z_dim, background_ratio=0.7, crop_background=True, pretrained_background=False,
                         nerf_params=synth.nerf_config(Nc=args.nc, Nf=args.nf, origin_location=args.origin_location,
                                                       constant_triplane=False))
    gen = TriNARFGenerator(cfg, args.size, 24, synth.SMPL_PARENTS, 23, black_background=True)
    gen.register_canonical_pose(np.load(args.canonical))
    report = formats.load_generator_snapshot(args.snapshot, gen)
    print(f"snapshot: {len(report.loaded)} tensors loaded, {len(report.missing)} missing, {len(report.ignored)} ignored",
          file=sys.stderr)
    gen = gen.to(dev).eval()

    pose = torch.cat([shifted(torch.from_numpy(data.pose_3d[e:e + 1].astype(np.float32)), args.shift, k, K)
                      for k, e in enumerate(entries)]).to(dev)
    bone_length = torch.from_numpy(data.bone_length[entries].astype(np.float32)).to(dev)
    inv_intrinsics = torch.inverse(torch.from_numpy(data.intrinsics[entries[0]].astype(np.float32)))[None].to(dev)
    target = read_target(args.target, args.size).to(dev)
    if args.mask:
        mask = torch.from_numpy((np.load(args.mask, allow_pickle=False) != 0).astype(np.float32))[None].to(dev)
    else:
        mask = (target != args.background).any(dim=1).float()
    owner = None
    if args.instances:
        owner = torch.from_numpy(np.load(args.instances, allow_pickle=False).astype(np.int64))[None].to(dev)
        if tuple(owner.shape) != (1, args.size, args.size):
            raise SystemExit(f"{args.instances}: map {tuple(owner.shape[1:])}, expected ({args.size}, {args.size})")
    z = torch.cat([torch.randn(1, args.z_dim * 3, generator=torch.Generator().manual_seed(args.seed + k)) for k in range(K)]).to(dev)
    z_tri, z_rend, _ = gen._latent_parts(z)
    fitted, history = fit_scene(gen, target, mask, pose, bone_length, (z_tri, z_rend), inv_intrinsics, steps=args.steps,
                                lr=args.lr, n_rays=args.rays, background=args.background, target_instance=owner,
                                instance_weight=args.instance_weight, truncation_psi=args.truncation_psi)
    np.save(args.out, fitted.cpu().numpy())
    h = history.cpu()
    print(json.dumps({"out": args.out, "avatars": K, "steps": args.steps, "lr": args.lr, "rays": args.rays,
                      "loss_first": float(h[0]), "loss_last": float(h[-1]), "loss_min": float(h.min())}))


if __name__ == "__main__":
    main()
