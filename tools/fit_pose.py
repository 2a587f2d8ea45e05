#!/usr/bin/env python3
"""Fit the pose of one identity of an ENARF-GAN snapshot to a picture (models/fit.fit_pose: Adam on per-joint rotation
residuals and a root translation, through render_posable and the photometric loss; the pose gradient is the HIP kernel's,
ops.query_pose_bwd).

  python tools/fit_pose.py --snapshot snapshot_latest.pth --sample-data sample_data.pickle --canonical canonical.npy \\
      --entry 3 --target picture.npy --steps 200 --lr 5e-3 --out fitted_pose.npy

The starting pose, the camera and the bone lengths are entry --entry of a sample_data.pickle (formats.read_sample_data);
`--canonical` is the canonical pose (24, 4, 4) the model was trained with. The target is a .npy image of the model's size:
(S, S, 3) or (3, S, S), uint8 (0..255) or floating point in [-1, 1]; its foreground mask is `--mask` ((S, S), non-zero =
person) or, without one, every pixel that differs from the background colour --background. The identity is the latent
drawn from --seed (as tools/animate.py draws it). Writes the fitted pose (24, 4, 4) fp32 to --out and prints one JSON line
with the loss of the first and the last step. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from enarf_gan_amd import formats, synth  # noqa: E402
from enarf_gan_amd.models.fit import fit_pose  # noqa: E402
from enarf_gan_amd.models.generator import TriNARFGenerator  # noqa: E402


def read_target(path, size):
    """(1, 3, S, S) fp32 in [-1, 1]"""
    img = np.load(path, allow_pickle=False)
    if img.ndim == 3 and img.shape[-1] == 3:
        img = img.transpose(2, 0, 1)
    if img.shape != (3, size, size):
        raise SystemExit(f"{path}: image {img.shape}, expected ({size}, {size}, 3) or (3, {size}, {size})")
    img = img.astype(np.float32) / 127.5 - 1.0 if img.dtype == np.uint8 else img.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(img))[None]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--snapshot", required=True)
    ap.add_argument("--sample-data", required=True)
    ap.add_argument("--canonical", required=True, help="canonical pose, .npy (24, 4, 4)")
    ap.add_argument("--entry", type=int, default=0, help="entry of the sample data: starting pose, camera, bone lengths")
    ap.add_argument("--target", required=True, help="the picture, .npy")
    ap.add_argument("--mask", default=None, help="its foreground mask, .npy (S, S)")
    ap.add_argument("--background", type=float, default=-1.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0, help="seed of the identity's latent")
    ap.add_argument("--truncation-psi", type=float, default=0.4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--z-dim", type=int, default=256)
    ap.add_argument("--nc", type=int, default=48)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--origin-location", default="center_fixed")
    ap.add_argument("--out", required=True, help="the fitted pose, .npy (24, 4, 4)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_pose.py renders on the GPU; none is available (nothing was fitted)")

    dev = torch.device("cuda")
    data = formats.read_sample_data(args.sample_data)
    cfg = synth.AttrDict(z_dim=args.z_dim, background_ratio=0.7, crop_background=True, pretrained_background=False,
                         nerf_params=synth.nerf_config(Nc=args.nc, Nf=args.nf, origin_location=args.origin_location,
                                                       constant_triplane=False))
    gen = TriNARFGenerator(cfg, args.size, 24, synth.SMPL_PARENTS, 23, black_background=True)
    gen.register_canonical_pose(np.load(args.canonical))
    report = formats.load_generator_snapshot(args.snapshot, gen)
    print(f"snapshot: {len(report.loaded)} tensors loaded, {len(report.missing)} missing, {len(report.ignored)} ignored",
          file=sys.stderr)
    gen = gen.to(dev).eval()

    e = args.entry
    pose = torch.from_numpy(data.pose_3d[e:e + 1].astype(np.float32)).to(dev)
    bone_length = torch.from_numpy(data.bone_length[e:e + 1].astype(np.float32)).to(dev)
    inv_intrinsics = torch.inverse(torch.from_numpy(data.intrinsics[e].astype(np.float32)))[None].to(dev)
    target = read_target(args.target, args.size).to(dev)
    if args.mask:
        mask = torch.from_numpy((np.load(args.mask, allow_pickle=False) != 0).astype(np.float32))[None].to(dev)
    else:
        mask = (target != args.background).any(dim=1).float()
    z = torch.randn(1, args.z_dim * 3, generator=torch.Generator().manual_seed(args.seed)).to(dev)
    z_tri, z_rend, _ = gen._latent_parts(z)
    fitted, history = fit_pose(gen, target, mask, pose, bone_length, (z_tri, z_rend), inv_intrinsics, steps=args.steps,
                               lr=args.lr, n_rays=args.rays, background=args.background, truncation_psi=args.truncation_psi)
    np.save(args.out, fitted[0].cpu().numpy())
    h = history.cpu()
    print(json.dumps({"out": args.out, "steps": args.steps, "lr": args.lr, "rays": args.rays,
                      "loss_first": float(h[0]), "loss_last": float(h[-1]), "loss_min": float(h.min())}))


if __name__ == "__main__":
    main()
