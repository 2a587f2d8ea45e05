#!/usr/bin/env python3
"""A 96-frame animation of one identity at 128 x 128, two routes to the same uint8 frames on the host:

  --route a   TriNARFGenerator.render_animation: one interpolate_pose launch, the tri-plane and the background once, the
              frames marched 8 at a time on the shared tri-plane, one compose_frames launch per chunk, one copy of the
              finished bytes to the host;
  --route b   the reference demo's route on this project (ENARF_GAN_demo.py:60-79): interpolate_pose in numpy on the host
              (tests/anim_reference.py, the float64 restatement of the reference's), the poses uploaded, one gen(...) call
              per frame - tri-plane and background network included, as the demo runs them - and per frame
              .cpu().numpy(), transpose, * 127.5 + 127.5, clip, astype(uint8).

The generator is the one tools/bench_gan_step.py builds (its own StyleGAN2-ADA tri-plane producer and background
network, random weights, synthetic key poses). Wall-clock time of the whole route between two synchronisations, median
of --runs after a warm-up run, and the number of kernel launches of one run (torch.profiler, a run of its own). Prints
one JSON line. Route (b) is the yardstick; run each route as a process of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import anim_reference as A  # noqa: E402
from enarf_gan_amd import synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle  # noqa: E402
from enarf_gan_amd.models.generator import TriNARFGenerator  # noqa: E402


def build(S, Nc, Nf, dev):
    zd = 256
    sc = synth.make_scene(S, 1, "center_fixed", zd)
    cfg = synth.AttrDict(z_dim=zd, background_ratio=0.7, crop_background=True, pretrained_background=False,
                         nerf_params=synth.nerf_config(Nc=Nc, Nf=Nf, constant_triplane=False))
    gen = TriNARFGenerator(cfg, S, 24, sc["parents"], 23)
    gen.register_canonical_pose(sc["canonical_pose"])
    gen = gen.to(dev).eval()
    first = sc["pose_to_camera"][:1]
    keys = torch.cat([rotate_pose_by_angle(first, torch.tensor([a])) for a in (0.0, 0.6, -0.5)]).double()
    z = torch.randn(1, 4 * zd, generator=torch.Generator().manual_seed(0)).to(dev)
    return gen, sc, keys, z


def route_a(gen, sc, keys, z, num, dev):
    frames, _, _ = gen.render_animation(keys.to(dev), sc["bone_length"][:1].to(dev), sc["intrinsics"][:1].to(dev), z, num=num,
                                        loop=True, truncation_psi=0.4, frames_per_batch=8)
    return frames.cpu().numpy()


def route_b(gen, sc, keys, z, num, dev):
    poses = torch.from_numpy(A.interpolate_pose(keys.numpy(), sc["parents"], num, True)).float().to(dev)
    bone_length, K_inv = sc["bone_length"][:1].to(dev), sc["inv_intrinsics"][:1].to(dev)
    out = []
    with torch.no_grad():
        for i in range(num):
            image = gen(poses[i:i + 1], None, bone_length, z, K_inv, truncation_psi=0.4)[0]
            image = image.cpu().numpy()[0].transpose(1, 2, 0) * 127.5 + 127.5
            out.append(np.clip(image, 0, 255).astype("uint8"))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("a", "b"), required=True)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--nc", type=int, default=48)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen, sc, keys, z = build(args.size, args.nc, args.nf, dev)
    route = route_a if args.route == "a" else route_b
    frames = route(gen, sc, keys, z, args.frames, dev)                 # warm-up
    assert frames.shape == (args.frames, args.size, args.size, 3) and frames.dtype == np.uint8
    times = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        route(gen, sc, keys, z, args.frames, dev)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            route(gen, sc, keys, z, args.frames, dev)
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name
                       and "emset" not in e.name)
    except Exception as e:      # noqa: BLE001 - the count is a side figure; the times stand without it
        print(f"kernel count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
    print(json.dumps({"tool": "bench_animation", "route": args.route, "frames": args.frames, "size": args.size, "Nc": args.nc,
                      "Nf": args.nf, "seconds_median": sorted(times)[len(times) // 2], "seconds_runs": times,
                      "ms_per_frame": sorted(times)[len(times) // 2] * 1e3 / args.frames, "kernel_launches": launches,
                      "foreground_fraction": float((frames != frames[:, :1, :1]).any(-1).mean())}), flush=True)


if __name__ == "__main__":
    main()
