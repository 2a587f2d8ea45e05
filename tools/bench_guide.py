#!/usr/bin/env python3
"""Cost of the GAN's mask-guidance loss on the device, one JSON line:

  loss_hip_us / loss_torch_us   forward + backward of the loss at (32, 128, 128) against a (32, 128, 128) bone mask,
                                ratio 0.7 (the training shape), as ops.mask_guidance_loss (libenarf_guide.so) and as
                                models.loss.nerf_patch_loss (topk + scatter + compare + reductions through autograd),
                                same process, same inputs, alternating rounds
  pooled_hip_us / _torch_us     the same at (8, 64, 64) against a (8, 128, 128) bone mask (pooled by 2 in the kernel)

Each figure is the median over ROUNDS rounds of the mean time of ITERS back-to-back calls between two device events,
after a warm-up round; `spread` gives the (max - min) / median of the rounds. `--once hip|torch` runs ITERS calls of
one candidate and nothing else: the process to put under a kernel trace for the launch counts."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from enarf_gan_amd import ops
from enarf_gan_amd.models.loss import nerf_patch_loss

ROUNDS = 5
ITERS = 50


def timed(fn, iters):
    """mean milliseconds per call over `iters` calls, between device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def rounds(fns, iters):
    """{name: (median, spread)} with the candidates alternating inside every round"""
    for fn in fns.values():
        timed(fn, max(iters // 4, 2))                      # warm-up
    samples = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            samples[k].append(timed(fn, iters))
    out = {}
    for k, v in samples.items():
        v = sorted(v)
        out[k] = (v[len(v) // 2], (v[-1] - v[0]) / v[len(v) // 2])
    return out


def candidates(shape, bone_shape, ratio):
    g = torch.Generator(device="cuda").manual_seed(0)
    mask = torch.rand(shape, device="cuda", generator=g).requires_grad_()
    bone = (torch.rand(bone_shape, device="cuda", generator=g) > 0.97).float()

    def hip():
        mask.grad = None
        ops.mask_guidance_loss(mask, bone, ratio).backward()

    def plain():
        mask.grad = None
        nerf_patch_loss(mask, bone, ratio).backward()
    return {"hip": hip, "torch": plain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", choices=("hip", "torch"), default=None)
    ap.add_argument("--iters", type=int, default=ITERS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_guide needs the GPU"
    full = candidates((32, 128, 128), (32, 128, 128), 0.7)
    if args.once:
        for _ in range(args.iters):
            full[args.once]()
        torch.cuda.synchronize()
        print(json.dumps({"once": args.once, "calls": args.iters}))
        return
    res, spread = {}, {}
    for tag, fns in (("loss", full), ("pooled", candidates((8, 64, 64), (8, 128, 128), 0.7))):
        for k, (median, s) in rounds(fns, args.iters).items():
            res[f"{tag}_{k}_us"], spread[f"{tag}_{k}_us"] = median * 1e3, s
    print(json.dumps({"metric": "mask-guidance loss forward + backward, microseconds per call (not the headline metric)",
                      **{k: round(v, 2) for k, v in res.items()}, "spread": {k: round(v, 3) for k, v in spread.items()},
                      "rounds": ROUNDS, "iters": args.iters, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
