#!/usr/bin/env python3
"""Differentiable scenes (libenarf_sgrad.so), measured on the device. The settings are tools/bench_scene.py's.

  composite_bwd  ops.scene_composite_bwd (one launch of sgrad_composite_bwd_kernel, both outputs, all four upstream
                 gradients) at K = 2 and K = 4 avatars, Nf 64, 128 x 128 rays, on bench_scene's seeded sample lists,
                 beside the forward ops.scene_composite on the same inputs and against torch.autograd.grad through
                 bench_scene.torch_composite (fp32: a sort, K gathers, cumsums and their scatter-add backwards; its graph
                 is built once, only the backward is timed): time, kernel launches, compulsory bytes and GB/s of the
                 kernel, and the largest difference between the two gradients. The density gradients are compared at
                 the samples of positive density; at a sample of density exactly 0 (a fifth of them) the two differ by
                 design and the figure is given apart: the kernel returns the derivative from inside s >= 0, torch
                 differentiates the forward's `where(sigma > 0, ..., 0)` and drops the colour and instance terms of
                 segments without density;
  render         one rendering.render_scene_posable forward + backward with K avatars on the synthetic scene at 128 x 128
                 (Nc 48, Nf 64) beside K render_posable forward + backward calls of one avatar each;
  fit            one models.fit.fit_scene step at 1024 rays (the mean of 5 steps of one call, after a call to warm up);
each side timed with device events over --batch back-to-back calls, the sides taking turns, the median of --runs rounds
(after one warm-up call of every side). One JSON line per result, also appended to --log. Needs a GPU: there is no CPU
path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_scene import NF, SIZE, alternate, launches, samples, timed, torch_composite  # noqa: E402
from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NeRF.rendering import render_posable, render_scene, render_scene_posable  # noqa: E402
from enarf_gan_amd.models.fit import fit_scene  # noqa: E402
from enarf_gan_amd.models.narf import TriPlaneNARF  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r19_sgrad.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sgrad.py measures on the GPU; none is available (nothing was measured)")
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    emit({"device": torch.cuda.get_device_name(0), "runs": args.runs, "batch": args.batch})

    # ---- the backward kernel beside the forward kernel and against torch's autograd
    n = SIZE * SIZE
    for K in (2, 4):
        depth, density, color, valid = samples(K, n, NF, dev)
        g = torch.Generator(device=dev).manual_seed(1)
        up = [torch.randn(shape, device=dev, generator=g) for shape in ((1, 3, n), (1, n), (1, n), (1, K, n))]
        backward = lambda: ops.scene_composite_bwd(depth, density, color, valid, 1.0, *up)
        forward = lambda: ops.scene_composite(depth, density, color, valid)
        s, c = density.clone().requires_grad_(True), color.clone().requires_grad_(True)
        outs = torch_composite(depth, s, c, valid)[:4]
        loss = sum((o * u).sum() for o, u in zip(outs, up))
        by_torch = lambda: torch.autograd.grad(loss, (s, c), retain_graph=True)
        got, want = backward(), by_torch()
        ms = alternate({"scene_composite_bwd": backward, "scene_composite": forward, "torch_autograd_backward": by_torch},
                       args.runs, args.batch)
        mb = (K * n * NF * 5 * 4 + K * n + n * (3 + 1 + 1 + K) * 4 + K * n * NF * 4 * 4) / 1e6
        scale_s, scale_c = float(want[0].abs().max()), float(want[1].abs().max())
        emit({"what": "composite_bwd", "K": K, "Nf": NF, "rays": n, "ms_per_call": ms, "batch": args.batch,
              "backward_over_forward": round(ms["scene_composite_bwd"] / ms["scene_composite"], 2),
              "launches": {"scene_composite_bwd": launches(backward), "torch_autograd_backward": launches(by_torch)},
              "compulsory_MB": round(mb, 2), "GB_per_s": round(mb / ms["scene_composite_bwd"], 1),
              "max_abs_density_gradient_difference_over_max": float(((got.density - want[0]).abs() * (density > 0)).max()) / scale_s,
              "same_at_samples_of_zero_density": float(((got.density - want[0]).abs() * (density == 0)).max()) / scale_s,
              "max_abs_colour_gradient_difference_over_max": float((got.color - want[1]).abs().max()) / scale_c})
        del got, want, outs, loss, s, c

    # ---- render_scene_posable beside K render_posable calls, and one fit_scene step, on the synthetic scene
    sc = synth.make_scene(SIZE, 1, "center_fixed", 20)
    model = TriPlaneNARF(synth.nerf_config(origin_location="center_fixed"), 20, 24, parent=sc["parents"], num_bone_param=23)
    model.register_canonical_pose(sc["canonical_pose"])
    model.load_state_dict({f"mlp.{k}": v for k, v in sc["mlp"].items()}, strict=False)
    with torch.no_grad():
        model.tri_plane.copy_(sc["tri_plane"][:1])
    model = model.cuda().eval()
    K_inv = torch.linalg.inv_ex(sc["intrinsics"][:1].cuda().float()).inverse
    nc, nf = model.config.Nc, model.config.Nf
    pixels = sc["image_coord"].cuda()
    for K in (2, 4):
        pose = sc["pose_to_camera"].cuda().repeat(K, 1, 1, 1)
        pose[:, :, 0, 3] += torch.linspace(-0.6, 0.6, K, device=dev)[:, None]            # side by side, arms crossing
        pose[:, :, 2, 3] += torch.linspace(0.0, 0.4, K, device=dev)[:, None]
        bl, z = sc["bone_length"].cuda().repeat(K, 1, 1), sc["z_rend"].cuda().repeat(K, 1)
        pose.requires_grad_(True)

        def scene():
            pp, blp = model.transform_pose(pose, bl)
            c, m, d = render_scene_posable(model, pixels, pp, K_inv, Nc=nc, Nf=nf, model_input={"z": None, "z_rend": z, "bone_length": blp},
                                           seed=1)
            (c.sum() + m.sum() + d.sum()).backward()

        def singles():
            for k in range(K):
                pp, blp = model.transform_pose(pose[k:k + 1], bl[k:k + 1])
                c, m, d = render_posable(model, pixels, pp, K_inv, Nc=nc, Nf=nf,
                                         model_input={"z": None, "z_rend": z[k:k + 1], "bone_length": blp}, seed=1)
                (c.sum() + m.sum() + d.sum()).backward()

        ms = alternate({"render_scene_posable_fwd_bwd": scene, "K_render_posable_fwd_bwd": singles}, args.runs, max(1, args.batch // 4))
        emit({"what": "render", "K": K, "size": SIZE, "Nc": nc, "Nf": nf, "ms_per_call": ms,
              "launches": {"render_scene_posable_fwd_bwd": launches(scene), "K_render_posable_fwd_bwd": launches(singles)}})

        with torch.no_grad():
            mi = {"z": None, "z_rend": z, "bone_length": model.transform_pose(pose.detach(), bl)[1]}
            c, m, _ = render_scene(model, pixels, model.transform_pose(pose.detach(), bl)[0], K_inv, Nc=nc, Nf=nf, model_input=mi, seed=1)
        target, target_mask = (c + (m[:, None] - 1)).reshape(1, 3, SIZE, SIZE), (m > 0.5).float().reshape(1, SIZE, SIZE)
        steps = 5
        fit = lambda: fit_scene(model, target, target_mask, pose.detach(), bl, (None, z), K_inv, steps=steps, lr=1e-3, n_rays=1024,
                                Nc=nc, Nf=nf)
        fit()
        torch.cuda.synchronize()
        times = sorted(timed(fit) / steps for _ in range(args.runs))
        emit({"what": "fit", "K": K, "rays": 1024, "Nc": nc, "Nf": nf, "ms_per_step": round(times[len(times) // 2], 3),
              "steps_per_call": steps})
    log.close()


if __name__ == "__main__":
    main()
