#!/usr/bin/env python3
"""Multi-avatar scenes (libenarf_scene.so), measured on the device.

  composite  ops.scene_composite (one launch of scene_composite_kernel, the six default outputs) at K = 2 and K = 4
             avatars, Nf 64, 128 x 128 rays, on seeded interleaved sample lists, against the same composition written in
             torch in fp32 (cummax, a stable sort of the K Nf breakpoints, a cumsum and a gather per avatar, a cumsum of
             the optical depth): time, kernel launches of one call of each, and the largest difference between the two;
  render     rendering.render_scene with K avatars on the synthetic scene of tools/bench_geom.py at 128 x 128 (Nc 48, Nf
             64) beside K forward calls of one avatar, one forward call of a batch of K, and the same batch marched with
             its taps (debug=True), which is what render_scene pays for the samples it composes;
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

from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NeRF.rendering import render_scene  # noqa: E402
from enarf_gan_amd.models.narf import TriPlaneNARF  # noqa: E402

SIZE, NF = 128, 64


def timed(fn, batch=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name
                   and "emset" not in e.name)
    except Exception as e:      # noqa: BLE001 - the count is a side figure; the times stand without it
        print(f"kernel count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def alternate(sides, runs, batch):
    """{name: fn} -> {name: median ms per call}, the sides taking turns within each round"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            times[k].append(timed(fn, batch))
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}


def samples(K, n, Nf, dev, seed=0):
    """(depth, density (1, K, n, Nf), color (1, K, 3, n, Nf), valid (1, K, n)): overlapping depth ranges, a fifth of the
    samples empty, a tenth of the (avatar, ray) pairs invalid"""
    g = torch.Generator(device=dev).manual_seed(seed)
    near = 2.0 + 0.5 * torch.rand(1, K, n, 1, device=dev, generator=g)
    depth = near + torch.rand(1, K, n, Nf, device=dev, generator=g).sort(-1).values * (0.5 + torch.rand(1, K, n, 1, device=dev, generator=g))
    density = torch.exp(6 * torch.rand(1, K, n, Nf, device=dev, generator=g) - 3) * (torch.rand(1, K, n, Nf, device=dev, generator=g) > 0.2)
    color = 2 * torch.rand(1, K, 3, n, Nf, device=dev, generator=g) - 1
    valid = (torch.rand(1, K, n, device=dev, generator=g) > 0.1).to(torch.uint8)
    return depth.contiguous(), density.contiguous(), color.contiguous(), valid


def torch_composite(depth, density, color, valid, render_scale=1.0, threshold=0.5):
    """the contract of include/enarf_scene.h from torch calls in fp32, for inputs that pass the screening: (color (F, 3, n),
    mask, disparity (F, n), instance_mass (F, K, n), instance (F, n))"""
    F, K, n, Nf = depth.shape
    live = valid.bool()[..., None]                                               # (F, K, n, 1)
    D = torch.where(live, depth.cummax(-1).values, torch.full_like(depth, float("inf")))
    keys = D.permute(0, 2, 1, 3).reshape(F, n, K * Nf)                           # flat index k Nf + i breaks ties, as the key does
    t, order = keys.sort(dim=-1, stable=True)
    who = torch.div(order, Nf, rounding_mode="floor")
    finite = torch.isfinite(t)
    step = torch.where(finite[..., 1:] & finite[..., :-1], t[..., 1:] - t[..., :-1], torch.zeros_like(t[..., 1:]))
    sigma, mixed, dens = torch.zeros_like(t), torch.zeros(F, 3, n, K * Nf, device=t.device), []
    for k in range(K):
        active = (who == k).cumsum(-1) - 1
        has = (active >= 0) & (active <= Nf - 2) & valid[:, k].bool()[..., None]
        idx = active.clamp(0, Nf - 2)
        s = torch.where(has, density[:, k].gather(-1, idx), torch.zeros_like(t))
        c = color[:, k].gather(-1, idx[:, None].expand(-1, 3, -1, -1))
        sigma, mixed = sigma + s, mixed + s[:, None] * c
        dens.append(s)
    tau = torch.zeros_like(t)
    tau[..., :-1] = sigma[..., :-1] * step * render_scale
    w = torch.exp(-(tau.cumsum(-1) - tau)) * -torch.expm1(-tau)
    share = torch.where(sigma > 0, w / sigma.clamp(min=1e-38), torch.zeros_like(w))
    mask = w.sum(-1)
    mass = torch.stack([(share * s).sum(-1) for s in dens], dim=1)
    instance = torch.where(mask >= threshold, mass.argmax(1), torch.full_like(mass[:, 0], -1, dtype=torch.long)).int()
    disparity = torch.where(finite, w / t, torch.zeros_like(w)).sum(-1)
    return (share[:, None] * mixed).sum(-1), mask, disparity, mass, instance


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r18_scene.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene.py measures on the GPU; none is available (nothing was measured)")
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    emit({"device": torch.cuda.get_device_name(0), "runs": args.runs, "batch": args.batch})

    # ---- the composite kernel against torch
    n = SIZE * SIZE
    for K in (2, 4):
        depth, density, color, valid = samples(K, n, NF, dev)
        kernel = lambda: ops.scene_composite(depth, density, color, valid)
        by_torch = lambda: torch_composite(depth, density, color, valid)
        got, want = kernel(), by_torch()
        ms = alternate({"scene_composite": kernel, "torch": by_torch}, args.runs, args.batch)
        mb = (K * n * NF * 5 * 4 + K * n + n * (3 + 1 + 1 + K + 1 + 1) * 4) / 1e6
        emit({"what": "composite", "K": K, "Nf": NF, "rays": n, "ms_per_call": ms, "batch": args.batch,
              "launches": {"scene_composite": launches(kernel), "torch": launches(by_torch)},
              "compulsory_MB": round(mb, 2), "GB_per_s": round(mb / ms["scene_composite"], 1),
              "max_abs_colour_difference": float((got.color - want[0]).abs().max()),
              "max_abs_mask_difference": float((got.mask - want[1]).abs().max()),
              "max_abs_disparity_difference": float((got.disparity - want[2]).abs().max()),
              "max_abs_instance_mass_difference": float((got.instance_mass - want[3]).abs().max()),
              "instances_differ": int((got.instance != want[4]).sum()), "skipped_rays": int((got.skipped != 0).sum())})
        del got, want

    # ---- render_scene beside forward calls, on the synthetic scene
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
        parts, pack = ops.prepare(pose, bl, model.canonical_bone_length, z, model.mlp.as_dict(), model.parent_id,
                                  model.origin_location, model.coordinate_scale)
        tri, feat_cl = model._tri_plane_pair({"z": None, "bone_length": bl})
        mi = {"z": None, "z_rend": z, "bone_length": bl}
        stand_in = pose.new_empty(K, model.num_bone, 4, 4)
        coord, Ki = pixels.expand(K, -1, -1, -1), K_inv.expand(K, -1, -1)
        with torch.no_grad():
            scene = lambda: render_scene(model, pixels, stand_in, K_inv, Nc=nc, Nf=nf, model_input=mi, seed=1, _parts=parts, _pack=pack)
            singles = lambda: [ops.render_fwd(pixels, K_inv, parts[k:k + 1], model.canonical_pose, tri, feat_cl, pack[k:k + 1], nc,
                                              nf, seed=1, mlp_mode=model.mlp_mode, **model.kernel_flags()) for k in range(K)]
            batched = lambda: ops.render_fwd(coord, Ki, parts, model.canonical_pose, tri, feat_cl, pack, nc, nf, seed=1,
                                             mlp_mode=model.mlp_mode, **model.kernel_flags())
            tapped = lambda: ops.render_fwd(coord, Ki, parts, model.canonical_pose, tri, feat_cl, pack, nc, nf, seed=1,
                                            mlp_mode=model.mlp_mode, debug=True, **model.kernel_flags())
            ms = alternate({"render_scene": scene, "K_forward_marches": singles, "one_march_of_K": batched,
                            "one_march_of_K_with_taps": tapped}, args.runs, args.batch)
            _, mask, _ = scene()
            inst = model.buffers_tensors["instance"]
            emit({"what": "render", "K": K, "size": SIZE, "Nc": nc, "Nf": nf, "ms_per_call": ms,
                  "taps_cost_ms": round(ms["one_march_of_K_with_taps"] - ms["one_march_of_K"], 4),
                  "composite_and_glue_ms": round(ms["render_scene"] - ms["one_march_of_K_with_taps"], 4),
                  "launches": {"render_scene": launches(scene), "K_forward_marches": launches(singles)},
                  "pixels_of_each_avatar": [int((inst == k).sum()) for k in range(K)], "mask_mean": float(mask.mean()),
                  "skipped_rays": int((model.buffers_tensors["skipped"] != 0).sum())})
    log.close()


if __name__ == "__main__":
    main()
