#!/usr/bin/env python3
"""The pose gradient (libenarf_pgrad.so) on the fine samples of a C1 frame: 128^2 rays x 64 fine samples = 1 048 576
points of the synthetic scene, taken from one march's taps. Device events, one warm-up round, the median, minimum and
maximum of --runs rounds, the sides taking turns in one process (as tools/bench_skin.py).

  (a) ops.query_pose_bwd (two launches: pgrad_query_kernel, pgrad_finish_kernel) beside ops.query_fwd (mode f32, one
      launch) and the existing ops.query_bwd (tri-plane and MLP gradients) on the same points and upstream gradients. No
      other device implementation of the pose gradient exists to compare with.
  (b) one step of models.fit.fit_pose at --rays rays, Nc 48 / Nf 64: sampler, PoseCorrection, the march under no_grad,
      query_posable forward and backward, compositing, loss, Adam - the mean over --fit-steps steps of one call.
One JSON line per result, also appended to --log. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.models.fit import fit_pose  # noqa: E402
from enarf_gan_amd.models.narf import TriPlaneNARF  # noqa: E402

SIZE, NC, NF = 128, 48, 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(sides, runs):
    """{name: fn} -> {name: {median, min, max} ms}, the sides taking turns within each round"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            times[k].append(timed(fn))
    return {k: {"median": round(sorted(v)[len(v) // 2], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--fit-steps", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r17_pgrad.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pgrad.py measures on the GPU; none is available (nothing was measured)")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    sc = synth.make_scene(SIZE, 1, "center_fixed", 256)
    m = TriPlaneNARF(synth.nerf_config(Nc=NC, Nf=NF, origin_location="center_fixed", constant_triplane=True, mlp_mode="f32"),
                     256, 24, parent=sc["parents"], num_bone_param=23)
    m.register_canonical_pose(sc["canonical_pose"])
    m.load_state_dict({f"mlp.{k}": v for k, v in sc["mlp"].items()}, strict=False)
    with torch.no_grad():
        m.tri_plane.copy_(sc["tri_plane"][:1])
    m = m.cuda().eval()
    pose, bl, z_rend, inv_K = (sc[k].cuda() for k in ("pose_to_camera", "bone_length", "z_rend", "inv_intrinsics"))
    emit({"device": torch.cuda.get_device_name(0), "size": SIZE, "Nc": NC, "Nf": NF, "runs": args.runs})

    # ---- (a) the three query kernels on the fine samples of one frame
    with torch.no_grad():
        _, _, (pts, _) = m(1, sc["image_coord"].cuda(), pose, inv_K, None, z_rend, bl, Nc=NC, Nf=NF, return_intermediate=True, seed=1)
    pts = pts.contiguous()
    N = pts.shape[-1]
    parts, pack = ops.prepare(pose, bl, m.canonical_bone_length, z_rend, m.mlp.as_dict(), m.parent_id, m.origin_location,
                              m.coordinate_scale)
    tri = m.tri_plane.detach()
    feat_cl = ops.triplane_pack(tri)
    g = torch.Generator(device="cuda").manual_seed(0)
    gd, gc = torch.randn(1, N, device="cuda", generator=g), torch.randn(1, 3, N, device="cuda", generator=g)
    a = (pts, parts, m.canonical_pose, tri, feat_cl, pack)
    ms = alternate({"query_pose_bwd": lambda: ops.query_pose_bwd(*a, gd, gc),
                    "query_fwd_f32": lambda: ops.query_fwd(*a, mlp_mode="f32"),
                    "query_bwd": lambda: ops.query_bwd(*a, gd, gc)}, args.runs)
    _, _, vb = ops.query_fwd(*a, mlp_mode="f32", need_valid=True)
    emit({"a": "query kernels on the fine samples of a C1 frame", "points": N, "points_in_a_cube": int((vb != 0).sum()),
          "ms": ms, "launches": {"query_pose_bwd": 2, "query_fwd_f32": 1},
          "ns_per_point_query_pose_bwd": round(ms["query_pose_bwd"]["median"] * 1e6 / N, 3)})

    # ---- (b) one fit_pose step
    with torch.no_grad():
        c, al, _ = m.render_entire_img(pose, inv_K, None, z_rend, bl, render_size=SIZE, Nc=NC, Nf=NF)
    target, tmask = (c - (1 - al))[None], al[None]
    step = lambda: fit_pose(m, target, tmask, pose, bl, (None, z_rend), inv_K, steps=args.fit_steps, lr=1e-3,  # noqa: E731
                            n_rays=args.rays, Nc=NC, Nf=NF)
    ms = alternate({"fit_pose": step}, max(3, args.runs // 3))["fit_pose"]
    emit({"b": "fit_pose", "rays": args.rays, "steps_per_call": args.fit_steps,
          "ms_per_step": {k: round(v / args.fit_steps, 4) for k, v in ms.items()}})
    log.close()


if __name__ == "__main__":
    main()
