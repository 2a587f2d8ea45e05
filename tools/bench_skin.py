#!/usr/bin/env python3
"""Rigged meshes (libenarf_skin.so) on the synthetic scene of tools/bench_mesh.py, the mesh of the demo's voxel (0.003: a
667^3 lattice) unless --voxel says otherwise. Device events, one warm-up round, the median of --runs rounds, the sides of
a comparison taking turns in one process (as tools/bench_seg.py).

  (a) skin weights: the ops.skin_weights launch over the vertex array (K = 4 and 8) beside extract_mesh.
  (b) posing --frames frames: one ops.skin_pose launch, against the same arithmetic composed in torch (a gather of
      (F, P, 3, 4) matrices and an einsum, fp64, in chunks of 8 frames) and against one extract_mesh per frame, the only
      way to a mesh in a new pose without the rig; achieved bytes per second against the compulsory traffic (12 B out a
      vertex a frame, 12 + 8 K B in a vertex a group of 8 frames).
  (c) the whole animation: gen.render_mesh_animation at 512^2 against gen.render_mesh_turntable over as many angles
      (the same rasteriser and shading per frame; the difference is posing against turning).
  (d) how good the rig is: at interpolated poses between two random key poses, the posed mesh against a mesh extracted
      again at that pose, both through rasterize_mesh at --quality-size: silhouette IoU and the median relative z-buffer
      difference over the pixels both cover, at K = 4 and 8, on the mesh of --quality-voxel; and the distribution of
      kept_mass. Recorded, not gated.
One JSON line per result, also appended to --log. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.mesh_rendering import rasterize_mesh, skin_mesh  # noqa: E402
from enarf_gan_amd.libraries.NeRF.rendering import _parts_from_part_poses  # noqa: E402
from enarf_gan_amd.models.generator import TriNARFGenerator  # noqa: E402

SIZE, R, MESH_TH, GROUP = 128, 512, 15.0, 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(sides, runs):
    """{name: fn} -> {name: median ms}, the sides taking turns within each round"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            times[k].append(timed(fn))
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}


def torch_pose(v, joints, weights, rest, parts, cs, out):
    """ops.skin_pose composed in torch, fp64: per-part (F, P, 3, 4) matrices, a gather per slot, one einsum"""
    A, B = rest[0].double(), parts.double()
    rho = A[None, :, 12] / B[:, :, 12]
    L = rho[..., None, None] * (B[:, :, :9].reshape(B.shape[0], -1, 3, 3) @ A[:, :9].reshape(-1, 3, 3).transpose(-1, -2))
    t = B[:, :, 9:12] / cs - (L @ (A[:, 9:12] / cs)[None, :, :, None])[..., 0]
    M = torch.cat([L, t[..., None]], dim=-1)                                # (F, P, 3, 4)
    vh = torch.cat([v.double(), torch.ones_like(v[:, :1], dtype=torch.float64)], dim=1)
    w = torch.where(joints >= 0, weights, torch.zeros_like(weights)).double()
    idx = joints.clamp(min=0).long()
    for a in range(0, M.shape[0], GROUP):
        blend = torch.einsum("vk,fvkij->fvij", w, M[a:a + GROUP][:, idx])   # (f, V, 3, 4)
        out[a:a + GROUP] = torch.einsum("fvij,vj->fvi", blend, vh).float()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--voxel", type=float, default=0.003)
    ap.add_argument("--quality-voxel", type=float, default=0.01)
    ap.add_argument("--quality-size", type=int, default=256)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r15_skin.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skin.py measures on the GPU; none is available (nothing was measured)")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    sc = synth.make_scene(SIZE, 2, "center_fixed", 256)
    cfg = synth.AttrDict(z_dim=256, background_ratio=0.7, crop_background=True, pretrained_background=False,
                         nerf_params=synth.nerf_config(origin_location="center_fixed", constant_triplane=False))
    gen = TriNARFGenerator(cfg, SIZE, 24, sc["parents"], 23, black_background=True)
    gen.register_canonical_pose(sc["canonical_pose"])
    gen.nerf.load_state_dict({f"mlp.{k}": v for k, v in sc["mlp"].items()}, strict=False)
    gen = gen.cuda().eval()
    tri = sc["tri_plane"][:1].cuda()
    gen.nerf.tri_plane_gen = lambda z_, enc, truncation_psi=1: tri.repeat(z_.shape[0], 1, 1, 1)
    nerf, cs = gen.nerf, float(gen.nerf.coordinate_scale)
    z = torch.cat([torch.randn(1, 512, generator=torch.Generator().manual_seed(0)), sc["z_rend"][:1]], dim=1).cuda()
    keys = sc["pose_to_camera"][:2].double().cuda()                        # two random poses of the synthetic skeleton
    pose, bl, K = keys[:1].float(), sc["bone_length"][:1].cuda(), sc["intrinsics"][:1].cuda()
    F = args.frames
    emit({"device": torch.cuda.get_device_name(0), "size": SIZE, "R": R, "runs": args.runs, "frames": F, "voxel": args.voxel})

    # ---- (a) the skin-weight launch beside extract_mesh
    mesh = dict(voxel_size=args.voxel, mesh_th=MESH_TH)
    rigs = {k: gen.extract_rigged_mesh(pose, z, bl, **mesh, max_influences=k, return_colors=True) for k in (4, 8)}
    rig = rigs[4]
    V, T = rig.vertices.shape[0], rig.triangles.shape[0]
    rest = _parts_from_part_poses(nerf, rig.rest_pose, rig.rest_bone_length)
    mask_tri = nerf.compute_tri_plane_feature(gen._latent_parts(z)[0], bl, 0.4)
    flags = nerf.kernel_flags()
    weigh = {f"skin_weights_k{k}": (lambda k=k: ops.skin_weights(rig.vertices, rest, nerf.canonical_pose, mask_tri, max_influences=k,
                                                                 clamp_mask=flags["clamp_mask"],
                                                                 uniform_part_weight=flags["uniform_part_weight"], coordinate_scale=cs))
             for k in (4, 8)}
    ms = alternate({**weigh, "extract_mesh": lambda: gen.extract_mesh(pose, z, bl, **mesh)}, args.runs)
    emit({"a": "skin weights", "V": V, "T": T, "ms": ms})

    # ---- (b) posing F frames
    poses32 = ops.interpolate_pose(keys, nerf.parent_id, F, True, return_f32=True)[1]
    pose_parts, bl_parts = nerf.transform_pose(poses32, bl.expand(F, -1, -1))
    parts = _parts_from_part_poses(nerf, pose_parts, bl_parts)
    out = torch.empty(F, V, 3, device="cuda")
    ref = torch.empty(F, V, 3, device="cuda")
    sides = {f"skin_pose_k{k}": (lambda k=k: ops.skin_pose(rigs[k].vertices, rigs[k].joints, rigs[k].weights, rest, parts,
                                                           coordinate_scale=cs, out=out)) for k in (4, 8)}
    sides["torch_k4"] = lambda: torch_pose(rig.vertices, rig.joints, rig.weights, rest, parts, cs, ref)
    ms = alternate(sides, args.runs)
    ops.skin_pose(rig.vertices, rig.joints, rig.weights, rest, parts, coordinate_scale=cs, out=out)
    agree = float((out - ref).abs().max())
    groups = (F + GROUP - 1) // GROUP
    traffic = {k: 12 * V * F + (12 + 8 * k) * V * groups for k in (4, 8)}
    emit({"b": "posing", "V": V, "frames": F, "ms": ms, "skin_vs_torch_max_abs": agree, "compulsory_bytes": traffic,
          "achieved_GB_per_s": {k: round(traffic[k] / ms[f"skin_pose_k{k}"] / 1e6, 1) for k in (4, 8)}})
    one = alternate({"extract_mesh_per_frame": lambda: gen.extract_mesh(poses32[F // 2:F // 2 + 1], z, bl, **mesh)}, args.runs)
    emit({"b": "re-extraction", "ms_per_frame": one["extract_mesh_per_frame"],
          "ms_for_all_frames": round(one["extract_mesh_per_frame"] * F, 2), "skin_pose_k4_ms_for_all_frames": ms["skin_pose_k4"]})
    del out, ref

    # ---- (d) the posed mesh against a mesh extracted again at the pose
    Rq = args.quality_size
    qmesh = dict(voxel_size=args.quality_voxel, mesh_th=MESH_TH)
    qposes = ops.interpolate_pose(keys, nerf.parent_id, 8, False, return_f32=True)[1][[2, 4, 7]]
    qparts, qbl = nerf.transform_pose(qposes, bl.expand(3, -1, -1))
    for k in (4, 8):
        qrig = gen.extract_rigged_mesh(pose, z, bl, **qmesh, max_influences=k)
        posed = skin_mesh(nerf, qrig, qparts, qbl)
        rows = []
        for i in range(3):
            a = rasterize_mesh(posed[i], qrig.triangles, K, SIZE, Rq)
            v2, t2 = gen.extract_mesh(qposes[i:i + 1], z, bl, **qmesh)
            b = rasterize_mesh(v2, t2, K, SIZE, Rq)
            ca, cb = a.pix_to_face >= 0, b.pix_to_face >= 0
            both = ca & cb
            rel = ((a.zbuf - b.zbuf).abs() / b.zbuf.abs().clamp(min=1e-6))[both]
            rows.append({"silhouette_iou": round(float(both.sum() / (ca | cb).sum().clamp(min=1)), 4),
                         "median_rel_zbuf_diff": float(rel.median()) if rel.numel() else None,
                         "p90_rel_zbuf_diff": float(rel.quantile(0.9)) if rel.numel() else None})
        many = qrig.kept_mass[(qrig.kept_mass > 0) & (qrig.kept_mass < 1)]
        emit({"d": "rig quality", "K": k, "V": qrig.vertices.shape[0], "voxel": args.quality_voxel, "poses": rows,
              "kept_mass": {"mean": float(qrig.kept_mass.mean()), "unowned": int((qrig.kept_mass == 0).sum()),
                            "more_than_K_valid": int(many.numel()),
                            "mean_there": float(many.mean()) if many.numel() else None,
                            "p10_there": float(many.quantile(0.1)) if many.numel() else None}})

    # ---- (c) the whole animation at R x R
    angles = torch.arange(F, dtype=torch.float32, device="cuda") * (6.283185307179586 / F)
    ms = alternate({"render_mesh_animation": lambda: gen.render_mesh_animation(rig, keys, bl, K, num=F, render_size=R),
                    "render_mesh_turntable": lambda: gen.render_mesh_turntable(pose, K, z, bl, angles, **mesh, render_size=R)},
                   max(1, args.runs // 2 + 1))
    emit({"c": "animation", "frames": F, "R": R, "V": V, "ms": ms,
          "ms_per_frame": {k: round(v / F, 4) for k, v in ms.items()}})
    log.close()


if __name__ == "__main__":
    main()
