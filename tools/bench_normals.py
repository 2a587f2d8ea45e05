#!/usr/bin/env python3
"""Field normals (libenarf_nrm.so) on a C1 frame of the synthetic scene: 128^2 rays, Nc 48 / Nf 64, so 1 048 576 fine
samples, taken from one march's taps. Device events, one warm-up round, the median, minimum and maximum of --runs
rounds, the sides taking turns in one process (as tools/bench_pgrad.py).

  (a) ops.field_gradient (one launch: nrm_gradient_kernel) beside ops.query_pose_bwd with g_density = 1 and g_color = None
      (two launches, the same gradient) and ops.query_fwd (mode f32, one launch) on the same points; the largest
      difference between the two gradients is reported with them, and the number of points that differ by more than
      1e-5 of the largest gradient (the two kernels round their fp32 sums differently, and a point with one of its 132
      pre-activations within a rounding of zero lands on the other slope of the activation in one of them).
  (b) ops.ray_normals (one launch: nrm_ray_kernel) beside ops.geometry_buffers on the same frame.
  (c) TriPlaneNARF.render_geometry with normals="field" and without, beside forward, at 128^2.
  (d) agreement, reported and not asserted: the median angle between the field normals and the stencil normals of
      geometry_buffers where a ray has both, and between the field normals and the rasteriser's face normals on the
      covered pixels of the scene's mesh (paint_mesh's per-pixel buffer).
One JSON line per result, also appended to --log. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.mesh_rendering import pixel_field_normals, rasterize_mesh  # noqa: E402
from enarf_gan_amd.libraries.NeRF.rendering import _march_with_gradient  # noqa: E402
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


def median_angle(a, b):
    """median angle in degrees between two sets of vectors (n, 3), each normalised first"""
    a, b = torch.nn.functional.normalize(a.double(), dim=-1), torch.nn.functional.normalize(b.double(), dim=-1)
    return float(torch.rad2deg(torch.acos((a * b).sum(-1).clamp(-1, 1))).median()) if len(a) else float("nan")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--voxel-size", type=float, default=0.01, help="(d): the density sweep's voxel of the mesh")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r22_normals.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals.py measures on the GPU; none is available (nothing was measured)")
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
    coord = sc["image_coord"].cuda()
    emit({"device": torch.cuda.get_device_name(0), "size": SIZE, "Nc": NC, "Nf": NF, "runs": args.runs})

    # ---- (a) the gradient kernel on the fine samples of one frame
    parts, pack = ops.prepare(pose, bl, m.canonical_bone_length, z_rend, m.mlp.as_dict(), m.parent_id, m.origin_location,
                              m.coordinate_scale)
    mi = {"z": None, "z_rend": z_rend, "bone_length": bl, "truncation_psi": 1}
    out, gradient = _march_with_gradient(m, coord, inv_K, parts, pack, NC, NF, 1, mi, None, 1)
    pts = m.buffers_tensors["fine_points"].contiguous()
    N = pts.shape[-1]
    tri = m.tri_plane.detach()
    feat_cl = ops.triplane_pack(tri)
    ones = torch.ones(1, N, device="cuda")
    a = (pts, parts, m.canonical_pose, tri, feat_cl, pack)
    ms = alternate({"field_gradient": lambda: ops.field_gradient(*a),
                    "query_pose_bwd_gd1": lambda: ops.query_pose_bwd(*a, ones, None),
                    "query_fwd_f32": lambda: ops.query_fwd(*a, mlp_mode="f32")}, args.runs)
    den, grad = ops.field_gradient(*a)
    g_points, _ = ops.query_pose_bwd(*a, ones, None)
    fwd, _, vb = ops.query_fwd(*a, mlp_mode="f32", need_valid=True)
    emit({"a": "gradient kernels on the fine samples of a C1 frame", "points": N, "points_in_a_cube": int((vb != 0).sum()),
          "points_with_a_gradient": int((grad != 0).any(dim=1).sum()), "ms": ms,
          "launches": {"field_gradient": 1, "query_pose_bwd_gd1": 2, "query_fwd_f32": 1},
          "ns_per_point_field_gradient": round(ms["field_gradient"]["median"] * 1e6 / N, 3),
          "max_abs_gradient": float(grad.abs().max()), "max_abs_diff_to_query_pose_bwd": float((grad - g_points).abs().max()),
          "points_off_query_pose_bwd_by_1e-5_of_max": int(((grad - g_points).abs().amax(dim=1) > 1e-5 * grad.abs().max()).sum()),
          "max_abs_density_diff_to_query_fwd": float((den - fwd[:, 0]).abs().max()), "max_density": float(fwd.max())})

    # ---- (b) the ray kernel beside geometry_buffers
    disparity = out.disparity * m.coordinate_scale
    geo = ops.geometry_buffers(disparity, out.mask, inv_K, size=(SIZE, SIZE), shade="lit")
    mask2 = out.mask.reshape(1, SIZE, SIZE)
    ray = lambda: ops.ray_normals(gradient, out.fine_weights, mask2, fallback=geo.normals, flags=geo.flags,  # noqa: E731
                                  points=geo.points, shade="lit")
    ms = alternate({"ray_normals": ray,
                    "geometry_buffers": lambda: ops.geometry_buffers(disparity, out.mask, inv_K, size=(SIZE, SIZE), shade="lit")},
                   args.runs)
    emit({"b": "per-frame kernels at 128^2", "rays": SIZE * SIZE, "Nf": NF, "ms": ms,
          "launches": {"ray_normals": 1, "geometry_buffers": 1}})

    # ---- (c) the model's entry point
    geom = lambda **kw: m.render_geometry(pose, inv_K, None, z_rend, bl, SIZE, Nc=NC, Nf=NF, shade="lit", **kw)  # noqa: E731
    with torch.no_grad():
        ms = alternate({"render_geometry_field": lambda: geom(normals="field"), "render_geometry": lambda: geom(),
                        "forward": lambda: m(1, coord, pose, inv_K, None, z_rend, bl, Nc=NC, Nf=NF)}, args.runs)
    emit({"c": "render_geometry at 128^2", "ms": ms,
          "launches_added_by_field": {"field_gradient": 1, "ray_normals": 1, "march": "with its taps"}})

    # ---- (d) agreement with the stencil normals and with the mesh's face normals
    field = ray()
    both = ((field.flags & 4) > 0) & ((geo.flags & 2) > 0)
    row = {"d": "median angles, degrees", "rays_with_both_normals": int(both.sum()), "rays_with_a_field_normal": int(((field.flags & 4) > 0).sum()),
           "valid_rays": int(((geo.flags & 1) > 0).sum()), "field_vs_stencil": round(median_angle(field.normals[both], geo.normals[both]), 3)}
    th = float(m.density_volume(pose, None, z_rend, bl, voxel_size=args.voxel_size).max()) * 0.4
    v, t = m.extract_mesh(pose, None, z_rend, bl, voxel_size=args.voxel_size, mesh_th=th)
    frag = rasterize_mesh(v, t, sc["intrinsics"].cuda(), SIZE)
    buf = pixel_field_normals(frag, v, t, m.mesh_field(pose, None, z_rend, bl))
    covered = frag.pix_to_face >= 0
    differs = covered & (buf != frag.normals).any(dim=-1)
    row.update(mesh_triangles=len(t), covered_pixels=int(covered.sum()), covered_pixels_with_a_field_normal=int(differs.sum()),
               field_vs_mesh=round(median_angle(buf[differs], frag.normals[differs]), 3))
    emit(row)
    log.close()


if __name__ == "__main__":
    main()
