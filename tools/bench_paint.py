#!/usr/bin/env python3
"""Coloured meshes (libenarf_paint.so) at the demo's output size (R = 512) on the synthetic scene of tools/bench_mesh.py.

For the meshes extract_mesh gives at voxel 0.01 (201^3) and 0.003 (667^3, the demo's), in the field's vertex colours:
  shade   ops.shade_fragments on the buffers of rasterize_mesh - one launch of paint_shade_kernel;
  torch   the same three outputs composed from torch calls on the same buffers (index gathers plus elementwise ops, fp64);
  raster  the rasterize_mesh call that precedes either;
each timed with device events over --batch back-to-back calls (a single shade is too short for the event clock), the
sides taking turns, the median of --runs rounds, and the kernel launches of one call of each. Then extract_mesh with
return_colors against the plain call (single calls, median of --runs): the difference is the colour query over V
vertices. Last, for the one sample of the scene, the mean absolute difference between the unlit field-coloured mesh
image and the volume render at the same camera and size, over the pixels both cover (mesh: a face; volume: mask > 0.5,
its colour divided by the mask): how well the surface colour stands in for the composited colour. One JSON line per
result, also appended to --log. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.mesh_rendering import extract_mesh, paint_mesh, rasterize_mesh  # noqa: E402
from enarf_gan_amd.libraries.NeRF.rendering import render_entire_img  # noqa: E402
from enarf_gan_amd.models.narf import TriPlaneNARF  # noqa: E402

SIZE, R, MESH_TH = 128, 512, 15.0


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


def torch_shade(f, verts, tris, colors):
    """shade_fragments(lit=True) from torch calls on the rasteriser's buffers, in fp64 as the kernel computes"""
    drawn = f.pix_to_face >= 0
    idx = tris[f.pix_to_face.clamp(min=0)]                                  # (R, R, 3)
    b = f.bary.double()[..., None]
    texel = (b * colors[idx].double()).sum(-2)
    q = (b * verts[idx].double()).sum(-2)
    n = f.normals.double()
    N = n / n.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    c = -(N * q).sum(-1) / q.norm(dim=-1).clamp(min=1e-6)
    spec = torch.where(c > 0, (2 * c * c - 1).clamp(min=0) ** 64, torch.zeros_like(c))
    shaded = texel * (0.5 + 0.3 * c.clamp(min=0))[..., None] + 0.2 * spec[..., None]
    texel = torch.where(drawn[..., None], texel, torch.ones_like(texel))
    shaded = torch.where(drawn[..., None], shaded, torch.ones_like(shaded))
    return (255 * shaded.clamp(0, 1)).floor().to(torch.uint8), texel.float(), shaded.float()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--voxels", default="0.01,0.003")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r12_paint.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paint.py measures on the GPU; none is available (nothing was measured)")

    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    sc = synth.make_scene(SIZE, 1, "center_fixed", 20)
    m = TriPlaneNARF(synth.nerf_config(origin_location="center_fixed"), 20, 24, parent=sc["parents"], num_bone_param=23)
    m.register_canonical_pose(sc["canonical_pose"])
    m.load_state_dict({f"mlp.{k}": v for k, v in sc["mlp"].items()}, strict=False)
    with torch.no_grad():
        m.tri_plane.copy_(sc["tri_plane"][:1])
    m = m.cuda().eval()
    pose, bl, z = sc["pose_to_camera"].cuda(), sc["bone_length"].cuda(), sc["z_rend"].cuda()
    K = sc["intrinsics"][:1].cuda()
    center, pose_parts, mi = m._mesh_inputs(pose, None, z, bl, 0.4)
    emit({"device": torch.cuda.get_device_name(0), "size": SIZE, "R": R, "runs": args.runs, "batch": args.batch})

    for voxel in (float(v) for v in args.voxels.split(",")):
        verts, tris, colors = extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi, return_colors=True)
        frag = rasterize_mesh(verts, tris, K, SIZE, R)
        shade = lambda: ops.shade_fragments(frag.pix_to_face, frag.bary, frag.normals, verts, tris, vertex_colors=colors)
        by_torch = lambda: torch_shade(frag, verts, tris, colors)
        raster = lambda: rasterize_mesh(verts, tris, K, SIZE, R)
        got, want = shade(), by_torch()
        level = int((got.image.int() - want[0].int()).abs().max())
        ms = alternate({"shade": shade, "torch": by_torch, "raster": raster}, args.runs, args.batch)
        emit({"voxel": voxel, "V": verts.shape[0], "T": tris.shape[0], "covered": int((frag.pix_to_face >= 0).sum()),
              "ms_per_call": ms, "launches": {"shade": launches(shade), "torch": launches(by_torch), "raster": launches(raster)},
              "shade_vs_torch_max_level": level,
              "shade_vs_torch_max_abs_shaded": float((got.shaded - want[2]).abs().max())})
        plain = lambda: extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)
        coloured = lambda: extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi, return_colors=True)
        ms = alternate({"extract_mesh": plain, "extract_mesh_with_colors": coloured}, args.runs, 1)
        emit({"voxel": voxel, "V": verts.shape[0], "ms_per_call": ms,
              "colour_query_ms": round(ms["extract_mesh_with_colors"] - ms["extract_mesh"], 4)})
        del frag, got, want

    # the surface colour against the composited colour, one sample, the scene's camera at the scene's size
    voxel = 0.003
    verts, tris, colors = extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi, return_colors=True)
    frag, painted = paint_mesh(verts, tris, K, SIZE, SIZE, vertex_colors=colors, lit=False)
    K_inv = torch.linalg.inv_ex(K[0].float()).inverse
    nc, nf = m.config.Nc, m.config.Nf
    vol, mask, _ = render_entire_img(m, pose_parts, K_inv, None, SIZE, nc, nf, model_input=mi)
    both = (frag.pix_to_face >= 0) & (mask > 0.5)
    surface = painted.albedo[both]                                            # (n, 3) in [0, 1]
    composited = ((vol / mask.clamp(min=1e-6) + 1) / 2).permute(1, 2, 0)[both]
    emit({"voxel": voxel, "size": SIZE, "Nc": nc, "Nf": nf, "mesh_pixels": int((frag.pix_to_face >= 0).sum()),
          "volume_pixels": int((mask > 0.5).sum()), "both": int(both.sum()),
          "mean_abs_difference_0_1": float((surface - composited).abs().mean()),
          "mean_abs_difference_levels": float((surface - composited).abs().mean() * 255)})
    log.close()


if __name__ == "__main__":
    main()
