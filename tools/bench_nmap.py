#!/usr/bin/env python3
"""Tangent-space normal maps (libenarf_nmap.so) on the synthetic scene of tools/bench_bake.py, for the meshes extract_mesh
gives at voxel 0.02 and 0.05 and atlases of 1024, 2048 and 4096 texels a side (a size the layout cannot fit the mesh into is
reported and left out):
  encode   ops.encode_normal_map on random vectors - one launch of nmap_encode_kernel - against the same map composed from
           torch calls (gathers, the frame and the projection in fp64);
  shade    ops.shade_normal_mapped at R = 512 on the buffers of rasterize_mesh with the RGBA8 map and the RGBA8 texture - one
           launch of nmap_shade_kernel - against torch calls (bench_bake's torch_shade with the normal tapped by grid_sample);
each timed with device events over --batch back-to-back calls after one warm-up round, the sides taking turns, the median of
--runs rounds with the spread (min, max), the kernel launches of one call of each, and the achieved bytes a second against
the compulsory traffic (encode: 20 bytes a texel and the mesh once; shade: 71 bytes a pixel and 32 a covered pixel).
Then, single calls, median of --runs:
  bake     bake_normal_map end to end beside bake_texture and extract_mesh;
  frame    a 512^2 frame of the textured animation (skin_pose, rasterize_mesh, shade) with and without the map;
  still    paint_normal_mapped_mesh against paint_textured_mesh(normals="field"), the per-frame field query the map replaces.
Last, on the mesh of the finest voxel simplified to cells of 2, 4 and 8 voxels: the mean angle, in the rest pose, between the
shading normal and field_normals at the covered pixels' surface points - for the face normals, the 8-bit map and the fp32
map. One JSON line per result, also appended to --log. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_bake import MESH_TH, R, SIZE, _corner_table, alternate, launches  # noqa: E402
from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.mesh_rendering import (bake_normal_map, bake_texture, extract_mesh,  # noqa: E402
                                                         extract_rigged_mesh, field_normals, paint_normal_mapped_mesh,
                                                         paint_textured_mesh, rasterize_mesh, skin_mesh)
from enarf_gan_amd.models.narf import TriPlaneNARF  # noqa: E402


def torch_frames(verts, tris):
    """(t^, b^, n^) of every triangle from torch calls, fp64"""
    p = verts.double()[tris]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = F.normalize(torch.linalg.cross(e1, e2), dim=-1)
    s = 1.0 - 2.0 * (torch.arange(tris.shape[0], device=verts.device) % 2).double()
    t = F.normalize(e1, dim=-1) * s[:, None]
    return t, torch.linalg.cross(t, n), n


def torch_encode(face, vectors, verts, tris):
    own = (face >= 0).reshape(-1)
    k = face.reshape(-1).clamp(min=0).long()
    t, b, n = torch_frames(verts, tris)
    g = -vectors.double().t()
    m = g.norm(dim=-1, keepdim=True)
    q = torch.stack([(g * t[k]).sum(-1), (g * b[k]).sum(-1), (g * n[k]).sum(-1)], -1) / m.clamp(min=1e-300)
    flat = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=face.device)
    q = torch.where((own & (m[:, 0] > 0) & torch.isfinite(m[:, 0]))[:, None], q, flat)
    rgb = (255 * ((q + 1) / 2).clamp(0, 1) + 0.5).floor().to(torch.uint8)
    return torch.cat([rgb, torch.where(own, 255, 0).to(torch.uint8)[:, None]], 1).reshape(face.shape + (4,))


def torch_shade(f, verts, tris, nmap, texture, lay):
    """shade_normal_mapped(lit=True) with RGBA8 textures from torch calls on the rasteriser's buffers"""
    c, n, _ = lay
    A = texture.shape[0]
    drawn = f.pix_to_face >= 0
    face = f.pix_to_face.clamp(min=0)
    idx = tris[face]
    q, h = face // 2, face % 2
    origin = torch.stack([(q % n) * c, (q // n) * c], -1).double()
    U = origin[..., None, :] + _corner_table(c, verts.device)[h]
    b = f.bary.double()[..., None]
    grid = ((b * U).sum(-2) / A * 2 - 1).float()[None]
    both = torch.cat([texture[..., :3].float() / 255, nmap[..., :3].float() * (2 / 255) - 1], -1).permute(2, 0, 1)[None]
    tap = F.grid_sample(both, grid, mode="bilinear", padding_mode="border", align_corners=False)[0].permute(1, 2, 0).double()
    texel, m = tap[..., :3], tap[..., 3:]
    t, bt, nr = torch_frames(verts, tris)
    ns = F.normalize(m[..., :1] * t[face] + m[..., 1:2] * bt[face] + m[..., 2:] * nr[face], dim=-1)
    p = (b * verts[idx].double()).sum(-2)
    cosine = -(ns * p).sum(-1) / p.norm(dim=-1).clamp(min=1e-6)
    spec = torch.where(cosine > 0, (2 * cosine * cosine - 1).clamp(min=0) ** 64, torch.zeros_like(cosine))
    shaded = texel * (0.5 + 0.3 * cosine.clamp(min=0))[..., None] + 0.2 * spec[..., None]
    shaded = torch.where(drawn[..., None], shaded, torch.ones_like(shaded))
    return (255 * shaded.clamp(0, 1)).floor().to(torch.uint8), ns.float(), shaded.float()


def kernels(m, pose_parts, mi, verts, tris, frag, voxel, sizes, args, emit):
    fit = []
    covered = int((frag.pix_to_face >= 0).sum())
    for A in sizes:
        try:
            lay = ops.bake_layout(tris.shape[0], A)
        except NotImplementedError as e:
            emit({"voxel": voxel, "atlas": A, "unsupported": str(e)})
            continue
        fit.append(A)
        atlas = bake_texture(m, pose_parts, verts, tris, mi, size=A)
        nmap = bake_normal_map(m, pose_parts, verts, tris, mi, size=A)
        baked = ops.bake_points(verts, tris, A)
        vectors = torch.randn(3, A * A, device="cuda")
        sides = {"encode": lambda: ops.encode_normal_map(baked.texel_face, vectors, verts, tris),
                 "encode_torch": lambda: torch_encode(baked.texel_face, vectors, verts, tris),
                 "shade": lambda: ops.shade_normal_mapped(frag.pix_to_face, frag.bary, frag.normals, verts, tris, nmap.texture,
                                                          texture=atlas.texture),
                 "shade_torch": lambda: torch_shade(frag, verts, tris, nmap.texture, atlas.texture, lay)}
        got, want = sides["shade"](), sides["shade_torch"]()
        enc, enc_t = sides["encode"]().texture, sides["encode_torch"]()
        ms = alternate(sides, args.runs, args.batch)
        bytes_encode = 20 * A * A + 24 * tris.shape[0] + 12 * verts.shape[0]
        bytes_shade = 71 * R * R + 32 * covered
        emit({"voxel": voxel, "atlas": A, "cell": lay.cell, "ms_per_call": ms, "launches": {k: launches(fn) for k, fn in sides.items()},
              "compulsory_bytes": {"encode": bytes_encode, "shade": bytes_shade},
              "GBps": {"encode": round(bytes_encode / ms["encode"][0] / 1e6, 1), "shade": round(bytes_shade / ms["shade"][0] / 1e6, 1)},
              "encode_vs_torch_max_level": int((enc.int() - enc_t.int()).abs().max()),
              "shade_vs_torch_max_level": int((got.image.int() - want[0].int()).abs().max())})
        del atlas, nmap, baked, vectors, got, want, enc, enc_t
    return fit


def end_to_end(m, pose, bl, K, center, pose_parts, mi, verts, tris, voxel, A, args, emit):
    sides = {"extract_mesh": lambda: extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi),
             "bake_texture": lambda: bake_texture(m, pose_parts, verts, tris, mi, size=A),
             "bake_normal_map": lambda: bake_normal_map(m, pose_parts, verts, tris, mi, size=A)}
    emit({"voxel": voxel, "atlas": A, "ms_per_call": alternate(sides, args.runs, 1),
          "launches": {"bake_normal_map": launches(sides["bake_normal_map"])}})
    # a frame of the textured animation: skin_pose, rasterize_mesh and one shade launch, with and without the map
    rig = extract_rigged_mesh(m, pose_parts, center, voxel, MESH_TH, mi, texture_size=A, normal_map_size=A)
    posed = torch.empty((1,) + tuple(rig.vertices.shape), device="cuda")

    def frame(mapped):
        skin_mesh(m, rig, pose_parts, mi["bone_length"], out=posed)
        f = rasterize_mesh(posed[0], rig.triangles, K, SIZE, R)
        if mapped:
            return ops.shade_normal_mapped(f.pix_to_face, f.bary, f.normals, posed[0], rig.triangles, rig.normal_map.texture,
                                           texture=rig.texture.texture).image
        return ops.shade_textured(f.pix_to_face, f.bary, f.normals, posed[0], rig.triangles, rig.texture.texture).image

    f = rasterize_mesh(rig.vertices, rig.triangles, K, SIZE, R)
    shade_only = {"shade_textured": lambda: ops.shade_textured(f.pix_to_face, f.bary, f.normals, rig.vertices, rig.triangles,
                                                               rig.texture.texture),
                  "shade_normal_mapped": lambda: ops.shade_normal_mapped(f.pix_to_face, f.bary, f.normals, rig.vertices, rig.triangles,
                                                                         rig.normal_map.texture, texture=rig.texture.texture)}
    emit({"voxel": voxel, "atlas": A, "R": R, "animation_frame_ms": alternate({"textured": lambda: frame(False),
                                                                             "textured_normal_mapped": lambda: frame(True)}, args.runs, args.batch),
          "shade_launch_ms": alternate(shade_only, args.runs, args.batch)})
    # a still frame: the map against the per-pixel field query it replaces
    field = (m, pose_parts, mi)
    still = {"paint_normal_mapped_mesh": lambda: paint_normal_mapped_mesh(rig.vertices, rig.triangles, rig.normal_map, K, SIZE, R, atlas=rig.texture),
             "paint_textured_mesh_field_normals": lambda: paint_textured_mesh(rig.vertices, rig.triangles, rig.texture, K, SIZE, R, normals="field", field=field),
             "paint_textured_mesh": lambda: paint_textured_mesh(rig.vertices, rig.triangles, rig.texture, K, SIZE, R)}
    emit({"voxel": voxel, "atlas": A, "R": R, "still_frame_ms": alternate(still, args.runs, args.batch),
          "launches": {k: launches(fn) for k, fn in still.items()}})


def angles(m, K, pose_parts, mi, verts, tris, voxel, A, emit):
    """the mean angle between the shading normal and the field's own normal at the covered pixels, per simplification"""
    for cells in (2, 4, 8):
        small = ops.simplify_mesh(verts, tris, cells * voxel)
        sv, st = small.vertices, small.triangles
        try:
            nmap = bake_normal_map(m, pose_parts, sv, st, mi, size=A, want_float=True)
        except NotImplementedError as e:
            emit({"voxel": voxel, "cells": cells, "atlas": A, "unsupported": str(e)})
            continue
        f = rasterize_mesh(sv, st, K, SIZE, R)
        cov = f.pix_to_face >= 0
        surface = (f.bary[..., None] * sv[st[f.pix_to_face.clamp(min=0)]]).sum(-2)
        truth = field_normals(m, pose_parts, surface.reshape(-1, 3), mi).reshape(R, R, 3)
        has = cov & (truth.abs().sum(-1) > 0)
        row = {"voxel": voxel, "simplify_cells": cells, "atlas": A, "cell": nmap.cell, "T": int(st.shape[0]), "pixels": int(has.sum())}
        shading = {"face": F.normalize(f.normals, dim=-1)}
        for name, use_float in (("map_8bit", False), ("map_fp32", True)):
            shading[name] = paint_normal_mapped_mesh(sv, st, nmap, K, SIZE, R, lit=False, use_float=use_float)[1].normal
        for name, ns in shading.items():
            cosine = (ns[has].double() * truth[has].double()).sum(-1).clamp(-1, 1)
            row[f"mean_angle_deg_{name}"] = round(float(torch.rad2deg(torch.acos(cosine)).mean()), 3)
        emit(row)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--voxels", default="0.02,0.05")
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r23_nmap.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nmap.py measures on the GPU; none is available (nothing was measured)")

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
    emit({"device": torch.cuda.get_device_name(0), "runs": args.runs, "batch": args.batch, "ms": "[median, min, max]"})
    voxels = [float(v) for v in args.voxels.split(",")]
    sizes = [int(a) for a in args.sizes.split(",")]
    for voxel in voxels:
        verts, tris = extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)
        frag = rasterize_mesh(verts, tris, K, SIZE, R)
        emit({"voxel": voxel, "size": SIZE, "R": R, "V": verts.shape[0], "T": tris.shape[0], "covered": int((frag.pix_to_face >= 0).sum())})
        fit = kernels(m, pose_parts, mi, verts, tris, frag, voxel, sizes, args, emit)
        if fit:
            end_to_end(m, pose, bl, K, center, pose_parts, mi, verts, tris, voxel, fit[0], args, emit)
    verts, tris = extract_mesh(m, pose_parts, center, min(voxels), MESH_TH, mi)
    angles(m, K, pose_parts, mi, verts, tris, min(voxels), sizes[0] if len(sizes) == 1 else sizes[1], emit)
    log.close()


if __name__ == "__main__":
    main()
