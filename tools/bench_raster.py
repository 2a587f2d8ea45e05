#!/usr/bin/env python3
"""Mesh rasterisation at the demo's output size (R = 512) on the synthetic scene of tools/bench_mesh.py.

extract_mesh at voxel 0.01 (201^3) and 0.003 (667^3, the demo's), then rasterize_mesh of that mesh with the scene's
camera, after a warm-up, timed with device events (median of 5): extract_mesh, rasterize_mesh, and the one host copy
of the image. Prints T, the covered pixels and the number of triangles whose pixel box exceeds the depth pass's limit
(they go to raster_big_kernel; counted here with torch from the same projection). Kernel by kernel: run it under
`rocprofv3 --kernel-trace --stats`."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from enarf_gan_amd import synth
from enarf_gan_amd.models.narf import TriPlaneNARF
from enarf_gan_amd.libraries.NARF.mesh_rendering import extract_mesh, rasterize_mesh

SIZE, R, MESH_TH, REPS, BIG = 128, 512, 15.0, 5, 256     # BIG = kBigPixels of csrc/enarf_raster.hip
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


def big_triangles(verts, tris):
    """triangles drawn with a pixel-centre box above BIG (the box rule of raster_depth_kernel, in fp64)"""
    k = K[0].double()
    s = SIZE / R
    v = verts.double()
    px = (k[0, 0] * v[:, 0] / v[:, 2] + k[0, 2]) / s
    py = (k[1, 1] * v[:, 1] / v[:, 2] + k[1, 2]) / s
    X, Y = px[tris], py[tris]
    c0 = torch.clamp(torch.floor(X.min(1).values - 0.5), min=0)
    c1 = torch.clamp(torch.ceil(X.max(1).values - 0.5), max=R - 1)
    r0 = torch.clamp(torch.floor(Y.min(1).values - 0.5), min=0)
    r1 = torch.clamp(torch.ceil(Y.max(1).values - 0.5), max=R - 1)
    n = torch.clamp(c1 - c0 + 1, min=0) * torch.clamp(r1 - r0 + 1, min=0)
    return int(((n > BIG) & (v[tris][:, :, 2] > 0).all(1)).sum())


for voxel in (0.01, 0.003):
    verts, tris = extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)      # warm-up: code objects, allocator
    rasterize_mesh(verts, tris, K, SIZE, R).image.cpu()
    torch.cuda.synchronize()
    rows = []
    for _ in range(REPS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        t0 = time.perf_counter()
        ev[0].record()
        verts, tris = extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)
        ev[1].record()
        out = rasterize_mesh(verts, tris, K, SIZE, R)
        ev[2].record()
        img = out.image.cpu()
        ev[3].record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rows.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3]), wall * 1e3))
    rows.sort(key=lambda r: r[1])
    ext, ras, copy, wall = rows[len(rows) // 2]
    covered = int((out.pix_to_face >= 0).sum())
    lit = float((out.image[..., 0][out.pix_to_face >= 0] > 127).float().mean()) if covered else 0.0
    print(f"voxel {voxel}: V = {verts.shape[0]}, T = {tris.shape[0]}, R = {R}: covered pixels {covered} "
          f"({covered / R / R * 100:.1f} %, {lit * 100:.1f} % of them lit), big triangles {big_triangles(verts, tris)}; "
          f"extract_mesh {ext:.3f} ms, rasterize_mesh {ras:.3f} ms, image to host {copy:.3f} ms, "
          f"wall {wall:.1f} ms (median of {REPS} by rasterize_mesh)", flush=True)
    del verts, tris, out
