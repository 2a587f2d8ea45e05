#!/usr/bin/env python3
"""Throughput of the create_mesh density sweep (667^3 = 297 M points at the reference's voxel_size 0.003), through the
model mirror: TriPlaneNARF.density_volume -> one lattice-mode launch of enarf_query_fwd. OFFSET=x moves the lattice x
units away from the body (an all-empty sweep: the fixed cost per tile).

Then the whole extraction (extract_mesh: sweep -> HIP marching cubes -> transform) at voxel 0.01 and 0.003, after a
warm-up, timed with device events per phase: sweep, count + scan (to the totals read), emit. Prints V and T."""
import ctypes as C
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from enarf_gan_amd import synth, _mesh_lib
from enarf_gan_amd.models.narf import TriPlaneNARF

sc = synth.make_scene(128, 1, "center_fixed", 20)
m = TriPlaneNARF(synth.nerf_config(origin_location="center_fixed"), 20, 24, parent=sc["parents"], num_bone_param=23)
m.register_canonical_pose(sc["canonical_pose"])
m.load_state_dict({f"mlp.{k}": v for k, v in sc["mlp"].items()}, strict=False)
with torch.no_grad():
    m.tri_plane.copy_(sc["tri_plane"][:1])
m = m.cuda().eval()
pose, bl, z = sc["pose_to_camera"].cuda(), sc["bone_length"].cuda(), sc["z_rend"].cuda()
from enarf_gan_amd.libraries.NARF.mesh_rendering import density_volume, extract_mesh
center, pose_parts, mi = m._mesh_inputs(pose, None, z, bl, 0.4)
center = center.clone()
center[:, 0] += float(os.environ.get("OFFSET", "0"))                # the lattice moved sideways, away from the body
for voxel in (0.01, 0.003):
    density_volume(m, pose_parts, center, 0.05, mi)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = density_volume(m, pose_parts, center, voxel, mi)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"voxel {voxel}: {vol.shape[0]}^3 = {vol.numel() / 1e6:.1f} M points in {dt * 1e3:.1f} ms = {vol.numel() / dt / 1e9:.2f} G points/s, "
          f"occupied (> 15): {float((vol > 15).float().mean()) * 100:.2f} %", flush=True)
    del vol

# extraction, phase by phase (the same calls _mesh_lib.marching_cubes makes), median of REPS after one warm-up
MESH_TH, REPS = 15.0, 5
lib = _mesh_lib.load()
for voxel in (0.01, 0.003):
    extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)          # warm-up: code objects, allocator
    torch.cuda.synchronize()
    rows = []
    for _ in range(REPS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        t0 = time.perf_counter()
        ev[0].record()
        vol = density_volume(m, pose_parts, center, voxel, mi)
        ev[1].record()
        X, Y, Z = vol.shape
        ws = torch.empty(lib.enarf_mesh_workspace_bytes(X, Y, Z), dtype=torch.uint8, device="cuda")
        totals = torch.empty(2, dtype=torch.int64, device="cuda")
        _mesh_lib.check(lib.enarf_mesh_count(vol.data_ptr(), X, Y, Z, MESH_TH, ws.data_ptr(), totals.data_ptr(), stream), "count")
        ev[2].record()
        V, T = (int(x) for x in totals.cpu())
        verts = torch.empty(V, 3, dtype=torch.float32, device="cuda")
        tris = torch.empty(T, 3, dtype=torch.int64, device="cuda")
        e_emit = torch.cuda.Event(enable_timing=True)
        e_emit.record()
        if V:
            _mesh_lib.check(lib.enarf_mesh_emit(vol.data_ptr(), X, Y, Z, MESH_TH, ws.data_ptr(), verts.data_ptr(),
                                                tris.data_ptr(), stream), "emit")
        ev[3].record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rows.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), e_emit.elapsed_time(ev[3]), wall * 1e3))
        del vol, ws, verts, tris
    rows.sort(key=lambda r: r[3])
    sweep, count, emit, wall = rows[len(rows) // 2]
    # bytes a single pass must read: the volume once
    gb = X * Y * Z * 4 / 1e9
    print(f"extract voxel {voxel}: {X}^3, V = {V}, T = {T}; sweep {sweep:.3f} ms, count+scan {count:.3f} ms "
          f"({gb / count:.2f} TB/s of volume), emit {emit:.3f} ms ({gb / emit:.2f} TB/s of volume), "
          f"marching cubes {count + emit:.3f} ms, wall {wall:.1f} ms (median of {REPS})", flush=True)
v, t = extract_mesh(m, pose_parts, center, 0.003, MESH_TH, mi)
torch.cuda.synchronize()
print(f"extract_mesh voxel 0.003: vertices {tuple(v.shape)}, triangles {tuple(t.shape)}, "
      f"index range [{int(t.min())}, {int(t.max())}], bbox {v.min(0).values.tolist()} .. {v.max(0).values.tolist()}")
