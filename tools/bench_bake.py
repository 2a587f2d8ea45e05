#!/usr/bin/env python3
"""Texture atlases (libenarf_bake.so) on the synthetic scene of tools/bench_mesh.py, for the meshes extract_mesh gives at
voxel 0.02 and 0.05 (meshes coarse enough for other tools; the scene fills its volume, so the mesh at 0.02 still has 243 k
triangles and does not fit an atlas below 2094).

For atlases of 1024, 2048 and 4096 texels a side (a size the layout cannot fit the mesh into is reported and left out):
  points   ops.bake_points - one launch of bake_points_kernel - against the same points and owners composed from torch
           calls (index arithmetic on the texel grid, gathers, fp64);
  resolve  ops.bake_resolve on the query's colours - one launch of bake_resolve_kernel - against torch calls;
  shade    ops.shade_textured at R = 512 on the buffers of rasterize_mesh - one launch of bake_shade_kernel - against torch
           calls (the uv from index arithmetic, the tap by grid_sample);
each timed with device events over --batch back-to-back calls, the sides taking turns, the median of --runs rounds with the
spread (min, max), and the kernel launches of one call of each. Then bake_texture end to end beside extract_mesh, and
render_textured_mesh beside render_colored_mesh (single calls, median of --runs). Last, a sine pattern with a wavelength
of two voxels baked into the atlas against the same pattern on the vertices: the mean absolute error of either albedo
against the pattern at each pixel's surface point. One JSON line per result, also appended to --log. Needs a GPU: there
is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.mesh_rendering import (bake_texture, extract_mesh, paint_mesh, paint_textured_mesh,  # noqa: E402
                                                         rasterize_mesh)
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
    """{name: fn} -> {name: [median, min, max] ms per call}, the sides taking turns within each round"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            times[k].append(timed(fn, batch))
    return {k: [round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)] for k, v in times.items()}


def _corner_table(c, dev):
    return torch.tensor([[[1, 1], [c - 3, 1], [1, c - 3]], [[c - 1, c - 1], [3, c - 1], [c - 1, 3]]], dtype=torch.float64, device=dev)


def torch_points(verts, tris, A, lay):
    """bake_points from torch calls, fp64"""
    c, n, _ = lay
    dev, T = verts.device, tris.shape[0]
    y, x = torch.meshgrid(torch.arange(A, device=dev), torch.arange(A, device=dev), indexing="ij")
    cx, cy = x // c, y // c
    i, j = x - cx * c, y - cy * c
    h = (i + j + 1 > c).long()
    face = 2 * (cy * n + cx) + h
    own = (cx < n) & (cy < n) & (face < T)
    idx = tris[face.clamp(max=T - 1)]
    own &= ((idx >= 0) & (idx < verts.shape[0])).all(-1)
    u, w = i.double() + 0.5, j.double() + 0.5
    a1 = torch.where(h == 0, u - 1, (c - 1) - u) / (c - 4)
    a2 = torch.where(h == 0, w - 1, (c - 1) - w) / (c - 4)
    a0 = 1 - a1 - a2
    q = verts.double()[idx.clamp(0, verts.shape[0] - 1)]
    p = a0[..., None] * q[..., 0, :] + a1[..., None] * q[..., 1, :] + a2[..., None] * q[..., 2, :]
    p = torch.where(own[..., None], p, torch.zeros_like(p))
    return p.reshape(-1, 3).t().float().contiguous(), torch.where(own, face, -torch.ones_like(face)).int()


def torch_resolve(face, color):
    own = (face >= 0).reshape(-1)
    v = torch.where(own[:, None], (color.double().t() + 1) / 2, torch.zeros(1, dtype=torch.float64, device=face.device))
    rgb = (255 * v.nan_to_num(0).clamp(0, 1)).floor().to(torch.uint8)
    alpha = torch.where(own, 255, 0).to(torch.uint8)
    return torch.cat([rgb, alpha[:, None]], 1).reshape(face.shape + (4,))


def torch_shade(f, verts, tris, texture, lay):
    """shade_textured(lit=True) from torch calls on the rasteriser's buffers"""
    c, n, _ = lay
    A = texture.shape[0]
    drawn = f.pix_to_face >= 0
    face = f.pix_to_face.clamp(min=0)
    idx = tris[face]
    q, h = face // 2, face % 2
    origin = torch.stack([(q % n) * c, (q // n) * c], -1).double()
    U = origin[..., None, :] + _corner_table(c, verts.device)[h]            # (R, R, 3, 2)
    b = f.bary.double()[..., None]
    uv = (b * U).sum(-2)
    grid = (uv / A * 2 - 1).float()[None]
    tex = (texture[..., :3].float() / 255).permute(2, 0, 1)[None]
    texel = F.grid_sample(tex, grid, mode="bilinear", padding_mode="border", align_corners=False)[0].permute(1, 2, 0).double()
    p = (b * verts[idx].double()).sum(-2)
    nn = f.normals.double()
    N = nn / nn.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    cosine = -(N * p).sum(-1) / p.norm(dim=-1).clamp(min=1e-6)
    spec = torch.where(cosine > 0, (2 * cosine * cosine - 1).clamp(min=0) ** 64, torch.zeros_like(cosine))
    shaded = texel * (0.5 + 0.3 * cosine.clamp(min=0))[..., None] + 0.2 * spec[..., None]
    texel = torch.where(drawn[..., None], texel, torch.ones_like(texel))
    shaded = torch.where(drawn[..., None], shaded, torch.ones_like(shaded))
    return (255 * shaded.clamp(0, 1)).floor().to(torch.uint8), texel.float(), shaded.float()


def measure(m, pose, bl, z, K, center, pose_parts, mi, voxel, sizes, args, emit):
    """every figure of one mesh: the extract_mesh mesh of the scene at `voxel`, atlases of `sizes` (a size too small for the
    mesh is reported as such and left out)"""
    verts, tris = extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)
    frag = rasterize_mesh(verts, tris, K, SIZE, R)
    emit({"voxel": voxel, "size": SIZE, "R": R,
          "V": verts.shape[0], "T": tris.shape[0], "covered": int((frag.pix_to_face >= 0).sum()), "ms": "[median, min, max]"})

    fit = []
    for A in sizes:
        try:
            lay = ops.bake_layout(tris.shape[0], A)
        except NotImplementedError as e:
            emit({"voxel": voxel, "atlas": A, "unsupported": str(e)})
            continue
        fit.append(A)
        atlas = bake_texture(m, pose_parts, verts, tris, mi, size=A)
        baked = ops.bake_points(verts, tris, A)
        color = torch.rand(3, A * A, device="cuda") * 2 - 1
        sides = {"points": lambda: ops.bake_points(verts, tris, A), "points_torch": lambda: torch_points(verts, tris, A, lay),
                 "resolve": lambda: ops.bake_resolve(baked.texel_face, color=color),
                 "resolve_torch": lambda: torch_resolve(baked.texel_face, color),
                 "shade": lambda: ops.shade_textured(frag.pix_to_face, frag.bary, frag.normals, verts, tris, atlas.texture),
                 "shade_torch": lambda: torch_shade(frag, verts, tris, atlas.texture, lay)}
        got, want = sides["shade"](), sides["shade_torch"]()
        pt, ft = sides["points_torch"]()
        ms = alternate(sides, args.runs, args.batch)
        emit({"voxel": voxel, "atlas": A, "cell": lay.cell, "fill": round((lay.cell - 4) ** 2 / lay.cell ** 2, 4), "ms_per_call": ms,
              "launches": {k: launches(fn) for k, fn in sides.items()},
              "GBps_points_stores": round(16 * A * A / ms["points"][0] / 1e6, 1),
              "points_vs_torch_max_abs": float((baked.points - pt).abs().max()), "owners_equal": bool(torch.equal(baked.texel_face, ft)),
              "resolve_equal": bool(torch.equal(sides["resolve"]().texture, sides["resolve_torch"]())),
              "shade_vs_torch_max_level": int((got.image.int() - want[0].int()).abs().max())})
        del atlas, baked, color, got, want, pt, ft

    if not fit:
        return
    A = fit[0]
    plain = lambda: extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)
    bake = lambda: bake_texture(m, pose_parts, verts, tris, mi, size=A)
    textured = lambda: m.render_textured_mesh(pose, K, None, z, bl, voxel, MESH_TH, 0.4, SIZE, A)
    coloured = lambda: m.render_colored_mesh(pose, K, None, z, bl, voxel, MESH_TH, 0.4, SIZE)
    emit({"voxel": voxel, "atlas": A, "ms_per_call": alternate({"extract_mesh": plain, "bake_texture": bake, "render_textured_mesh": textured,
                                                "render_colored_mesh": coloured}, args.runs, 1),
          "launches": {"bake_texture": launches(bake)}})

    # detail: a sine pattern of wavelength two voxels, in the atlas and on the vertices, against the pattern itself
    k = torch.tensor([1.0, 0.8, 0.6], device="cuda", dtype=torch.float64) * (3.141592653589793 / voxel)
    pattern = lambda p: 0.5 + 0.5 * torch.sin(p.double() * k)
    for A in fit:
        atlas = bake_texture(None, None, verts, tris, size=A, color_fn=pattern)
        f, tex = paint_textured_mesh(verts, tris, atlas, K, SIZE, R, lit=False)
        _, vert = paint_mesh(verts, tris, K, SIZE, R, vertex_colors=pattern(verts).float(), lit=False)
        cov = f.pix_to_face >= 0
        surface = (f.bary.double()[..., None] * verts[tris[f.pix_to_face.clamp(min=0)]].double()).sum(-2)
        truth = pattern(surface)[cov]
        emit({"voxel": voxel, "atlas": A, "cell": atlas.cell, "pattern_wavelength_voxels": 2,
              "mean_abs_error_textured": float((tex.albedo[cov].double() - truth).abs().mean()),
              "mean_abs_error_vertex_colours": float((vert.albedo[cov].double() - truth).abs().mean())})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--voxels", default="0.02,0.05")
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r20_bake.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bake.py measures on the GPU; none is available (nothing was measured)")

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
    emit({"device": torch.cuda.get_device_name(0), "runs": args.runs, "batch": args.batch})
    for voxel in (float(v) for v in args.voxels.split(",")):
        measure(m, pose, bl, z, K, center, pose_parts, mi, voxel, [int(a) for a in args.sizes.split(",")], args, emit)
    log.close()


if __name__ == "__main__":
    main()
