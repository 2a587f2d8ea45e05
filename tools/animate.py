#!/usr/bin/env python3
"""Moving pictures of one identity of an ENARF-GAN snapshot, on the device from the key poses to the bytes:
TriNARFGenerator.render_animation (one interpolate_pose launch, one tri-plane, the frames marched in chunks on it, one
compose_frames launch per chunk) and a single copy of the finished uint8 frames to the host.

  python tools/animate.py --snapshot snapshot_latest.pth --sample-data sample_data.pickle --canonical canonical.npy \\
      --keys 0,7,19 --num 96 --orbit-turns 1 --out frames/        # PNGs frame_0000.png ... (PIL)
  python tools/animate.py ... --out walk.npy                      # one (num, S, S, 3) uint8 array
  python tools/animate.py ... --parts --out parts/                 # the part segmentation in motion (render_part_animation)
  python tools/animate.py ... --mesh-turntable field --out turn/   # the coloured mesh of the first key on a turntable
  python tools/animate.py ... --geometry normal --out shape/       # the march's own geometry in motion (render_geometry_animation)
  python tools/animate.py ... --skinned-mesh field --out skin/     # the first key's mesh, rigged once, posed per frame
  python tools/animate.py ... --skinned-mesh parts --export-glb avatar.glb --out skin/   # ... and the rig as binary glTF

The key poses, the camera and the bone lengths are entries of a sample_data.pickle (formats.read_sample_data; the
camera and bone lengths of the first key); `--canonical` is the canonical pose (24, 4, 4) the model was trained with
(the data set's canonical.npy). The generator is built from the options below with the shipping nerf_params
(synth.nerf_config, a tri-plane per identity) and the snapshot's weights are loaded into it; keys the snapshot lacks
are reported. `num` must be a multiple of the number of keys (with --no-loop: of the number of keys minus one).
`--parts` draws the frames in the colours of the part that owns each ray, over white. `--mesh-turntable field|parts`
extracts the mesh of the first key once (HIP marching cubes), in the radiance field's colours or the part colours, and
turns it through `--num` angles of one turn (render_mesh_turntable: HIP rasteriser and deferred shading per frame).
`--geometry normal|lit|depth` draws the shape the march itself carries - the normal map, a lit white surface, or the
inverse depth between `--depth-range` - from the disparity of each frame (ops.geometry_buffers, no mesh extracted).
`--normals field` shades `--geometry` and `--mesh-turntable` with the field's own normals, minus the density gradient
(libenarf_nrm.so), instead of the depth stencil's or the mesh faces'.
`--skinned-mesh field|parts|white` extracts the mesh of the first key once, binds it to the model's parts
(extract_rigged_mesh: `--influences` 4 or 8 a vertex) and moves it through the key poses by linear-blend skinning
(render_mesh_animation: one skin_pose launch a chunk, HIP rasteriser and deferred shading per frame); `--export-glb PATH`
writes that rig as a skinned binary glTF (mesh_rendering.export_glb), with or without --skinned-mesh. `--texture-size N`
bakes the field's colour into an N x N texture atlas of that mesh (libenarf_bake.so): the glTF then carries the texture in
place of the vertex colours, and `--skinned-mesh texture` draws the posed mesh with it; `--clip` writes the interpolated
sequence into the glTF as an animation clip. `--simplify CELL` simplifies the extracted mesh of --skinned-mesh,
--mesh-turntable and --export-glb to cells of CELL (libenarf_simp.so: vertex clustering with quadric placement) before it is
coloured, rigged and baked: extract at a fine --voxel-size, keep few triangles. `--normal-map-size N` bakes the field's
own normals into an N x N tangent-space normal map of that (simplified) mesh (libenarf_nmap.so): `--skinned-mesh texture`
(N must then be the texture's size) and `--skinned-mesh white` shade the posed mesh with it, and --export-glb writes it as
the material's normalTexture, with tangents."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from enarf_gan_amd import formats, synth  # noqa: E402
from enarf_gan_amd.models.generator import TriNARFGenerator  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--snapshot", required=True)
    ap.add_argument("--sample-data", required=True)
    ap.add_argument("--canonical", required=True, help="canonical pose, .npy (24, 4, 4)")
    ap.add_argument("--keys", default="0,1", help="comma-separated entries of the sample data used as key poses")
    ap.add_argument("--num", type=int, default=96)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--orbit-turns", type=float, default=0.0, help="turntable: whole turns over the sequence (0 = none)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the identity's latent")
    ap.add_argument("--truncation-psi", type=float, default=0.4)
    ap.add_argument("--frames-per-batch", type=int, default=8)
    ap.add_argument("--black-background", action="store_true")
    ap.add_argument("--parts", action="store_true", help="the part segmentation in place of the colour")
    ap.add_argument("--geometry", choices=["normal", "lit", "depth"], default=None,
                    help="the shape image of the march's depth in place of the colour")
    ap.add_argument("--depth-range", default="1.0,5.0", help="--geometry depth: near,far in the poses' units")
    ap.add_argument("--normals", choices=["default", "field"], default="default",
                    help="--geometry and --mesh-turntable: 'field' shades with the field's own normals (the density "
                         "gradient) instead of the depth stencil's or the mesh faces'")
    ap.add_argument("--mesh-turntable", choices=["field", "parts"], default=None,
                    help="a turntable of the first key's coloured mesh in place of the march")
    ap.add_argument("--skinned-mesh", choices=["field", "parts", "white", "texture"], default=None,
                    help="the first key's mesh, rigged once and posed per frame, in place of the march")
    ap.add_argument("--influences", type=int, choices=[4, 8], default=4, help="skinned mesh: parts a vertex is bound to")
    ap.add_argument("--export-glb", default=None, help="write the rigged mesh of the first key as binary glTF to this path")
    ap.add_argument("--texture-size", type=int, default=None,
                    help="bake the field's colour into a texture atlas of this size: --export-glb embeds it in place of the "
                         "vertex colours; --skinned-mesh texture draws with it (1024 when not given)")
    ap.add_argument("--clip", action="store_true",
                    help="--export-glb: write the interpolated sequence into the file as an animation clip")
    ap.add_argument("--fps", type=float, default=24.0, help="--clip: key frames a second")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL",
                    help="simplify the extracted mesh to cells of this size (the poses' units) before colouring, rigging "
                         "and baking it")
    ap.add_argument("--normal-map-size", type=int, default=None, metavar="N",
                    help="bake the field's normals into a tangent-space normal map of this size: --skinned-mesh texture|white "
                         "shade with it, --export-glb embeds it")
    ap.add_argument("--voxel-size", type=float, default=0.003, help="mesh turntable: the density sweep's voxel")
    ap.add_argument("--mesh-th", type=float, default=15.0, help="mesh turntable: the density threshold")
    ap.add_argument("--unlit", action="store_true", help="mesh turntable: the colour itself, without the Phong terms")
    ap.add_argument("--render-size", type=int, default=512, help="mesh turntable: the frames' size")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--z-dim", type=int, default=256)
    ap.add_argument("--nc", type=int, default=48)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--origin-location", default="center_fixed")
    ap.add_argument("--out", required=True, help="a directory for PNGs, or a path ending in .npy")
    args = ap.parse_args()

    dev = torch.device("cuda")
    data = formats.read_sample_data(args.sample_data)
    keys = [int(k) for k in args.keys.split(",")]
    cfg = synth.AttrDict(z_dim=args.z_dim, background_ratio=0.7, crop_background=True, pretrained_background=False,
                         nerf_params=synth.nerf_config(Nc=args.nc, Nf=args.nf, origin_location=args.origin_location,
                                                       constant_triplane=False))
    gen = TriNARFGenerator(cfg, args.size, 24, synth.SMPL_PARENTS, 23, black_background=args.black_background)
    gen.register_canonical_pose(np.load(args.canonical))
    report = formats.load_generator_snapshot(args.snapshot, gen)
    print(f"snapshot: {len(report.loaded)} tensors loaded, {len(report.missing)} missing, {len(report.ignored)} ignored"
          + (f", iteration {report.iteration}" if report.iteration is not None else ""), file=sys.stderr)
    gen = gen.to(dev).eval()

    key_poses = torch.from_numpy(data.pose_3d[keys].astype(np.float64)).to(dev)
    bone_length = torch.from_numpy(data.bone_length[keys[:1]].astype(np.float32)).to(dev)
    intrinsics = torch.from_numpy(data.intrinsics[keys[0]].astype(np.float32)).to(dev)
    shares = 3 if args.black_background else 4
    z = torch.randn(1, args.z_dim * shares, generator=torch.Generator().manual_seed(args.seed)).to(dev)
    orbit = None
    if args.orbit_turns:
        orbit = torch.arange(args.num, dtype=torch.float64, device=dev) * (2 * math.pi * args.orbit_turns / args.num)
    rig = None
    textured = args.skinned_mesh == "texture"
    if args.normal_map_size is not None and args.skinned_mesh in ("field", "parts"):
        raise SystemExit("--normal-map-size shades --skinned-mesh texture or white (the vertex colours have no normal-mapped shade)")
    if args.skinned_mesh or args.export_glb:
        rig = gen.extract_rigged_mesh(key_poses[:1].float(), z, bone_length, voxel_size=args.voxel_size, mesh_th=args.mesh_th,
                                      truncation_psi=args.truncation_psi, max_influences=args.influences,
                                      return_colors=True, return_part_labels=True,
                                      texture_size=1024 if textured and args.texture_size is None else args.texture_size,
                                      simplify_cell=args.simplify, normal_map_size=args.normal_map_size)
        if args.export_glb:
            from enarf_gan_amd import ops
            from enarf_gan_amd.libraries.NARF.mesh_rendering import export_glb
            clips = None
            if args.clip:
                poses = ops.interpolate_pose(key_poses, gen.nerf.parent_id, args.num, not args.no_loop, orbit)
                part_poses, part_lengths = gen.nerf.transform_pose(poses.float(), bone_length.expand(poses.shape[0], -1, -1))
                clips = {"sequence": (np.arange(poses.shape[0]) / args.fps, part_poses, part_lengths)}
            export_glb(rig, args.export_glb, clips=clips)
            print(f"{args.export_glb}: {len(rig.vertices)} vertices, {len(rig.triangles)} triangles, "
                  f"{rig.joints.shape[1]} influences"
                  + (f", a {rig.texture.size} x {rig.texture.size} texture (cell {rig.texture.cell})" if rig.texture else "")
                  + (f", a {rig.normal_map.size} x {rig.normal_map.size} normal map" if rig.normal_map else "")
                  + (f", a clip of {len(clips['sequence'][0])} keys" if clips else ""), file=sys.stderr)
    if textured:
        frames, _ = gen.render_textured_mesh_animation(rig, key_poses, bone_length, intrinsics, num=args.num,
                                                       loop=not args.no_loop, orbit=orbit, lit=not args.unlit,
                                                       render_size=args.render_size, frames_per_batch=args.frames_per_batch,
                                                       normal_map=args.normal_map_size is not None)
    elif args.skinned_mesh:
        frames, _ = gen.render_mesh_animation(rig, key_poses, bone_length, intrinsics, num=args.num, loop=not args.no_loop,
                                              orbit=orbit, color=None if args.skinned_mesh == "white" else args.skinned_mesh,
                                              lit=not args.unlit, render_size=args.render_size,
                                              frames_per_batch=args.frames_per_batch,
                                              normal_map=args.normal_map_size is not None)
    elif args.mesh_turntable:
        angles = torch.arange(args.num, dtype=torch.float32, device=dev) * (2 * math.pi / args.num)
        frames = gen.render_mesh_turntable(key_poses[:1].float(), intrinsics, z, bone_length, angles,
                                           voxel_size=args.voxel_size, mesh_th=args.mesh_th,
                                           truncation_psi=args.truncation_psi, color=args.mesh_turntable,
                                           lit=not args.unlit, render_size=args.render_size, simplify_cell=args.simplify,
                                           normals="field" if args.normals == "field" else "mesh")
    elif args.geometry:
        near, far = (float(v) for v in args.depth_range.split(","))
        frames, _, _ = gen.render_geometry_animation(key_poses, bone_length, intrinsics, z, num=args.num,
                                                     loop=not args.no_loop, orbit=orbit, truncation_psi=args.truncation_psi,
                                                     frames_per_batch=args.frames_per_batch, shade=args.geometry,
                                                     normals="field" if args.normals == "field" else "stencil",
                                                     near=near, far=far)
    elif args.parts:
        frames, _, _ = gen.render_part_animation(key_poses, bone_length, intrinsics, z, num=args.num, loop=not args.no_loop,
                                                 orbit=orbit, truncation_psi=args.truncation_psi,
                                                 frames_per_batch=args.frames_per_batch)
    else:
        frames, _, _ = gen.render_animation(key_poses, bone_length, intrinsics, z, num=args.num, loop=not args.no_loop,
                                            orbit=orbit, truncation_psi=args.truncation_psi,
                                            frames_per_batch=args.frames_per_batch)
    frames = frames.cpu().numpy()                                       # the one device-to-host copy
    if args.out.endswith(".npy"):
        np.save(args.out, frames)
        print(args.out, frames.shape, file=sys.stderr)
        return
    from PIL import Image
    os.makedirs(args.out, exist_ok=True)
    for i, frame in enumerate(frames):
        Image.fromarray(frame).save(os.path.join(args.out, f"frame_{i:04d}.png"))
    print(f"{args.out}: {len(frames)} PNGs of {frames.shape[1]} x {frames.shape[2]}", file=sys.stderr)


if __name__ == "__main__":
    main()
