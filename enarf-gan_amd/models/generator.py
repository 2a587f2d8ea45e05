"""Generator shells around the HIP renderer: `TriNARFGenerator` (GAN) and `DSONARFGenerator` (single dynamic scene).

They keep the constructor arguments, method names, argument order and return tuples of the reference's
`models/generator.py` (TriNARFGenerator :14-118, DSONARFGenerator :182-300) so that its train / demo scripts can switch
over; everything inside is this package's own plumbing around `TriPlaneNARF`.

The background network is the StyleGAN2 skip generator of `libraries/custom_stylegan2/net.py` (generator.py:32-38:
n_mlp 4, `crop_background` from the config, or the pretrained church generator), built on this repo's HIP ops; with
`black_background=True` / `black_bg_if_possible=True` nothing of it runs.
"""
import functools
import inspect
from typing import Optional

import numpy as np
import torch
from torch import nn

from ..libraries.custom_stylegan2.net import Generator as StyleGANGenerator
from ..libraries.custom_stylegan2.net import PretrainedStyleGAN
from ..libraries.NARF.mesh_rendering import _adds_return_normals
from ..libraries.NeRF.ray_sampler import mask_based_sampler, whole_image_grid_ray_sampler
from .narf import TriPlaneNARF


def _passes_on(keyword, default, callee, with_size=False):
    """Decorator of a generator method that hands its arguments to the TriPlaneNARF method `callee`, which takes them after
    (z_nerf, z_render) in place of z: adds `keyword` (at `default`: the method as it stands), which goes to that method
    with the method's own arguments (and img_size = the generator's size `with_size`). The method keeps its signature."""
    def decorate(method):
        signature = inspect.signature(method)

        @functools.wraps(method)
        def wrapper(self, *args, **kwargs):
            value = kwargs.pop(keyword, default)
            if value == default:
                return method(self, *args, **kwargs)
            inner = {k: kwargs.pop(k) for k in list(kwargs) if k not in signature.parameters}    # an inner decorator's keywords
            bound = signature.bind(self, *args, **kwargs)
            bound.apply_defaults()
            a = dict(bound.arguments)
            a.pop("self")
            z_nerf, z_render, _ = self._latent_parts(a.pop("z"))
            if with_size:
                a["img_size"] = self.size
            return getattr(self.nerf, callee)(z=z_nerf, z_rend=z_render, **a, **inner, **{keyword: value})
        return wrapper
    return decorate


class _RendererShell(nn.Module):
    """What both generators share: the config / size bookkeeping and the tri-plane NARF they wrap."""

    def __init__(self, config, size, num_bone, parent_id, num_bone_param, z_dim, **nerf_kwargs):
        super().__init__()
        self.config, self.size, self.num_bone = config, size, num_bone
        params = config.nerf_params
        # with the head as an extra part every joint has a bone-length parameter (generator.py:30-31, :198-199)
        n_param = num_bone if params.origin_location == "center+head" else num_bone_param
        self.nerf = TriPlaneNARF(params, z_dim=z_dim, num_bone=num_bone, bone_length=True, parent=parent_id,
                                 num_bone_param=n_param, **nerf_kwargs)

    @property
    def memory_cost(self):
        return self.nerf.memory_cost

    @property
    def flops(self):
        return self.nerf.flops

    def register_canonical_pose(self, pose: np.ndarray):
        self.nerf.register_canonical_pose(pose)

    @property
    def _samples(self):
        p = self.config.nerf_params
        return dict(Nc=p.Nc, Nf=p.Nf)


class TriNARFGenerator(_RendererShell):
    def __init__(self, config, size, num_bone=1, parent_id=None, num_bone_param=None, black_background=False):
        super().__init__(config, size, num_bone, parent_id, num_bone_param, z_dim=[2 * config.z_dim, config.z_dim])
        self.ray_sampler = whole_image_grid_ray_sampler
        self.background_ratio = config.background_ratio
        self.black_background = black_background
        self.background_generator = None
        if not black_background:                   # generator.py:32-38
            if config.pretrained_background:
                self.background_generator = PretrainedStyleGAN()
            else:
                self.background_generator = StyleGANGenerator(size=size, style_dim=config.z_dim, n_mlp=4, last_channel=3,
                                                              crop_background=config.crop_background)

    def normalized_inv_intrinsics(self, intrinsics: torch.Tensor):
        bottom = intrinsics.new_tensor([[0, 0, 1]])
        return torch.linalg.inv(torch.cat([intrinsics[:2] / self.size, bottom], dim=0))

    def _latent_parts(self, z: torch.Tensor):
        """z = [tri-plane (2u) | renderer (u) | background (u, absent on black)] -> (z_nerf, z_render, z_bg or None)."""
        shares = 3 if self.black_background else 4
        u = z.shape[1] // shares
        pieces = torch.split(z, [2 * u, u] + [u] * (shares - 3), dim=1)
        return pieces[0], pieces[1], (pieces[2] if shares == 4 else None)

    def _background(self, z_bg, z_render, force_black: bool):
        if self.black_background or force_black:
            return -1
        bg = self.background_generator
        image, _ = bg([z_bg, z_render], inject_index=bg.n_latent - 4)
        return image

    def forward(self, pose_to_camera, pose_to_world, bone_length, z=None, inv_intrinsics=None,
                return_intermediate=False, truncation_psi=1, black_bg_if_possible=False, return_disparity=False,
                return_bg=False):
        if self.num_bone != 1 and (bone_length is None or pose_to_camera is None):
            raise AssertionError("bone_length and pose_to_camera are required")
        B, S = pose_to_camera.shape[0], self.size
        _, pixels = self.ray_sampler(S, S, B, device=pose_to_camera.device)
        z_nerf, z_render, z_bg = self._latent_parts(z)
        K_inv = torch.as_tensor(inv_intrinsics).float().to(pixels.device)
        rendered = self.nerf(B, pixels, pose_to_camera, K_inv, z_nerf, z_render, bone_length,
                             return_intermediate=return_intermediate, truncation_psi=truncation_psi,
                             return_disparity=return_disparity, **self._samples)
        person = rendered[0].reshape(B, 3, S, S)
        alpha = rendered[1].reshape(B, S, S)
        backdrop = self._background(z_bg, z_render, black_bg_if_possible)
        image = person + (1 - alpha[:, None]) * backdrop
        if return_intermediate:                      # (fine_points, fine_density) ride along as the last item
            points, density = rendered[-1]
            return image, alpha, points, density
        if return_disparity:                         # back to metric units
            return image, alpha, rendered[2] * self.config.nerf_params.coordinate_scale
        if return_bg:
            return person, alpha, backdrop
        side = self.nerf.buffers_tensors
        return image, alpha, side["fine_weights"], side["fine_depth"]


    def render_mesh(self, pose_to_camera, intrinsics, z, bone_length, voxel_size=0.003, mesh_th=15, truncation_psi=0.4):
        """models/generator.py:120-129."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.render_mesh(pose_to_camera, intrinsics, z_nerf, z_render, bone_length, voxel_size, mesh_th,
                                     truncation_psi, self.size)

    def create_mesh(self, pose_to_camera, z, bone_length, voxel_size=0.003, mesh_th=15, truncation_psi=0.4):
        """models/generator.py:131-140 (whose call passes arguments `create_mesh` does not take and cannot run as
        written): the same sweep as render_mesh, returning (vertices, triangles, textures)."""
        from ..libraries.NARF.mesh_rendering import create_mesh
        z_nerf, z_render, _ = self._latent_parts(z)
        center, pose_parts, model_input = self.nerf._mesh_inputs(pose_to_camera, z_nerf, z_render, bone_length,
                                                                 truncation_psi)
        return create_mesh(self.nerf, pose_parts, center=center, voxel_size=voxel_size, mesh_th=mesh_th,
                           model_input=model_input)

    def density_volume(self, pose_to_camera, z, bone_length, voxel_size=0.003, truncation_psi=0.4):
        """The density grid behind render_mesh / create_mesh, without the third-party marching cubes."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.density_volume(pose_to_camera, z_nerf, z_render, bone_length, voxel_size, truncation_psi)

    @_adds_return_normals(lambda a: a["self"].nerf.mesh_field(a["pose_to_camera"], *a["self"]._latent_parts(a["z"])[:2],
                                                              a["bone_length"], a["truncation_psi"]))
    def extract_mesh(self, pose_to_camera, z, bone_length, voxel_size=0.003, mesh_th=15, truncation_psi=0.4,
                     return_part_labels=False, return_colors=False, simplify_cell=None):
        """create_mesh's (vertices, triangles) built on the device (HIP marching cubes); one sample, as create_mesh.
        `return_part_labels` adds the (V,) int32 part that owns each vertex, `return_colors` the (V, 3) fp32 colour of
        the field at each vertex, in [0, 1] (after the labels when both are asked for). `simplify_cell` = h simplifies
        the mesh to cells of h camera units straight after marching cubes (HIP vertex clustering with quadric placement):
        extract fine, keep few triangles; labels and colours are then those of the simplified vertices. The keyword
        `return_normals` (mesh_rendering._adds_return_normals) adds, last, the (V, 3) fp32 unit normals of the field itself
        at the final vertices (HIP density gradient)."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.extract_mesh(pose_to_camera, z_nerf, z_render, bone_length, voxel_size, mesh_th, truncation_psi,
                                      return_part_labels, return_colors, simplify_cell)

    @torch.no_grad()
    def render_part_map(self, pose_to_camera, bone_length, z, inv_intrinsics, truncation_psi=1):
        """The part segmentation of the frames forward() renders: (semantic image (B, 3, S, S) in the colours of
        rendering.semantic_palette, part_map (B, S, S) int32 - the part that carries the most weight along each ray, -1
        where none does -, mask (B, S, S)), all on the device, with no host synchronisation inside."""
        B, S = pose_to_camera.shape[0], self.size
        _, pixels = self.ray_sampler(S, S, B, device=pose_to_camera.device)
        z_nerf, z_render, _ = self._latent_parts(z)
        K_inv = torch.as_tensor(inv_intrinsics).float().to(pixels.device)
        color, mask = self.nerf(B, pixels, pose_to_camera, K_inv, z_nerf, z_render, bone_length,
                                truncation_psi=truncation_psi, semantic_map=True, **self._samples)
        part_map = self.nerf.buffers_tensors["part_map"]
        return color.reshape(B, 3, S, S), part_map.reshape(B, S, S), mask.reshape(B, S, S)

    def render_geometry(self, pose_to_camera, bone_length, z, inv_intrinsics, truncation_psi=1, shade="normal",
                        normals="stencil", **buffer_kwargs):
        """The geometry of the frames forward() renders, from the march's own disparity: (image (B, S, S, 3) uint8 - the
        shape image in `shade` = "normal", "lit" or "depth" -, the GeometryBuffers of ops.geometry_buffers (depth, points,
        normals, flags, image), colour (B, 3, S, S), mask (B, S, S)), all on the device, one march and one launch more,
        with no host synchronisation inside. Depth and points are metric, in the space of pose_to_camera and of
        extract_mesh's vertices; buffer_kwargs go to ops.geometry_buffers (edge, mask_threshold, near, far, background,
        want, ...). normals="field" replaces normals, flags and image by the field's own normals (the HIP density gradient
        composited along each ray, the stencil normals as the fallback; TriPlaneNARF.render_geometry)."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.render_geometry(pose_to_camera, inv_intrinsics, z_nerf, z_render, bone_length, self.size,
                                         truncation_psi=truncation_psi, shade=shade, normals=normals, **self._samples,
                                         **buffer_kwargs)

    def render_extracted_mesh(self, pose_to_camera, intrinsics, z, bone_length, voxel_size=0.003, mesh_th=15,
                              truncation_psi=0.4):
        """render_mesh built on the device (HIP marching cubes, HIP hard-Phong rasteriser): (image (512, 512, 3) uint8
        numpy, (vertices, triangles)); one sample, as render_mesh."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.render_extracted_mesh(pose_to_camera, intrinsics, z_nerf, z_render, bone_length, voxel_size,
                                               mesh_th, truncation_psi, self.size)

    def render_colored_mesh(self, pose_to_camera, intrinsics, z, bone_length, voxel_size=0.003, mesh_th=15,
                            truncation_psi=0.4, color="field", lit=True, normals="mesh"):
        """render_extracted_mesh in colour: the mesh carries the radiance field's colour at each vertex (color="field")
        or the colour of the part that owns it (color="parts", (semantic_palette + 1) / 2), drawn by the HIP rasteriser
        and the HIP deferred shading; `lit` keeps the hard-Phong terms. (image (512, 512, 3) uint8 numpy, (vertices,
        triangles, colours (V, 3) fp32 or labels (V,) int32)); one sample, as render_mesh. normals="field" shades every
        covered pixel with the field's own normal instead of the interpolated face normal."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.render_colored_mesh(pose_to_camera, intrinsics, z_nerf, z_render, bone_length, voxel_size,
                                             mesh_th, truncation_psi, self.size, color, lit, normals)

    def render_mesh_turntable(self, pose_to_camera, intrinsics, z, bone_length, angles, voxel_size=0.003, mesh_th=15,
                              truncation_psi=0.4, color="field", lit=True, render_size=512, simplify_cell=None,
                              normals="mesh"):
        """The coloured mesh of render_colored_mesh (simplified to cells of `simplify_cell` when given) on a turntable: (num, R, R, 3) uint8 frames on the device, frame i
        the mesh turned by angles[i] about the y axis through the mean joint translation (rotate_mesh_by_angle). The
        mesh and its colours or labels are extracted once; every angle is one rotate_mesh_by_angle, one rasterize_mesh
        and one shade_fragments, with no host synchronisation inside. angles: num numbers or a (num,) tensor.
        normals="field" shades every covered pixel with the field's own normal: the pixel's surface point is turned back
        into the extraction pose, the field's normal taken there (one gradient launch a frame) and turned with the mesh."""
        from .. import ops
        from ..libraries.NARF.mesh_rendering import field_normals, rasterize_mesh
        from ..libraries.NARF.pose_utils import rotate_mesh_by_angle
        z_nerf, z_render, _ = self._latent_parts(z)
        vertices, triangles, _, how = self.nerf._colored_mesh(pose_to_camera, z_nerf, z_render, bone_length, voxel_size,
                                                              mesh_th, truncation_psi, color, simplify_cell)
        dev, R = vertices.device, int(render_size)
        angles = torch.as_tensor(angles).to(device=dev, dtype=torch.float32).reshape(-1)
        frames = torch.empty((angles.shape[0], R, R, 3), dtype=torch.uint8, device=dev)
        pose = pose_to_camera.to(device=dev, dtype=torch.float32)
        if normals not in ("mesh", "field"):
            raise ValueError(f"normals is 'mesh' or 'field', got {normals!r}")
        if normals == "field":
            _, pose_parts, model_input = self.nerf.mesh_field(pose_to_camera, z_nerf, z_render, bone_length, truncation_psi)
        for i in range(angles.shape[0]):
            turned = rotate_mesh_by_angle(pose, (vertices,), angles[i:i + 1])[0].contiguous()
            f = rasterize_mesh(turned, triangles, intrinsics, self.size, R)
            shading = f.normals
            if normals == "field":
                # barycentrics are those of the turned mesh; the same mix of the unturned corners is the point the field knows
                face = f.pix_to_face
                points = (f.bary[..., None] * vertices[triangles[face.clamp(min=0)]]).sum(dim=-2).reshape(-1, 3)
                n = field_normals(self.nerf, pose_parts, points, model_input)
                ends = rotate_mesh_by_angle(pose, (points + n,), angles[i:i + 1])[0]
                start = rotate_mesh_by_angle(pose, (points,), angles[i:i + 1])[0]
                has = ((face >= 0).reshape(-1, 1)) & (n.abs().sum(dim=1, keepdim=True) > 0)
                shading = torch.where(has, ends - start, f.normals.reshape(-1, 3)).reshape(f.normals.shape).contiguous()
            frames[i] = ops.shade_fragments(f.pix_to_face, f.bary, shading, turned, triangles, lit=lit, **how).image
        return frames

    @_passes_on("normal_map_size", None, "extract_rigged_mesh")
    def extract_rigged_mesh(self, pose_to_camera, z, bone_length, voxel_size=0.003, mesh_th=15, truncation_psi=0.4,
                            max_influences=4, return_colors=False, return_part_labels=False, texture_size=None,
                            texture_color="field", simplify_cell=None):
        """extract_mesh (with its `simplify_cell`) in the rest pose pose_to_camera, bound to the model's parts: a RiggedMesh (mesh_rendering) with
        joints and weights (V, max_influences = 4 or 8) from one launch of the HIP skin-weight kernel, ready for
        render_mesh_animation, mesh_rendering.skin_mesh and mesh_rendering.export_glb; one sample, as extract_mesh.
        `texture_size` adds rig.texture, the texture atlas of the mesh baked in this pose in `texture_color` ("field" or
        "parts"), for render_textured_mesh_animation and a textured export_glb. The keyword `normal_map_size` (_passes_on)
        adds rig.normal_map, the field's normals baked into an atlas of that size for the final (simplified) mesh: the
        animations draw it with normal_map=True, export_glb writes it as the material's normalTexture."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.extract_rigged_mesh(pose_to_camera, z_nerf, z_render, bone_length, voxel_size, mesh_th,
                                             truncation_psi, max_influences, return_colors, return_part_labels,
                                             texture_size, texture_color, simplify_cell)

    def bake_texture(self, pose_to_camera, z, bone_length, vertices, triangles, truncation_psi=0.4, size=1024,
                     color="field", palette=None, color_fn=None, want_float=False):
        """The texture atlas of a mesh extract_mesh returned for the same arguments: a TextureAtlas (mesh_rendering) of
        size x size texels holding the field's colour (color="field") or the part colours (color="parts") at the surface
        point of every texel, from the HIP bake kernels and one query launch a band of rows; one sample."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.bake_texture(pose_to_camera, z_nerf, z_render, bone_length, vertices, triangles, truncation_psi,
                                      size, color, palette, color_fn, want_float)

    def bake_normal_map(self, pose_to_camera, z, bone_length, vertices, triangles, truncation_psi=0.4, size=1024,
                        normal_fn=None, min_gradient=0.0, want_float=False):
        """The tangent-space normal map of a mesh extract_mesh returned for the same arguments: a TextureAtlas
        (mesh_rendering) of size x size texels holding the field's own normal at the surface point of every texel, in the
        frame of the texel's triangle, from the HIP bake, gradient and encode kernels, one launch each a band of rows."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.bake_normal_map(pose_to_camera, z_nerf, z_render, bone_length, vertices, triangles, truncation_psi,
                                         size, normal_fn, min_gradient, want_float)

    def _passes_normals_on(render):
        """Decorator of render_textured_mesh: adds the keyword normals = "mesh" (the method as it stands) or "field", which
        goes to TriPlaneNARF.render_textured_mesh with the method's own arguments. The method keeps its signature."""
        signature = inspect.signature(render)

        @functools.wraps(render)
        def wrapper(self, *args, normals="mesh", **kwargs):
            if normals == "mesh":
                return render(self, *args, **kwargs)
            bound = signature.bind(self, *args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            z_nerf, z_render, _ = self._latent_parts(a["z"])
            return self.nerf.render_textured_mesh(a["pose_to_camera"], a["intrinsics"], z_nerf, z_render, a["bone_length"],
                                                  a["voxel_size"], a["mesh_th"], a["truncation_psi"], self.size,
                                                  a["texture_size"], a["color"], a["lit"], a["simplify_cell"], normals=normals)
        return wrapper

    @_passes_on("normal_map", False, "render_textured_mesh", with_size=True)
    @_passes_normals_on
    def render_textured_mesh(self, pose_to_camera, intrinsics, z, bone_length, voxel_size=0.01, mesh_th=15,
                             truncation_psi=0.4, texture_size=1024, color="field", lit=True, simplify_cell=None):
        """render_colored_mesh with the colour in a texture atlas: a mesh coarse enough for other tools (voxel 0.01) keeps
        the field's colour detail. `simplify_cell` gets the coarse mesh from a fine extraction instead (a smaller
        voxel_size, simplified to cells of simplify_cell). The keyword normals="field" (_passes_normals_on) shades every
        covered pixel with the field's own normal. (image (512, 512, 3) uint8 numpy, (vertices, triangles, the
        TextureAtlas)); one sample."""
        z_nerf, z_render, _ = self._latent_parts(z)
        return self.nerf.render_textured_mesh(pose_to_camera, intrinsics, z_nerf, z_render, bone_length, voxel_size,
                                              mesh_th, truncation_psi, self.size, texture_size, color, lit, simplify_cell)

    del _passes_normals_on                               # a decorator, not a method

    def render_textured_mesh_animation(self, rig, key_poses, bone_length, intrinsics, num=100, loop=True, orbit=None,
                                       lit=True, render_size=512, frames_per_batch=8, normal_map=False):
        """render_mesh_animation drawn with rig.texture (a rig from extract_rigged_mesh(texture_size=...)): (frames
        (num, R, R, 3) uint8, poses (num, J, 4, 4) in key_poses' dtype), device tensors, with no host synchronisation
        inside. One interpolate_pose launch; the frames posed frames_per_batch at a time by one skin_pose launch; every
        frame one rasterize_mesh and one shade_textured: the texture was baked once, in the rest pose, and moves with the
        triangles. The bytes do not depend on frames_per_batch. normal_map=True shades every frame with rig.normal_map (a
        rig from extract_rigged_mesh(normal_map_size=...), the same atlas size as the texture) in place of the face normals:
        one shade_normal_mapped launch a frame instead of the shade_textured one, the map baked once in the rest pose, its
        frame rebuilt from the posed vertices."""
        from .. import ops
        from ..libraries.NARF.mesh_rendering import rasterize_mesh, skin_mesh
        if rig.texture is None:
            raise ValueError("render_textured_mesh_animation takes a rig extracted with texture_size=...")
        if normal_map:
            self._check_normal_map("render_textured_mesh_animation", rig, rig.texture.size)
        if rig.texture.num_triangles != rig.triangles.shape[0]:
            raise ValueError(f"render_textured_mesh_animation: the atlas was baked for {rig.texture.num_triangles} triangles, "
                             f"the rig has {rig.triangles.shape[0]}")
        if bone_length.shape[0] != 1:
            raise AssertionError("render_textured_mesh_animation takes one identity: bone_length of batch 1")
        per = int(frames_per_batch)
        if per < 1:
            raise ValueError(f"render_textured_mesh_animation: frames_per_batch {frames_per_batch} < 1")
        nerf, R = self.nerf, int(render_size)
        with torch.no_grad():
            poses, poses32 = ops.interpolate_pose(key_poses, nerf.parent_id, num, loop, orbit, return_f32=True)
            dev, n_frames, V = poses.device, poses.shape[0], rig.vertices.shape[0]
            frames = torch.empty((n_frames, R, R, 3), dtype=torch.uint8, device=dev)
            posed = torch.empty((min(per, n_frames), V, 3), dtype=torch.float32, device=dev)
            for a in range(0, n_frames, per):
                b = min(a + per, n_frames)
                pose_parts, bl = nerf.transform_pose(poses32[a:b], bone_length.float().expand(b - a, -1, -1))
                skin_mesh(nerf, rig, pose_parts, bl, out=posed[:b - a])
                for i in range(a, b):
                    f = rasterize_mesh(posed[i - a], rig.triangles, intrinsics, self.size, R)
                    if normal_map:
                        frames[i] = ops.shade_normal_mapped(f.pix_to_face, f.bary, f.normals, posed[i - a], rig.triangles,
                                                            rig.normal_map.texture, texture=rig.texture.texture, lit=lit).image
                    else:
                        frames[i] = ops.shade_textured(f.pix_to_face, f.bary, f.normals, posed[i - a], rig.triangles,
                                                       rig.texture.texture, lit=lit).image
        return frames, poses

    @staticmethod
    def _check_normal_map(who, rig, size=None):
        """ValueError unless rig.normal_map is a normal map of the rig's triangles (and of `size` texels a side)"""
        if getattr(rig, "normal_map", None) is None:
            raise ValueError(f"{who}: normal_map=True takes a rig extracted with normal_map_size=...")
        if rig.normal_map.num_triangles != rig.triangles.shape[0]:
            raise ValueError(f"{who}: the normal map was baked for {rig.normal_map.num_triangles} triangles, the rig has "
                             f"{rig.triangles.shape[0]}")
        if size is not None and rig.normal_map.size != size:
            raise ValueError(f"{who}: the normal map has {rig.normal_map.size} texels a side, the texture {size}: bake both at "
                             f"one size")

    def render_mesh_animation(self, rig, key_poses, bone_length, intrinsics, num=100, loop=True, orbit=None, color="field",
                              lit=True, render_size=512, frames_per_batch=8, normal_map=False, base_color=1.0):
        """The rigged mesh in motion, without a new extraction: (frames (num, R, R, 3) uint8, poses (num, J, 4, 4) in
        key_poses' dtype), device tensors, with no host synchronisation inside. One interpolate_pose launch; the frames
        posed frames_per_batch at a time by one skin_pose launch (linear-blend skinning of `rig`, the RiggedMesh of
        extract_rigged_mesh); every frame one rasterize_mesh and one shade_fragments, as render_mesh_turntable.
        color="field" draws rig.colors, "parts" the palette colours of rig.labels, None the white mesh; bone_length
        (1, J - 1, 1) are the bone lengths of the animation (a bone longer than the rig's stretches its part). The bytes
        do not depend on frames_per_batch. normal_map=True with color=None draws the mesh in the constant base_color shaded
        with rig.normal_map (extract_rigged_mesh(normal_map_size=...)): one shade_normal_mapped launch a frame."""
        from .. import ops
        from ..libraries.NARF.mesh_rendering import rasterize_mesh, skin_mesh
        from ..libraries.NeRF.rendering import semantic_palette
        if color not in ("field", "parts", None):
            raise ValueError(f"color is 'field', 'parts' or None (the white mesh), got {color!r}")
        if normal_map:
            if color is not None:
                raise ValueError("render_mesh_animation: normal_map=True draws a constant base_color (color=None); a coloured "
                                 "normal-mapped rig is render_textured_mesh_animation's")
            self._check_normal_map("render_mesh_animation", rig)
        if color == "field" and rig.colors is None or color == "parts" and rig.labels is None:
            raise ValueError(f"color={color!r} takes a rig extracted with "
                             f"{'return_colors' if color == 'field' else 'return_part_labels'}=True")
        if bone_length.shape[0] != 1:
            raise AssertionError("render_mesh_animation takes one identity: bone_length of batch 1")
        per = int(frames_per_batch)
        if per < 1:
            raise ValueError(f"render_mesh_animation: frames_per_batch {frames_per_batch} < 1")
        nerf, R = self.nerf, int(render_size)
        with torch.no_grad():
            poses, poses32 = ops.interpolate_pose(key_poses, nerf.parent_id, num, loop, orbit, return_f32=True)
            dev, n_frames, V = poses.device, poses.shape[0], rig.vertices.shape[0]
            how = {}
            if color == "field":
                how = dict(vertex_colors=rig.colors)
            elif color == "parts":
                how = dict(vertex_labels=rig.labels, palette=(semantic_palette(nerf.num_bone, dev) + 1) / 2)
            frames = torch.empty((n_frames, R, R, 3), dtype=torch.uint8, device=dev)
            posed = torch.empty((min(per, n_frames), V, 3), dtype=torch.float32, device=dev)
            for a in range(0, n_frames, per):
                b = min(a + per, n_frames)
                pose_parts, bl = nerf.transform_pose(poses32[a:b], bone_length.float().expand(b - a, -1, -1))
                skin_mesh(nerf, rig, pose_parts, bl, out=posed[:b - a])
                for i in range(a, b):
                    f = rasterize_mesh(posed[i - a], rig.triangles, intrinsics, self.size, R)
                    if normal_map:
                        frames[i] = ops.shade_normal_mapped(f.pix_to_face, f.bary, f.normals, posed[i - a], rig.triangles,
                                                            rig.normal_map.texture, base_color=base_color, lit=lit).image
                        continue
                    frames[i] = (ops.shade_fragments(f.pix_to_face, f.bary, f.normals, posed[i - a], rig.triangles, lit=lit,
                                                     **how).image if how else f.image)
        return frames, poses

    def render_part_animation(self, key_poses, bone_length, intrinsics, z, num=100, loop=True, orbit=None,
                              truncation_psi=0.4, frames_per_batch=8, background=1.0):
        """render_animation of the part segmentation: (frames (num, S, S, 3) uint8 in the colours of semantic_palette over
        `background` (a number in [-1, 1], white by default), part_maps (num, S, S) int32 - the part that carries the most
        weight along each ray, -1 where none does -, poses (num, J, 4, 4) in key_poses' dtype), all device tensors, with
        no host synchronisation inside. The structure is render_animation's: one interpolate_pose launch, one tri-plane,
        the frames marched frames_per_batch at a time through render(..., semantic_map=True), each chunk turned into
        bytes by one compose_frames launch; frames_per_batch=1 gives the bytes of one render() call per frame."""
        from .. import ops
        from ..libraries.NeRF.rendering import render
        if not (z.shape[0] == 1 and bone_length.shape[0] == 1):
            raise AssertionError("render_part_animation takes one identity: z and bone_length of batch 1")
        per = int(frames_per_batch)
        if per < 1:
            raise ValueError(f"render_part_animation: frames_per_batch {frames_per_batch} < 1")
        nerf, S = self.nerf, self.size
        with torch.no_grad():
            poses, poses32 = ops.interpolate_pose(key_poses, nerf.parent_id, num, loop, orbit, return_f32=True)
            dev, n_frames = poses.device, poses.shape[0]
            z_nerf, z_render, _ = self._latent_parts(z)
            tri = nerf.compute_tri_plane_feature(z_nerf, bone_length, truncation_psi)
            K_inv = torch.linalg.inv_ex(torch.as_tensor(intrinsics).float().to(dev).reshape(-1, 3, 3)[:1]).inverse
            _, pixels = self.ray_sampler(S, S, min(per, n_frames), device=dev)
            frames = torch.empty((n_frames, S, S, 3), dtype=torch.uint8, device=dev)
            part_maps = torch.empty((n_frames, S, S), dtype=torch.int32, device=dev)
            mlp = nerf.mlp.as_dict()
            for a in range(0, n_frames, per):
                b = min(a + per, n_frames)
                c = b - a
                bl, z_rend = bone_length.expand(c, -1, -1), z_render.expand(c, -1)
                parts, pack = ops.prepare(poses32[a:b], bl, nerf.canonical_bone_length, z_rend, mlp, nerf.parent_id,
                                          nerf.origin_location, nerf.coordinate_scale)
                model_input = {"z": z_nerf, "z_rend": z_rend, "bone_length": bl, "truncation_psi": truncation_psi,
                               "tri_plane_feature": tri}
                color, alpha, _ = render(nerf, pixels[:c], poses32.new_empty(c, nerf.num_bone, 4, 4), K_inv.expand(c, -1, -1),
                                         semantic_map=True, model_input=model_input, _parts=parts, _pack=pack,
                                         **self._samples)
                ops.compose_frames(color, alpha, background, return_masks=False, out=(frames[a:b], None))
                part_maps[a:b] = nerf.buffers_tensors["part_map"].reshape(c, S, S)
        return frames, part_maps, poses

    def render_geometry_animation(self, key_poses, bone_length, intrinsics, z, num=100, loop=True, orbit=None,
                                  truncation_psi=0.4, frames_per_batch=8, background=1.0, shade="normal",
                                  normals="stencil", **buffer_kwargs):
        """render_animation of the geometry: (frames (num, S, S, 3) uint8 - the shape image of ops.geometry_buffers in
        `shade` over `background` -, depth (num, S, S) fp32 in metric units, poses (num, J, 4, 4) in key_poses' dtype), all
        device tensors, with no host synchronisation inside. The structure is render_part_animation's: one
        interpolate_pose launch, one tri-plane, the frames marched frames_per_batch at a time, each chunk turned into
        bytes and depths by one geometry_buffers launch that writes into frames[a:b] and depth[a:b]; frames_per_batch=1
        gives the bytes of render_geometry on one frame. buffer_kwargs go to ops.geometry_buffers (edge, mask_threshold,
        near, far, ...), except `want` and `out`, which this function sets itself: passing either raises ValueError.
        normals="field" shades the frames with the field's own normals (render_geometry's keyword: a gradient launch and a
        ray-normal launch a chunk more, the image copied into frames[a:b])."""
        from .. import ops
        from ..libraries.NeRF.rendering import render
        taken = sorted(k for k in ("want", "out") if k in buffer_kwargs)
        if taken:
            raise ValueError(f"render_geometry_animation writes image and depth into its own tensors: {', '.join(taken)} "
                             "cannot be passed")
        if normals not in ("stencil", "field"):
            raise ValueError(f"normals is 'stencil' or 'field', got {normals!r}")
        if not (z.shape[0] == 1 and bone_length.shape[0] == 1):
            raise AssertionError("render_geometry_animation takes one identity: z and bone_length of batch 1")
        per = int(frames_per_batch)
        if per < 1:
            raise ValueError(f"render_geometry_animation: frames_per_batch {frames_per_batch} < 1")
        nerf, S = self.nerf, self.size
        with torch.no_grad():
            poses, poses32 = ops.interpolate_pose(key_poses, nerf.parent_id, num, loop, orbit, return_f32=True)
            dev, n_frames = poses.device, poses.shape[0]
            z_nerf, z_render, _ = self._latent_parts(z)
            tri = nerf.compute_tri_plane_feature(z_nerf, bone_length, truncation_psi)
            K_inv = torch.linalg.inv_ex(torch.as_tensor(intrinsics).float().to(dev).reshape(-1, 3, 3)[:1]).inverse
            _, pixels = self.ray_sampler(S, S, min(per, n_frames), device=dev)
            frames = torch.empty((n_frames, S, S, 3), dtype=torch.uint8, device=dev)
            depth = torch.empty((n_frames, S, S), dtype=torch.float32, device=dev)
            mlp = nerf.mlp.as_dict()
            for a in range(0, n_frames, per):
                b = min(a + per, n_frames)
                c = b - a
                bl, z_rend = bone_length.expand(c, -1, -1), z_render.expand(c, -1)
                parts, pack = ops.prepare(poses32[a:b], bl, nerf.canonical_bone_length, z_rend, mlp, nerf.parent_id,
                                          nerf.origin_location, nerf.coordinate_scale)
                model_input = {"z": z_nerf, "z_rend": z_rend, "bone_length": bl, "truncation_psi": truncation_psi,
                               "tri_plane_feature": tri}
                if normals == "field":
                    buffers, _, _ = nerf.field_geometry(pixels[:c], K_inv.expand(c, -1, -1), parts, pack, model_input, (S, S),
                                                        self._samples["Nc"], self._samples["Nf"], shade,
                                                        background=background, **buffer_kwargs)
                    frames[a:b], depth[a:b] = buffers.image, buffers.depth
                    continue
                _, alpha, disparity = render(nerf, pixels[:c], poses32.new_empty(c, nerf.num_bone, 4, 4),
                                             K_inv.expand(c, -1, -1), model_input=model_input, _parts=parts, _pack=pack,
                                             **self._samples)
                ops.geometry_buffers(disparity * nerf.coordinate_scale, alpha, K_inv, size=(S, S), shade=shade,
                                     background=background, want=("depth", "image"),
                                     out={"image": frames[a:b], "depth": depth[a:b]}, **buffer_kwargs)
        return frames, depth, poses

    def render_animation(self, key_poses, bone_length, intrinsics, z, num=100, loop=True, orbit=None, truncation_psi=0.4,
                         frames_per_batch=8, black_bg_if_possible=False):
        """One identity in motion, on the device from end to end: (frames (num, S, S, 3) uint8, masks (num, S, S) uint8,
        poses (num, J, 4, 4) in key_poses' dtype), all device tensors, with no host synchronisation inside.

        key_poses (K, J, 4, 4) joint-to-camera key poses on the device; z and bone_length of batch 1; intrinsics (3, 3)
        or (1, 3, 3); num, loop and orbit as in ops.interpolate_pose (orbit: num angles on the device, a turntable). The
        poses come from one interpolate_pose launch, the tri-plane and the background are computed once, and the frames
        are marched frames_per_batch at a time on the shared tri-plane (render() with the tri-plane in model_input,
        under no_grad), each chunk turned into bytes by one compose_frames launch. A chunk is one renderer batch: its
        near / far planes are reduced over its frames and its rays are numbered batch-wide for the importance samples,
        as in a forward() call on the chunk's frames. The bytes therefore depend on frames_per_batch (in the last bits
        of the march): frames_per_batch=1 gives exactly the bytes of one forward() call per frame."""
        from .. import ops
        from ..libraries.NeRF.rendering import render
        if not (z.shape[0] == 1 and bone_length.shape[0] == 1):
            raise AssertionError("render_animation takes one identity: z and bone_length of batch 1")
        per = int(frames_per_batch)
        if per < 1:
            raise ValueError(f"render_animation: frames_per_batch {frames_per_batch} < 1")
        nerf, S = self.nerf, self.size
        with torch.no_grad():
            poses, poses32 = ops.interpolate_pose(key_poses, nerf.parent_id, num, loop, orbit, return_f32=True)
            dev, n_frames = poses.device, poses.shape[0]
            z_nerf, z_render, z_bg = self._latent_parts(z)
            tri = nerf.compute_tri_plane_feature(z_nerf, bone_length, truncation_psi)
            backdrop = self._background(z_bg, z_render, black_bg_if_possible)
            K_inv = torch.linalg.inv_ex(torch.as_tensor(intrinsics).float().to(dev).reshape(-1, 3, 3)[:1]).inverse
            _, pixels = self.ray_sampler(S, S, min(per, n_frames), device=dev)
            frames = torch.empty((n_frames, S, S, 3), dtype=torch.uint8, device=dev)
            masks = torch.empty((n_frames, S, S), dtype=torch.uint8, device=dev)
            mlp = nerf.mlp.as_dict()
            for a in range(0, n_frames, per):
                b = min(a + per, n_frames)
                c = b - a
                bl, z_rend = bone_length.expand(c, -1, -1), z_render.expand(c, -1)
                parts, pack = ops.prepare(poses32[a:b], bl, nerf.canonical_bone_length, z_rend, mlp, nerf.parent_id,
                                          nerf.origin_location, nerf.coordinate_scale)
                model_input = {"z": z_nerf, "z_rend": z_rend, "bone_length": bl, "truncation_psi": truncation_psi,
                               "tri_plane_feature": tri}
                color, alpha, _ = render(nerf, pixels[:c], poses32.new_empty(c, nerf.num_bone, 4, 4), K_inv.expand(c, -1, -1),
                                         model_input=model_input, _parts=parts, _pack=pack, **self._samples)
                ops.compose_frames(color, alpha, backdrop, out=(frames[a:b], masks[a:b]))
        return frames, masks, poses

    def _scene_backdrop(self, background, z_bg, z_render, device):
        """The one background of a scene: "first" runs the background network on the first avatar's latents (-1 on a
        generator with a black background), a (1, 3, S, S) tensor is taken as it is, a number is a flat colour (-1: black)."""
        S = self.size
        if isinstance(background, str):
            if background != "first":
                raise ValueError(f"render_scene: background {background!r} is neither 'first', a (1, 3, {S}, {S}) tensor nor a number")
            return self._background(None if z_bg is None else z_bg[:1], z_render[:1], False)
        if isinstance(background, torch.Tensor):
            if tuple(background.shape) != (1, 3, S, S):
                raise ValueError(f"render_scene: a background image is (1, 3, {S}, {S}), got {tuple(background.shape)}")
            return background.to(device=device, dtype=torch.float32)
        try:
            return float(background)
        except (TypeError, ValueError):
            raise ValueError(f"render_scene: background {background!r} is neither 'first', a (1, 3, {S}, {S}) tensor nor a "
                             "number") from None

    @staticmethod
    def _instance_image(instance, K):
        """(F, S, S) int32 avatar indices -> (F, 3, S, S) fp32 in the colours of semantic_palette(K), white where no avatar
        owns the pixel"""
        from ..libraries.NeRF.rendering import semantic_palette
        palette = semantic_palette(K, instance.device)
        rgb = torch.where(instance[..., None] >= 0, palette[instance.clamp(min=0).long()], palette.new_ones(()))
        return rgb.permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def render_scene(self, pose_to_camera, bone_length, z, inv_intrinsics, truncation_psi=1, background="first",
                     return_instances=False, avatars_per_batch=None, return_bg=False, threshold=0.5, seed=None):
        """K identities in K poses in front of one camera, in one image: pose_to_camera (K, J, 4, 4), bone_length and z of
        batch K, one inv_intrinsics -> (image (1, 3, S, S), mask (1, S, S)); with return_instances also (instance map
        (1, S, S) int32 - the avatar that carries the largest share of the pixel's mask, -1 where the mask is below
        `threshold` -, its colour image (1, 3, S, S) in semantic_palette(K), white without an avatar). The avatars are
        marched on the same rays and composed by rendering.render_scene (one ops.scene_composite launch: depth-correct
        where bodies interleave, avatars_per_batch as there); image = colour + (1 - mask) background as forward()
        composes it, the background as _scene_backdrop takes it ("first": the background network on the first avatar's
        latents). return_bg returns (colour, mask, background) uncomposed, as forward(return_bg=True). The shares are
        left in self.nerf.buffers_tensors (instance_mass, skipped, avatar_masks). All on the device, no host
        synchronisation inside (a `seed` of None draws one from torch's CPU generator, as render() does)."""
        from .. import ops
        from ..libraries.NeRF.rendering import render_scene
        nerf, S, K = self.nerf, self.size, pose_to_camera.shape[0]
        if not (z.shape[0] == K and bone_length.shape[0] == K):
            raise AssertionError(f"render_scene takes z and bone_length of batch K = {K}, one entry an avatar")
        dev = pose_to_camera.device
        _, pixels = self.ray_sampler(S, S, 1, device=dev)
        z_nerf, z_render, z_bg = self._latent_parts(z)
        K_inv = torch.as_tensor(inv_intrinsics).float().to(dev)
        parts, pack = ops.prepare(pose_to_camera, bone_length, nerf.canonical_bone_length, z_render, nerf.mlp.as_dict(),
                                  nerf.parent_id, nerf.origin_location, nerf.coordinate_scale)
        model_input = {"z": z_nerf, "z_rend": z_render, "bone_length": bone_length, "truncation_psi": truncation_psi}
        color, mask, _ = render_scene(nerf, pixels, pose_to_camera.new_empty(K, nerf.num_bone, 4, 4), K_inv,
                                      model_input=model_input, avatars_per_batch=avatars_per_batch, seed=seed,
                                      threshold=threshold, _parts=parts, _pack=pack, **self._samples)
        person, alpha = color.reshape(1, 3, S, S), mask.reshape(1, S, S)
        backdrop = self._scene_backdrop(background, z_bg, z_render, dev)
        if return_bg:
            return person, alpha, backdrop
        image = person + (1 - alpha[:, None]) * backdrop
        if not return_instances:
            return image, alpha
        instance = nerf.buffers_tensors["instance"].reshape(1, S, S)
        return image, alpha, instance, self._instance_image(instance, K)

    def render_scene_posable(self, pose_to_camera, bone_length, z, inv_intrinsics, truncation_psi=1, background="first",
                             pixels=None, avatars_per_batch=None, seed=None):
        """render_scene for poses that require gradients: pose_to_camera (K, J, 4, 4) and bone_length may require them and
        receive the gradient of the image at fixed sample positions (rendering.render_scene_posable: the HIP pose
        gradient of every avatar's query, the HIP backward of the composite). `pixels` (1, 1, 3, n) names the rays
        (default: the whole S x S frame, n = S S) -> (image (1, 3, n), mask (1, n)), image = colour + (1 - mask)
        background. On the whole frame the background is _scene_backdrop's; on given pixels it is a number or a
        (1, 3, n) tensor, one colour a ray. instance_mass (differentiable), instance and skipped are left in
        self.nerf.buffers_tensors. The tri-planes are produced once, for the march and the query alike."""
        from ..libraries.NeRF.rendering import render_scene_posable
        nerf, S, K = self.nerf, self.size, pose_to_camera.shape[0]
        if not (z.shape[0] == K and bone_length.shape[0] == K):
            raise AssertionError(f"render_scene_posable takes z and bone_length of batch K = {K}, one entry an avatar")
        dev = pose_to_camera.device
        whole = pixels is None
        if whole:
            _, pixels = self.ray_sampler(S, S, 1, device=dev)
        z_nerf, z_render, z_bg = self._latent_parts(z)
        K_inv = torch.as_tensor(inv_intrinsics).float().to(dev)
        pose_parts, bl_parts = nerf.transform_pose(pose_to_camera, bone_length)
        model_input = {"z": z_nerf, "z_rend": z_render, "bone_length": bl_parts, "truncation_psi": truncation_psi}
        if not (nerf.uses_warp or nerf.constant_trimask):
            model_input["tri_plane_feature"] = nerf.compute_tri_plane_feature(z_nerf, bl_parts, truncation_psi)
        color, mask, _ = render_scene_posable(nerf, pixels, pose_parts, K_inv, model_input=model_input,
                                              avatars_per_batch=avatars_per_batch, seed=seed, **self._samples)
        if isinstance(background, torch.Tensor) and not whole:
            if tuple(background.shape) != tuple(color.shape):
                raise ValueError(f"render_scene_posable: a background on given pixels is {tuple(color.shape)}, got "
                                 f"{tuple(background.shape)}")
            backdrop = background.to(device=dev, dtype=torch.float32)
        elif isinstance(background, str) and not whole:
            raise ValueError("render_scene_posable: background 'first' needs the whole frame; pass a number or a (1, 3, n) tensor")
        else:
            backdrop = self._scene_backdrop(background, z_bg, z_render, dev)
            if isinstance(backdrop, torch.Tensor):
                backdrop = backdrop.reshape(1, 3, S * S)
        return color + (1 - mask[:, None]) * backdrop, mask

    def render_scene_animation(self, key_poses, bone_length, intrinsics, z, num=100, loop=True, orbit=None, truncation_psi=0.4,
                               frames_per_batch=8, background="first", threshold=0.5):
        """K identities in motion in front of one camera, on the device from end to end: (frames (num, S, S, 3) uint8,
        masks (num, S, S) uint8, instances (num, S, S) int32, poses (K, num, J, 4, 4) in key_poses' dtype), all device
        tensors, with no host synchronisation inside.

        key_poses (K, Kp, J, 4, 4), or a list of K (Kp, J, 4, 4) tensors, joint-to-camera key poses on the device; z and
        bone_length of batch K; intrinsics (3, 3) or (1, 3, 3); num, loop and orbit as in ops.interpolate_pose, one
        launch an avatar. The tri-plane of every avatar and the background are computed once. The frames are marched
        frames_per_batch at a time, avatar by avatar on its own tri-plane (a renderer batch is one avatar in the
        chunk's frames, every avatar on the chunk's one seed), and each chunk takes one ops.scene_composite launch and one
        ops.compose_frames launch. frames_per_batch=1 gives the bytes of render_scene(avatars_per_batch=1) on each
        frame's poses."""
        from .. import ops
        from ..libraries.NeRF.rendering import _march_taps, composite_marches
        K = len(key_poses)
        if not (z.shape[0] == K and bone_length.shape[0] == K):
            raise AssertionError(f"render_scene_animation takes z and bone_length of batch K = {K}, one entry an avatar")
        per = int(frames_per_batch)
        if per < 1:
            raise ValueError(f"render_scene_animation: frames_per_batch {frames_per_batch} < 1")
        nerf, S = self.nerf, self.size
        with torch.no_grad():
            both = [ops.interpolate_pose(key_poses[k], nerf.parent_id, num, loop, orbit, return_f32=True) for k in range(K)]
            poses = torch.stack([p for p, _ in both])
            dev, n_frames = poses.device, poses.shape[1]
            z_nerf, z_render, z_bg = self._latent_parts(z)
            tri = [nerf.compute_tri_plane_feature(z_nerf[k:k + 1], bone_length[k:k + 1], truncation_psi).detach().contiguous()
                   for k in range(K)]
            feat = [ops.triplane_pack(t) for t in tri]
            backdrop = self._scene_backdrop(background, z_bg, z_render, dev)
            K_inv = torch.linalg.inv_ex(torch.as_tensor(intrinsics).float().to(dev).reshape(-1, 3, 3)[:1]).inverse
            _, pixels = self.ray_sampler(S, S, 1, device=dev)
            frames = torch.empty((n_frames, S, S, 3), dtype=torch.uint8, device=dev)
            masks = torch.empty((n_frames, S, S), dtype=torch.uint8, device=dev)
            instances = torch.empty((n_frames, S, S), dtype=torch.int32, device=dev)
            mlp, flags = nerf.mlp.as_dict(), nerf.kernel_flags()
            for a in range(0, n_frames, per):
                b = min(a + per, n_frames)
                c = b - a
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                marches = []
                for k in range(K):
                    bl, z_rend = bone_length[k:k + 1].expand(c, -1, -1), z_render[k:k + 1].expand(c, -1)
                    parts, pack = ops.prepare(both[k][1][a:b], bl, nerf.canonical_bone_length, z_rend, mlp, nerf.parent_id,
                                              nerf.origin_location, nerf.coordinate_scale)
                    marches.append(_march_taps(nerf, pixels, K_inv, parts, tri[k], feat[k], pack, self._samples["Nc"],
                                               self._samples["Nf"], 1, seed, flags))
                color, alpha, _ = composite_marches(nerf, marches, 1, 1, threshold)
                ops.compose_frames(color, alpha, backdrop, out=(frames[a:b], masks[a:b]))
                instances[a:b] = nerf.buffers_tensors["instance"].reshape(c, S, S)
        return frames, masks, instances, poses


class DSONARFGenerator(_RendererShell):
    def __init__(self, config, size, num_bone=1, parent_id=None, num_bone_param=None):
        if not config.use_triplane:
            raise NotImplementedError("MLPNARF (use_triplane: False) is not the tri-plane path (SURVEY.md §2, OUT)")
        params = config.nerf_params
        latent = (20 if params.time_conditional else 0) + (9 * (num_bone - 1) if params.pose_conditional else 0)
        super().__init__(config, size, num_bone, parent_id, num_bone_param, z_dim=latent,
                         view_dependent=not params.no_ray_direction)
        self.ray_sampler = mask_based_sampler
        self.time_conditional, self.pose_conditional = params.time_conditional, params.pose_conditional

    @staticmethod
    def positional_encoding(x: torch.Tensor, num_frequency: int) -> torch.Tensor:
        """(B,) -> (B, 2 F): cos then sin of x * 2^f * pi."""
        octaves = torch.exp2(torch.arange(num_frequency, device=x.device).float())
        phase = x[:, None] * octaves * np.pi          # (x 2^f) pi, in this order
        return torch.cat([phase.cos(), phase.sin()], dim=1)

    @staticmethod
    def pose_encoding(pose: torch.Tensor):
        """Joint rotations relative to the root, flattened: (B, J, 4, 4) -> (B, 9 (J - 1))."""
        root_T = pose[:, :1, :3, :3].transpose(-1, -2)
        return (root_T @ pose[:, 1:, :3, :3]).flatten(1)

    def get_latents(self, frame_time: torch.Tensor, pose_to_camera: torch.Tensor):
        codes = []
        if self.time_conditional:
            codes.append(self.positional_encoding(frame_time, num_frequency=10))
        if self.pose_conditional:
            codes.append(self.pose_encoding(pose_to_camera))
        if not codes:
            raise AssertionError("neither time_conditional nor pose_conditional")
        z = torch.cat(codes, dim=1)
        return z, z

    def forward(self, pose_to_camera, camera_pose, mask, frame_time, bone_length, inv_intrinsics,
                background: Optional[float] = None):
        if bone_length is None or pose_to_camera is None or not isinstance(inv_intrinsics, torch.Tensor):
            raise AssertionError("bone_length, pose_to_camera and a tensor inv_intrinsics are required")
        ray_idx, pixels = self.ray_sampler(mask, self.config.ray_batchsize)
        z_tri, z_render = self.get_latents(frame_time, pose_to_camera)
        color, alpha = self.nerf(pose_to_camera.shape[0], pixels, pose_to_camera, inv_intrinsics, z_tri, z_render,
                                 bone_length, return_intermediate=False, camera_pose=camera_pose, **self._samples)
        backdrop = -1 if background is None else background
        return color + backdrop * (1 - alpha[:, None]), alpha, ray_idx

    def render_geometry(self, pose_to_camera, inv_intrinsics, frame_time, bone_length, camera_pose=None, render_size=128,
                        shade="normal", bbox=None, **buffer_kwargs):
        """The geometry of the frames render_entire_img renders, for every image of the batch: (image (B, H, W, 3) uint8,
        the GeometryBuffers of ops.geometry_buffers, colour (B, 3, H, W), mask (B, H, W)) with (H, W) = render_size squared
        or the rectangle bbox = (x0, y0, x1, y1); inv_intrinsics in pixels of the full frame. One march and one launch
        more, no host synchronisation inside; depth and points are metric, in the space of pose_to_camera."""
        z_tri, z_render = self.get_latents(frame_time, pose_to_camera)
        size, origin = (render_size, render_size), (0, 0)
        if bbox is not None:
            size, origin = (bbox[3] - bbox[1], bbox[2] - bbox[0]), (bbox[0], bbox[1])
        return self.nerf.render_geometry(pose_to_camera, inv_intrinsics, z_tri, z_render, bone_length, size, shade=shade,
                                         origin=origin, camera_pose=camera_pose, **self._samples, **buffer_kwargs)

    def render_entire_img(self, pose_to_camera, inv_intrinsics, frame_time, bone_length, camera_pose=None,
                          render_size=128, semantic_map=False, use_normalized_intrinsics=False, no_grad=True, bbox=None):
        z_tri, z_render = self.get_latents(frame_time, pose_to_camera)
        s = self._samples
        return self.nerf.render_entire_img(pose_to_camera, inv_intrinsics, z_tri, z_render, bone_length, camera_pose,
                                           render_size, s["Nc"], s["Nf"], semantic_map, use_normalized_intrinsics,
                                           no_grad=no_grad, bbox=bbox)
