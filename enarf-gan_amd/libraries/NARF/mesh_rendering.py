"""Density sweep behind `create_mesh` (libraries/NARF/mesh_rendering.py:50-81 of the reference).

The reference builds the (2/voxel_size + 1)^3 grid on the host, pushes it through
`calc_density_and_color_from_camera_coord_v2` in `render_bs` chunks and hands the volume to `mcubes`. Here the lattice
is generated inside `enarf_query_fwd` (lattice mode, density only, one launch; or chunk by chunk from device tensors when
`chunk` is given); the volume stays on the device. `create_mesh` keeps the reference's third-party stages (`mcubes`,
`pytorch3d`) and raises ImportError where the reference would. `extract_mesh` is the same mesh built on the device:
`density_volume` -> `marching_cubes` (libenarf_mesh.so) -> the reference's transform; `export_obj` writes it out.
`rasterize_mesh` is `render_mesh_`'s hard-Phong image of such a mesh, rendered on the device (libenarf_raster.so);
`render_mesh_` itself keeps pytorch3d. `vertex_colors` is the radiance field's colour at the vertices, `paint_mesh` the
image of the mesh in those colours or in the colours of its part labels (rasterize_mesh, then the deferred shading of
libenarf_paint.so); `export_obj` and `export_ply` carry the colours and labels out. `extract_rigged_mesh` binds such a mesh
to the model's parts (a `RiggedMesh`: extract_mesh plus one skin-weight launch of libenarf_skin.so), `skin_mesh` poses it by
linear-blend skinning without a new extraction, and `export_glb` writes it as a skinned binary glTF. `bake_texture` gives a
mesh a texture atlas of the field's colour (a `TextureAtlas`: libenarf_bake.so for the texel points and the texture, the
query kernel for the colours), `paint_textured_mesh` draws the mesh with it, and `export_glb` embeds it and animation clips.
`simplify_mesh` makes a finely extracted mesh small (vertex clustering with quadric placement, libenarf_simp.so);
`simplify_cell` on extract_mesh and extract_rigged_mesh does it straight after marching cubes, so that labels, colours, skin
weights and the texture are computed on the small mesh.
"""
from __future__ import annotations

import dataclasses
import functools
import inspect
from typing import Dict, Optional

import torch

from ... import ops
from ... import _mesh_lib
from ... import _raster_lib


def _grid_chunk(D: int, start: int, stop: int, center: torch.Tensor, scale: float, dev: torch.device) -> torch.Tensor:
    """Points [start, stop) of stack(meshgrid(bins, bins, bins)).reshape(1, 3, -1), bins = arange(-c, c + 1) / c."""
    c = (D - 1) // 2
    idx = torch.arange(start, stop, device=dev, dtype=torch.int64)
    ix = torch.div(idx, D * D, rounding_mode="floor")
    iy = torch.div(idx, D, rounding_mode="floor") % D
    iz = idx % D
    p = torch.stack([ix, iy, iz], dim=0).to(torch.float32)
    p = (p - c) / c                                           # == torch.arange(-c, c + 1) / c, elementwise
    return ((p[None] + center.to(dev).reshape(1, 3, 1)) * scale).contiguous()


@torch.no_grad()
def density_volume(model, pose_to_camera: torch.Tensor, center: torch.Tensor, voxel_size: float = 0.003,
                   model_input: Dict = {}, chunk: int = 1 << 31) -> torch.Tensor:
    """(D, D, D) density grid, D = 2 * int(1 / voxel_size) + 1, exactly the tensor the reference feeds to marching
    cubes. pose_to_camera (1, P, 4, 4): part frames with UNSCALED translation (scaled here, on a copy - the reference
    scales its argument in place)."""
    cube = int(1 / voxel_size)
    D = 2 * cube + 1
    dev = pose_to_camera.device
    pose = pose_to_camera.clone()
    if model.coordinate_scale != 1:
        pose[:, :, :3, 3] *= model.coordinate_scale
    B, P = pose.shape[:2]
    assert B == 1, "create_mesh sweeps one pose"
    parts = torch.zeros(B, P, 16, dtype=torch.float32, device=dev)
    parts[:, :, :9] = pose[:, :, :3, :3].reshape(B, P, 9)
    parts[:, :, 9:12] = pose[:, :, :3, 3]
    parts[:, :, 12] = (model.canonical_bone_length[:, None] / model_input["bone_length"] / model.coordinate_scale)[:, :, 0]
    tri, feat_cl = model._tri_plane_pair(model_input)
    pack = model._mlp_pack(model_input["z_rend"])
    flags = model.kernel_flags()
    total = D * D * D
    if chunk >= total and total < 2 ** 31:          # one launch, the lattice generated in the kernel (no point tensor)
        den, _ = ops.query_fwd(None, parts, model.canonical_pose, tri, feat_cl, pack, mlp_mode=model.mlp_mode,
                               need_color=False, **flags,
                               grid=(D, center.reshape(3).tolist(), float(model.coordinate_scale)))
        return den.reshape(D, D, D)
    out = torch.empty(total, dtype=torch.float32, device=dev)
    for s in range(0, total, chunk):
        e = min(s + chunk, total)
        pts = _grid_chunk(D, s, e, center, float(model.coordinate_scale), dev)
        den, _ = ops.query_fwd(pts, parts, model.canonical_pose, tri, feat_cl, pack, mlp_mode=model.mlp_mode,
                               need_color=False, **flags)
        out[s:e] = den.reshape(-1)
    return out.reshape(D, D, D)


def create_mesh(model, pose_to_camera, center, voxel_size=0.003, mesh_th=15, model_input={}):
    """mesh_rendering.py:50-81: density sweep + marching cubes -> (vertices, triangles, textures). The third-party
    imports come first, as in the reference (:52 and the module imports), so a missing PyMCubes / pytorch3d fails
    before any GPU work; `density_volume` is the sweep on its own."""
    try:
        import mcubes
        from pytorch3d.renderer import Textures
    except ImportError as e:      # same third-party requirements as the reference
        raise ImportError("create_mesh needs PyMCubes and pytorch3d (as the reference does); the density grid itself "
                          "is available from density_volume()") from e
    density = density_volume(model, pose_to_camera, center, voxel_size, model_input)
    cube = int(1 / voxel_size)
    dev = pose_to_camera.device
    vertices, triangles = mcubes.marching_cubes(density.cpu().numpy(), mesh_th)
    vertices = torch.tensor((vertices - cube) * voxel_size, device=dev).float() + center[:, :, 0]
    triangles = torch.tensor(triangles.astype("int64")).to(dev)
    return vertices, triangles, Textures(verts_rgb=torch.ones_like(vertices)[None])


def marching_cubes(volume: torch.Tensor, isovalue: float):
    """Marching cubes on the device (libenarf_mesh.so), same argument order as `mcubes.marching_cubes`.

    volume: contiguous fp32 (X, Y, Z) device tensor, X, Y, Z >= 2 and X*Y*Z < 2^31. Returns (vertices (V, 3) fp32 in
    index units, triangles (T, 3) int64) on the same device. A lattice point is inside iff its value > isovalue (NaN is
    outside). One vertex per crossing lattice edge (p, p + e_a), at p + t e_a with t = (iso - v[p]) / (v[p + e_a] - v[p])
    in fp32 (PyMCubes' interpolation), ordered by p's C-order index and then by a; triangles are ordered by cube (C order)
    and then by the case table, and (v1 - v0) x (v2 - v0) points from inside to outside (toward lower values).

    The table (csrc/enarf_mc_table.h, generated by tools/gen_mc_table.py) is face-consistent, so the surface has no
    cracks. It differs from PyMCubes' classic Lorensen table only in cubes with an ambiguous face: the vertex set is the
    same, the triangles there may differ, and PyMCubes' exact triangle order is not reproduced. No CPU fallback."""
    return _mesh_lib.marching_cubes(volume, isovalue)


@torch.no_grad()
def point_part_labels(model, pose_to_camera: torch.Tensor, points: torch.Tensor, model_input: Dict = {},
                      points_last: bool = False, return_valid_bits: bool = False):
    """The part that owns each point (ops.part_labels: label, top, second[, valid_bits], each (B, M)). points (B, 3, M),
    or with `points_last` (M, 3) / (B, M, 3), in camera coordinates; pose_to_camera (B, P, 4, 4) part frames with
    UNSCALED translation, as for density_volume. One launch; the tri-plane is the one the density sweep reads."""
    from ..NeRF.rendering import _parts_from_part_poses
    parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"])
    tri = _mask_tri_plane(model, model_input)
    cs = model.coordinate_scale
    flags = model.kernel_flags()
    return ops.part_labels(points.float() * cs if cs != 1 else points.float(), parts, model.canonical_pose, tri,
                           clamp_mask=flags["clamp_mask"], uniform_part_weight=flags["uniform_part_weight"],
                           points_last=points_last, return_valid_bits=return_valid_bits)


@torch.no_grad()
def vertex_colors(model, pose_to_camera: torch.Tensor, vertices: torch.Tensor, model_input: Dict = {}) -> torch.Tensor:
    """(V, 3) fp32 in [0, 1]: (the radiance field's colour + 1) / 2 at vertices (V, 3) in camera coordinates. The field is
    view-independent on the shipped path (no_ray_direction), so a surface point has one colour. One ops.query_fwd launch
    over the vertex array; pose_to_camera (1, P, 4, 4) part frames with UNSCALED translation, as for point_part_labels."""
    from ..NeRF.rendering import _parts_from_part_poses
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertex_colors takes (V, 3) vertices, got {tuple(vertices.shape)}")
    parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"])
    tri, feat_cl = model._tri_plane_pair(model_input)
    pack = model._mlp_pack(model_input["z_rend"])
    cs = model.coordinate_scale
    points = (vertices.float() * cs if cs != 1 else vertices.float()).t()[None].contiguous()
    _, color = ops.query_fwd(points, parts, model.canonical_pose, tri, feat_cl, pack, mlp_mode=model.mlp_mode,
                             need_color=True, **model.kernel_flags())
    return ((color[0] + 1) / 2).t().contiguous()


@torch.no_grad()
def field_normals(model, pose_to_camera: torch.Tensor, points: torch.Tensor, model_input: Dict = {},
                  fallback: Optional[torch.Tensor] = None, min_gradient: float = 0.0) -> torch.Tensor:
    """(N, 3) fp32 unit normals of the field at points (N, 3) in camera coordinates: -grad(density) / |grad(density)|, the
    density growing into the body. Where |grad| <= min_gradient (the scaled space's units; outside every cube and where
    the density head is off the gradient is an exact zero) the point takes `fallback` (N, 3) as given, or zeros. One
    ops.field_gradient launch over the point array; pose_to_camera (1, P, 4, 4) part frames with UNSCALED translation, as
    for vertex_colors. The scale between camera and scaled space is uniform, so the direction is that of either."""
    from ..NeRF.rendering import _parts_from_part_poses
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"field_normals takes (N, 3) points, got {tuple(points.shape)}")
    if fallback is not None and tuple(fallback.shape) != tuple(points.shape):
        raise ValueError(f"field_normals takes a fallback of the points' shape {tuple(points.shape)}, got {tuple(fallback.shape)}")
    parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"])
    tri, feat_cl = model._tri_plane_pair(model_input)
    pack = model._mlp_pack(model_input["z_rend"])
    cs = model.coordinate_scale
    scaled = (points.float() * cs if cs != 1 else points.float()).t()[None].contiguous()
    _, gradient = ops.field_gradient(scaled, parts, model.canonical_pose, tri, feat_cl, pack, **model.kernel_flags())
    g = gradient[0].t()
    m = torch.linalg.vector_norm(g, dim=1, keepdim=True)
    has = (m > min_gradient) & torch.isfinite(m)
    other = torch.zeros_like(g) if fallback is None else fallback.to(g.dtype)
    return torch.where(has, -g / torch.where(has, m, torch.ones_like(m)), other).contiguous()


def pixel_field_normals(fragments, vertices: torch.Tensor, triangles: torch.Tensor, field) -> torch.Tensor:
    """The (R, R, 3) normal buffer of paint_mesh(normals="field"): the surface point of every covered pixel, formed from
    the fragment's face, its barycentrics and the vertices, takes the field's normal there (field_normals, one launch
    over the R^2 points) with the rasteriser's interpolated normal as the fallback; an uncovered pixel keeps the
    rasteriser's. `field` = (model, pose_to_camera, model_input) as field_normals takes them."""
    model, pose_to_camera, model_input = field
    face = fragments.pix_to_face
    covered = face >= 0
    corners = vertices.float()[triangles[face.clamp(min=0)]]                      # (R, R, 3 corners, 3)
    points = (fragments.bary[..., None] * corners).sum(dim=-2)
    normals = field_normals(model, pose_to_camera, points.reshape(-1, 3), model_input,
                            fallback=fragments.normals.reshape(-1, 3)).reshape(fragments.normals.shape)
    return torch.where(covered[..., None], normals, fragments.normals).contiguous()


def _shading_normals(fragments, vertices, triangles, normals, field):
    if normals == "mesh":
        return fragments.normals
    if normals != "field":
        raise ValueError(f"normals is 'mesh' (the rasteriser's interpolated face normals) or 'field' (the density gradient at "
                         f"every covered pixel), got {normals!r}")
    if field is None:
        raise ValueError("normals='field' takes field=(model, pose_to_camera, model_input), the field the mesh came from")
    return pixel_field_normals(fragments, vertices, triangles, field)


def _adds_return_normals(field_of):
    """Decorator of a mesh extractor whose result starts with (vertices, triangles): adds the keyword `return_normals`,
    which appends (V, 3) fp32 unit normals - the field's own normal at each final vertex (field_normals, one gradient
    launch; zeros where the field has no gradient). field_of(arguments) -> (model, part frames, model_input), from the
    extractor's bound arguments. The extractor keeps its signature: the keyword belongs to the wrapper."""
    def decorate(extract):
        signature = inspect.signature(extract)

        @functools.wraps(extract)
        def wrapper(*args, return_normals: bool = False, **kwargs):
            out = extract(*args, **kwargs)
            if not return_normals:
                return out
            bound = signature.bind(*args, **kwargs)
            bound.apply_defaults()
            model, pose_parts, model_input = field_of(bound.arguments)
            return tuple(out) + (field_normals(model, pose_parts, out[0], model_input),)
        return wrapper
    return decorate


@_adds_return_normals(lambda a: (a["model"], a["pose_to_camera"], a["model_input"]))
@torch.no_grad()
def extract_mesh(model, pose_to_camera: torch.Tensor, center: torch.Tensor, voxel_size: float = 0.003, mesh_th: float = 15,
                 model_input: Dict = {}, return_part_labels: bool = False, return_colors: bool = False,
                 simplify_cell: Optional[float] = None):
    """create_mesh (mesh_rendering.py:50-81) on the device: density_volume -> marching_cubes -> the reference's
    transform (vertices - cube) * voxel_size + center, in fp32. Returns (vertices (V, 3), triangles (T, 3) int64) on
    pose_to_camera's device. `return_part_labels` adds (V,) int32: the part that owns each vertex (-1: none), one
    point_part_labels launch over the vertex array; `return_colors` adds (V, 3) fp32 in [0, 1], the field's colour at
    each vertex (vertex_colors, one query launch); with both the result is (vertices, triangles, labels, colors).
    `simplify_cell` = h simplifies the mesh straight after the transform (ops.simplify_mesh(vertices, triangles, h):
    extract fine, cluster to cells of h camera units); labels and colours are then those of the simplified vertices.
    The keyword `return_normals` (of the decorator above) adds, last, (V, 3) fp32 unit normals: the field's own normal at
    each final vertex, after the simplification - the shading normal does not degrade with the triangle count."""
    if pose_to_camera.device.type != "cuda":
        raise _mesh_lib.EnarfHipError("extract_mesh runs on the device (there is no CPU fallback)")
    density = density_volume(model, pose_to_camera, center, voxel_size, model_input)
    cube = int(1 / voxel_size)
    vertices, triangles = marching_cubes(density, mesh_th)
    vertices = (vertices - cube) * voxel_size + center.to(vertices.device).float()[:, :, 0]
    if simplify_cell is not None:
        vertices, triangles = ops.simplify_mesh(vertices, triangles, simplify_cell)[:2]
    out = (vertices, triangles)
    if return_part_labels:
        out += (point_part_labels(model, pose_to_camera, vertices, model_input, points_last=True)[0][0],)
    if return_colors:
        out += (vertex_colors(model, pose_to_camera, vertices, model_input),)
    return out


def simplify_mesh(vertices: torch.Tensor, triangles: torch.Tensor, cell: Optional[float] = None,
                  target_triangles: Optional[int] = None, origin=None, placement: str = "quadric", reg: float = 1e-3,
                  max_runs: int = 12):
    """A finely extracted mesh made small: ops.simplify_mesh (uniform-grid vertex clustering, every new vertex placed by
    the quadric of the fine triangles that touch its cell; libenarf_simp.so) at the cell size `cell`, or at the finest cell
    found for which the result has at most `target_triangles` triangles. Exactly one of the two must be given. Returns
    the named tuple of ops.simplify_mesh, (vertices (C, 3) fp32, triangles (T', 3) int64, vertex_cluster (V,) int32,
    cluster_size (C,) int32).

    With `target_triangles` the cell is bisected over at most `max_runs` (12) runs of ops.simplify_mesh: the coarse end
    starts at the bounding-box diagonal (one cluster, no triangle: always within the target), the fine end at 0, each run
    tries the midpoint and keeps it as the coarse end when T' <= target, as the fine end otherwise; the mesh of the last
    coarse end is returned (run 1 is the diagonal itself). simplify_steps gives every run's (cell, T').

    Clustering does not preserve topology: surfaces nearer than a cell can merge and edges can become non-manifold.
    Attributes are not carried across: evaluate labels, colours, skin weights and the texture at the new vertices."""
    if (cell is None) == (target_triangles is None):
        raise ValueError("simplify_mesh takes exactly one of cell and target_triangles, got " +
                         ("both" if cell is not None else "neither"))
    if cell is not None:
        return ops.simplify_mesh(vertices, triangles, cell, origin=origin, placement=placement, reg=reg)
    return simplify_steps(vertices, triangles, target_triangles, origin, placement, reg, max_runs)[0]


def simplify_steps(vertices: torch.Tensor, triangles: torch.Tensor, target_triangles: int, origin=None,
                   placement: str = "quadric", reg: float = 1e-3, max_runs: int = 12):
    """The bisection of simplify_mesh(target_triangles=...): (the mesh returned, [(cell, T') of every run, in order])"""
    target = int(target_triangles)
    if target < 0 or int(max_runs) < 1:
        raise ValueError(f"simplify_mesh: target_triangles >= 0 and max_runs >= 1, got {target_triangles!r}, {max_runs!r}")
    run = lambda h: ops.simplify_mesh(vertices, triangles, h, origin=origin, placement=placement, reg=reg)
    if vertices.shape[0] == 0:
        return run(1.0), []
    extent = (vertices.amax(0) - vertices.amin(0)).double()
    coarse = max(float(extent.square().sum().sqrt()), 1e-30) * 1.0001          # above the diagonal: every vertex in one cell
    fine, best, steps = 0.0, run(coarse), []
    steps.append((coarse, best.triangles.shape[0]))
    for _ in range(int(max_runs) - 1):
        h = 0.5 * (fine + coarse)
        try:
            got = run(h)
        except NotImplementedError:            # more than 2^21 cells an axis: finer than any useful target
            fine = h
            continue
        steps.append((h, got.triangles.shape[0]))
        if got.triangles.shape[0] <= target:
            coarse, best = h, got
        else:
            fine = h
    return best, steps


@dataclasses.dataclass
class TextureAtlas:
    """The texture of a mesh in the per-triangle atlas of include/enarf_bake.h: texture (A, A, 4) uint8 RGBA (alpha 255 on
    the texels a triangle owns, 0 elsewhere), optionally texture_f32 (A, A, 3) fp32, the same colours before they were
    quantised, num_triangles T, size A and cell c (ops.bake_layout(T, A).cell). The UVs are not stored: atlas_uv(T, A)."""
    texture: torch.Tensor
    texture_f32: Optional[torch.Tensor]
    num_triangles: int
    size: int
    cell: int


def atlas_uv(T: int, size: int):
    """(T, 3, 2) fp32 numpy: the UV of every triangle corner in [0, 1], u to the right and v down from the top row (glTF's
    convention), computed on the host from the layout alone"""
    import numpy as np
    from ..._bake_lib import atlas_corners
    return (atlas_corners(T, size) / float(int(size))).astype(np.float32)


@torch.no_grad()
def bake_texture(model, pose_to_camera, vertices: torch.Tensor, triangles: torch.Tensor, model_input: Dict = {},
                 size: int = 1024, color: str = "field", palette=None, color_fn=None, want_float: bool = False,
                 band_rows: Optional[int] = None) -> TextureAtlas:
    """The texture atlas of a mesh: ops.bake_points gives the surface point of every texel, band of rows by band (at most
    2^22 texels a band by default, so the peak memory is bounded at 8192^2), the colour there comes from
      color="field"  one ops.query_fwd launch a band with the scaling and flags of vertex_colors (a band the layout leaves
                     without an owned texel - the margin, cells past the last triangle - is skipped);
      color="parts"  one ops.part_labels launch a band, drawn in `palette` ((semantic_palette + 1) / 2 by default);
      color_fn       a function points (M, 3) -> colours (M, 3) fp32 in [0, 1], instead of the model (which may be None),
    and ops.bake_resolve writes the band's rows of the texture. vertices (V, 3) fp32 in camera space and triangles (T, 3)
    int64 on the device, pose_to_camera (1, P, 4, 4) part frames with UNSCALED translation, as for vertex_colors."""
    if color_fn is None and color not in ("field", "parts"):
        raise ValueError(f"color is 'field' (the radiance field's colour) or 'parts' (the part labels), got {color!r}")
    T, A = triangles.shape[0], int(size)
    lay = ops.bake_layout(T, A)
    dev = vertices.device
    texture = torch.empty(A, A, 4, dtype=torch.uint8, device=dev)
    texture_f32 = torch.empty(A, A, 3, dtype=torch.float32, device=dev) if want_float else None
    per = max(1, min(A, (1 << 22) // A)) if band_rows is None else max(1, int(band_rows))
    if color_fn is None:
        from ..NeRF.rendering import _parts_from_part_poses, semantic_palette
        cs = model.coordinate_scale
        flags = model.kernel_flags()
        parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"])
        if color == "field":
            tri, feat_cl = model._tri_plane_pair(model_input)
            pack = model._mlp_pack(model_input["z_rend"])
        else:
            tri = _mask_tri_plane(model, model_input)
            if palette is None:
                palette = (semantic_palette(model.num_bone, dev) + 1) / 2
    for a in range(0, A, per):
        b = min(a + per, A)
        out = (texture[a:b], None if texture_f32 is None else texture_f32[a:b])
        if color_fn is None and color == "field" and (a >= lay.cells_per_row * lay.cell
                                                      or 2 * (a // lay.cell) * lay.cells_per_row >= T):
            texture[a:b] = 0                     # rows of the margin or of cells past the last triangle: what resolve gives
            if texture_f32 is not None:
                texture_f32[a:b] = 0
            continue
        baked = ops.bake_points(vertices, triangles, A, rows=(a, b))
        if color_fn is not None:
            rgb = color_fn(baked.points.t()).to(torch.float32).t().contiguous()
            ops.bake_resolve(baked.texel_face, color=rgb, unit=True, out=out)
        elif color == "parts":
            points = (baked.points * cs if cs != 1 else baked.points)[None]
            labels = ops.part_labels(points, parts, model.canonical_pose, tri, clamp_mask=flags["clamp_mask"],
                                     uniform_part_weight=flags["uniform_part_weight"])[0]
            ops.bake_resolve(baked.texel_face, labels=labels.reshape(-1), palette=palette.float(), out=out)
        else:
            points = (baked.points * cs if cs != 1 else baked.points)[None]
            _, rgb = ops.query_fwd(points, parts, model.canonical_pose, tri, feat_cl, pack, mlp_mode=model.mlp_mode,
                                   need_color=True, **flags)
            ops.bake_resolve(baked.texel_face, color=rgb[0], out=out)
    return TextureAtlas(texture, texture_f32, T, A, lay.cell)


@torch.no_grad()
def bake_normal_map(model, pose_to_camera, vertices: torch.Tensor, triangles: torch.Tensor, model_input: Dict = {},
                    size: int = 1024, normal_fn=None, min_gradient: float = 0.0, want_float: bool = False,
                    band_rows: Optional[int] = None) -> TextureAtlas:
    """The tangent-space normal map of a mesh in the atlas of bake_texture (the same layout: a TextureAtlas whose texture
    holds normals, texture_f32 them unquantised with `want_float`): band of rows by band as there, ops.bake_points gives
    the surface point of every texel, one ops.field_gradient launch a band the density's gradient there with the scaling
    and flags of field_normals, and ops.encode_normal_map writes -gradient / |gradient| in the frame of the texel's
    triangle (include/enarf_nmap.h) into the band's rows; a texel whose |gradient| <= min_gradient is flat (the face
    normal). A band the layout leaves without an owned texel is filled with the empty texel and skipped. With `normal_fn`,
    a function points (M, 3) -> vectors (M, 3), the vectors are the normals themselves and the model may be None. The map
    is baked in the pose the vertices are in - the rest pose of a rig - and rides with the triangles through skin_mesh:
    the frame is rebuilt from the posed vertices when it is drawn. Nothing synchronises."""
    T, A = triangles.shape[0], int(size)
    lay = ops.bake_layout(T, A)
    dev = vertices.device
    texture = torch.empty(A, A, 4, dtype=torch.uint8, device=dev)
    texture_f32 = torch.empty(A, A, 3, dtype=torch.float32, device=dev) if want_float else None
    per = max(1, min(A, (1 << 22) // A)) if band_rows is None else max(1, int(band_rows))
    if normal_fn is None:
        from ..NeRF.rendering import _parts_from_part_poses
        cs = model.coordinate_scale
        flags = model.kernel_flags()
        parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"])
        tri, feat_cl = model._tri_plane_pair(model_input)
        pack = model._mlp_pack(model_input["z_rend"])
    for a in range(0, A, per):
        b = min(a + per, A)
        out = (texture[a:b], None if texture_f32 is None else texture_f32[a:b])
        if a >= lay.cells_per_row * lay.cell or 2 * (a // lay.cell) * lay.cells_per_row >= T:
            texture[a:b].view(torch.int32).fill_(0x00FF8080)   # rows of the margin or of cells past the last triangle: what
                                                               # encode gives an empty texel, (128, 128, 255, 0), as one word
            if texture_f32 is not None:
                texture_f32[a:b, :, :2] = 0
                texture_f32[a:b, :, 2] = 1
            continue
        baked = ops.bake_points(vertices, triangles, A, rows=(a, b))
        if normal_fn is not None:
            vectors = normal_fn(baked.points.t()).to(torch.float32).t().contiguous()
            ops.encode_normal_map(baked.texel_face, vectors, vertices, triangles, negate=False, min_length=min_gradient, out=out)
        else:
            points = (baked.points * cs if cs != 1 else baked.points)[None].contiguous()
            _, gradient = ops.field_gradient(points, parts, model.canonical_pose, tri, feat_cl, pack, **flags)
            ops.encode_normal_map(baked.texel_face, gradient[0], vertices, triangles, negate=True, min_length=min_gradient,
                                  out=out)
    return TextureAtlas(texture, texture_f32, T, A, lay.cell)


@dataclasses.dataclass
class RiggedMesh:
    """A mesh bound to the parts of the model it was extracted from: vertices (V, 3) fp32 in camera units in the rest
    pose, triangles (T, 3) int64, joints (V, K) int32 (-1: unused slot) and weights (V, K) fp32 by descending weight,
    kept_mass (V,) fp32 (the share of the part-probability mass the K kept parts carry; 0: no part contains the vertex, it
    follows the nearest), rest_pose (1, P, 4, 4) the rest part frames with UNSCALED translation, rest_bone_length
    (1, P, 1), and optionally colors (V, 3) fp32 in [0, 1], labels (V,) int32, texture, the TextureAtlas of the mesh
    baked in the rest pose, and normal_map, its tangent-space normal map (bake_normal_map) in an atlas of the same layout."""
    vertices: torch.Tensor
    triangles: torch.Tensor
    joints: torch.Tensor
    weights: torch.Tensor
    kept_mass: torch.Tensor
    rest_pose: torch.Tensor
    rest_bone_length: torch.Tensor
    colors: Optional[torch.Tensor] = None
    labels: Optional[torch.Tensor] = None
    texture: Optional[TextureAtlas] = None
    normal_map: Optional[TextureAtlas] = None


def _mask_tri_plane(model, model_input: Dict) -> torch.Tensor:
    """the tri-plane whose part-probability planes point_part_labels reads"""
    tri = model_input.get("tri_plane_feature")
    if tri is None:
        tri = model.tri_plane if model.uses_warp else model.compute_tri_plane_feature(
            model_input.get("z"), model_input["bone_length"], model_input.get("truncation_psi", 1))
    if tri.shape[0] > 1 and tri.stride(0) == 0:       # an expanded constant tri-plane
        tri = tri[:1]
    return tri.detach()


def _adds_normal_map_size(field_of):
    """Decorator of a rig extractor (its result a RiggedMesh): adds the keyword `normal_map_size`, which fills the record's
    normal_map - bake_normal_map of the final (simplified) mesh in the rest pose at that atlas size. field_of(arguments) ->
    (model, part frames, model_input), from the extractor's bound arguments. The extractor keeps its signature: the keyword
    belongs to the wrapper, as `return_normals` does to _adds_return_normals'."""
    def decorate(extract):
        signature = inspect.signature(extract)

        @functools.wraps(extract)
        def wrapper(*args, normal_map_size: Optional[int] = None, **kwargs):
            rig = extract(*args, **kwargs)
            if normal_map_size is None:
                return rig
            bound = signature.bind(*args, **kwargs)
            bound.apply_defaults()
            model, pose_parts, model_input = field_of(bound.arguments)
            rig.normal_map = bake_normal_map(model, pose_parts, rig.vertices, rig.triangles, model_input, size=normal_map_size)
            return rig
        return wrapper
    return decorate


@_adds_normal_map_size(lambda a: (a["model"], a["pose_to_camera"], a["model_input"]))
@torch.no_grad()
def extract_rigged_mesh(model, pose_to_camera: torch.Tensor, center: torch.Tensor, voxel_size: float = 0.003,
                        mesh_th: float = 15, model_input: Dict = {}, max_influences: int = 4, return_colors: bool = False,
                        return_part_labels: bool = False, texture_size: Optional[int] = None,
                        texture_color: str = "field", simplify_cell: Optional[float] = None) -> RiggedMesh:
    """extract_mesh in the pose pose_to_camera (1, P, 4, 4) - the rest pose of the rig - plus one ops.skin_weights launch
    over the vertex array: every vertex bound to the max_influences (4 or 8) parts of the largest part probability among
    the parts whose cube contains it. `return_colors` and `return_part_labels` fill the record's colors and labels as
    extract_mesh returns them; `texture_size` fills its texture: bake_texture of the mesh in this pose, in `texture_color`
    ("field" or "parts"). The mesh is posed by skin_mesh and written out by export_glb. `simplify_cell` as in extract_mesh:
    the skin weights, colours, labels and the texture are those of the simplified mesh. The keyword `normal_map_size` (of
    the decorator above) fills normal_map: the field's normals baked into an atlas of that size for the final mesh, so a
    simplified rig keeps the shading detail of the field (paint_normal_mapped_mesh, export_glb)."""
    from ..NeRF.rendering import _parts_from_part_poses
    got = extract_mesh(model, pose_to_camera, center, voxel_size, mesh_th, model_input, return_part_labels, return_colors,
                       simplify_cell)
    vertices, triangles, extra = got[0], got[1], list(got[2:])
    labels = extra.pop(0) if return_part_labels else None
    colors = extra.pop(0) if return_colors else None
    bone_length = model_input["bone_length"]
    parts = _parts_from_part_poses(model, pose_to_camera, bone_length)
    flags = model.kernel_flags()
    joints, weights, kept = ops.skin_weights(vertices, parts, model.canonical_pose, _mask_tri_plane(model, model_input),
                                             max_influences=max_influences, clamp_mask=flags["clamp_mask"],
                                             uniform_part_weight=flags["uniform_part_weight"],
                                             coordinate_scale=float(model.coordinate_scale))
    texture = None
    if texture_size is not None:
        texture = bake_texture(model, pose_to_camera, vertices, triangles, model_input, size=texture_size, color=texture_color)
    return RiggedMesh(vertices, triangles, joints, weights, kept, pose_to_camera.detach().float().clone(),
                      bone_length.detach().float().reshape(1, -1, 1).clone(), colors, labels, texture)


@torch.no_grad()
def skin_mesh(model, rig: RiggedMesh, pose_to_camera: torch.Tensor, bone_length: torch.Tensor, out=None) -> torch.Tensor:
    """The rigged mesh in F poses: (F, V, 3) fp32 vertices in camera units, one ops.skin_pose launch, no new extraction.
    pose_to_camera (F, P, 4, 4) part frames with UNSCALED translation, as for point_part_labels; bone_length (F, P, 1) or
    (1, P, 1) part bone lengths (a bone longer than in the rest pose stretches its part). `out` as in ops.skin_pose."""
    from ..NeRF.rendering import _parts_from_part_poses
    F, P = pose_to_camera.shape[:2]
    rest = _parts_from_part_poses(model, rig.rest_pose, rig.rest_bone_length)
    parts = _parts_from_part_poses(model, pose_to_camera.float(), bone_length.float().reshape(-1, P, 1).expand(F, -1, -1))
    return ops.skin_pose(rig.vertices, rig.joints, rig.weights, rest, parts, coordinate_scale=float(model.coordinate_scale),
                         out=out)


def _host(a, dtype=None):
    import numpy as np
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def export_obj(vertices, triangles, path: str, colors=None, normals=None) -> None:
    """Plain-text Wavefront OBJ ("v x y z" lines, then "f a b c" with 1-based indices), as mcubes.export_obj writes.
    With `colors` (V, 3) in [0, 1] the vertex lines are "v x y z r g b", the extension MeshLab and Blender read. With
    `normals` (V, 3) a "vn x y z" line per vertex follows the vertices and the faces read "f a//a b//b c//c"."""
    import numpy as np
    v, f = _host(vertices), _host(triangles)
    c = None if colors is None else _host(colors)
    if c is not None and c.shape != (len(v), 3):
        raise ValueError(f"export_obj takes ({len(v)}, 3) colors, got {c.shape}")
    vn = None if normals is None else _host(normals)
    if vn is not None and vn.shape != (len(v), 3):
        raise ValueError(f"export_obj takes ({len(v)}, 3) normals, got {vn.shape}")
    with open(path, "w") as fh:
        for i, x in enumerate(v):
            if c is None:
                fh.write("v %r %r %r\n" % (float(x[0]), float(x[1]), float(x[2])))
            else:
                fh.write("v %r %r %r %r %r %r\n" % (float(x[0]), float(x[1]), float(x[2]),
                                                   float(c[i, 0]), float(c[i, 1]), float(c[i, 2])))
        if vn is not None:
            for x in vn:
                fh.write("vn %r %r %r\n" % (float(x[0]), float(x[1]), float(x[2])))
        for t in f.astype(np.int64) + 1:
            if vn is None:
                fh.write("f %d %d %d\n" % (t[0], t[1], t[2]))
            else:
                fh.write("f %d//%d %d//%d %d//%d\n" % (t[0], t[0], t[1], t[1], t[2], t[2]))


def export_ply(vertices, triangles, path: str, colors=None, labels=None, normals=None) -> None:
    """Binary little-endian PLY: per vertex float x y z, with `normals` (V, 3) float nx ny nz (straight after the
    position, where readers expect them), with `colors` (V, 3) in [0, 1] uchar red green blue =
    floor(255 clamp(c, 0, 1)) (the bytes the painted image uses), with `labels` (V,) int `part`; per face
    `list uchar int vertex_indices` (0-based)."""
    import numpy as np
    v, f = _host(vertices, np.float32).reshape(-1, 3), _host(triangles, np.int64).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}",
              "property float x", "property float y", "property float z"]
    if normals is not None:
        vn = _host(normals, np.float32)
        if vn.shape != (len(v), 3):
            raise ValueError(f"export_ply takes ({len(v)}, 3) normals, got {vn.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        c = _host(colors, np.float64)
        if c.shape != (len(v), 3):
            raise ValueError(f"export_ply takes ({len(v)}, 3) colors, got {c.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    if labels is not None:
        lab = _host(labels)
        if lab.shape != (len(v),):
            raise ValueError(f"export_ply takes ({len(v)},) labels, got {lab.shape}")
        fields.append(("part", "<i4"))
        header.append("property int part")
    if len(f) and (f.min() < -2 ** 31 or f.max() >= 2 ** 31):
        raise ValueError("export_ply: a vertex index does not fit the int of the face list")
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.zeros(len(v), dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vert["nx"], vert["ny"], vert["nz"] = vn[:, 0], vn[:, 1], vn[:, 2]
    if colors is not None:
        with np.errstate(invalid="ignore"):
            byte = np.floor(255 * np.clip(np.nan_to_num(c, nan=0.0), 0, 1)).astype(np.uint8)
        vert["red"], vert["green"], vert["blue"] = byte[:, 0], byte[:, 1], byte[:, 2]
    if labels is not None:
        vert["part"] = lab
    face = np.zeros(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def _quaternion(R):
    """(P, 3, 3) rotation matrices (float64) -> (P, 4) unit quaternions (x, y, z, w), w >= 0"""
    import numpy as np
    q = np.empty((len(R), 4))
    for i, m in enumerate(R):
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        if tr > 0:
            s = 2.0 * np.sqrt(1.0 + tr)
            q[i] = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
        else:
            a = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
            b, c = (a + 1) % 3, (a + 2) % 3
            s = 2.0 * np.sqrt(max(1.0 + m[a, a] - m[b, b] - m[c, c], 1e-300))
            q[i, a], q[i, b], q[i, c], q[i, 3] = 0.25 * s, (m[b, a] + m[a, b]) / s, (m[c, a] + m[a, c]) / s, (m[c, b] - m[b, c]) / s
        q[i] /= np.linalg.norm(q[i])
        if q[i, 3] < 0:
            q[i] = -q[i]
    return q


def _png_rgba(pixels) -> bytes:
    """(H, W, 4) uint8 -> the bytes of an 8-bit RGBA PNG (zlib and struct only; no filtering)"""
    import struct
    import zlib
    import numpy as np
    h, w = pixels.shape[:2]
    rows = np.zeros((h, 1 + 4 * w), np.uint8)
    rows[:, 1:] = pixels.reshape(h, 4 * w)

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def export_glb(rig: RiggedMesh, path: str, texture: Optional[TextureAtlas] = None, clips: Optional[Dict] = None,
               normals=None, normal_map: Optional[TextureAtlas] = None) -> None:
    """The rigged mesh as binary glTF 2.0 (standard library and numpy only): one mesh primitive with POSITION, optional
    COLOR_0 (float RGB), JOINTS_0 / WEIGHTS_0 and, at 8 influences, JOINTS_1 / WEIGHTS_1 (joints as unsigned bytes, an
    unused slot as joint 0 with weight 0), 32-bit indices; a flat skeleton of P joint nodes under one identity root, node
    k carrying the rest frame of part k as translation and rotation (its rest bone length in `extras`), and
    inverseBindMatrices = the inverses of the rest frames. A viewer that sets node k to (t_k, R_k, uniform scale
    bone_length_k / rest bone_length_k) of another pose reproduces skin_mesh.

    With a texture (`texture`, else rig.texture: a TextureAtlas of this mesh) the primitive is de-indexed - 3 T vertices,
    the attributes of each corner copied, indices 0 ... 3 T - 1 - and carries TEXCOORD_0 = atlas_uv instead of COLOR_0, one
    material (baseColorTexture, metallicFactor 0, roughnessFactor 1), one sampler (LINEAR both ways, CLAMP_TO_EDGE both
    ways) and the texture as a PNG embedded through a buffer view.

    `clips`: name -> (times (F,) in seconds, pose_to_camera (F, P, 4, 4) part frames with UNSCALED translation, as
    skin_mesh takes them, bone_length (F, P, 1) or (1, P, 1)). Each becomes an entry of `animations` with a translation, a
    rotation and a scale sampler for every part node, interpolation LINEAR: the rotation keys are unit quaternions whose
    sign follows the previous key (no key has a negative dot product with its predecessor), the scale is bone_length /
    rest bone_length, uniform. A viewer that plays a clip shows skin_mesh of its poses at the keys. With neither a texture
    nor clips the file is the one earlier versions wrote, byte for byte.

    `normals` (V, 3): the NORMAL attribute (float VEC3) of the rest pose, e.g. extract_mesh(return_normals=True)'s or
    field_normals at rig.vertices - de-indexed with the primitive when a texture is written; viewers skin it themselves.
    normals=None writes the bytes a call without the keyword writes.

    With a normal map (`normal_map`, else rig.normal_map: bake_normal_map's atlas of this mesh) the primitive is de-indexed
    as with a texture - also when there is no colour texture, COLOR_0 then copied to the corners - and carries TEXCOORD_0 =
    atlas_uv, NORMAL = the flat unit normal of each corner's triangle and TANGENT = (t^, -1) as float VEC4, t^ the tangent
    of include/enarf_nmap.h: a viewer's bitangent cross(NORMAL, TANGENT.xyz) * w is the b^ the map was encoded in. A
    triangle without a frame gets NORMAL (0, 0, 1) and TANGENT (1, 0, 0, -1). The material gains normalTexture, a second
    embedded PNG that shares the sampler; without a colour texture it has no baseColorTexture. `normals=` together with a
    normal map is a ValueError: the frame needs the face normal. Without a normal map every file is what it was."""
    import json
    import struct
    import numpy as np
    v = _host(rig.vertices, np.float32).reshape(-1, 3)
    f = _host(rig.triangles, np.int64).reshape(-1, 3)
    joints, weights = _host(rig.joints, np.int64), _host(rig.weights, np.float32)
    frames = _host(rig.rest_pose, np.float64).reshape(-1, 4, 4)
    bone = _host(rig.rest_bone_length, np.float64).reshape(-1)
    P, K = len(frames), joints.shape[1]
    if joints.shape != (len(v), K) or weights.shape != joints.shape or K not in (4, 8):
        raise ValueError(f"export_glb takes ({len(v)}, 4 or 8) joints and weights, got {joints.shape} and {weights.shape}")
    if P > 256 or (joints.size and joints.max() >= P):
        raise ValueError(f"export_glb: joints up to {int(joints.max())} with {P} parts (joints are unsigned bytes)")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("export_glb: a triangle names a vertex the mesh does not have")
    vn = None if normals is None else _host(normals, np.float32)
    if vn is not None and vn.shape != (len(v), 3):
        raise ValueError(f"export_glb takes ({len(v)}, 3) normals, got {vn.shape}")
    weights = np.where(joints >= 0, weights, np.float32(0)).astype(np.float32)
    joints = np.where(joints >= 0, joints, 0).astype(np.uint8)
    R, t = frames[:, :3, :3], frames[:, :3, 3]
    inverse = np.tile(np.eye(4), (P, 1, 1))
    inverse[:, :3, :3] = R.transpose(0, 2, 1)
    inverse[:, :3, 3] = -np.einsum("pji,pj->pi", R, t)
    chunks, views, accessors = [], [], []

    def add(array, kind, component, target=None, bounds=False):
        data = np.ascontiguousarray(array).tobytes()
        offset = sum(len(c) for c in chunks)
        chunks.append(data + b"\0" * (-len(data) % 4))
        view = {"buffer": 0, "byteOffset": offset, "byteLength": len(data)}
        if target is not None:
            view["target"] = target
        views.append(view)
        acc = {"bufferView": len(views) - 1, "componentType": component, "count": len(array), "type": kind}
        if bounds:
            acc["min"], acc["max"] = [float(x) for x in array.min(axis=0)], [float(x) for x in array.max(axis=0)]
        accessors.append(acc)
        return len(accessors) - 1

    FLOAT, UBYTE, UINT, ARRAY, ELEMENT = 5126, 5121, 5125, 34962, 34963
    texture = rig.texture if texture is None else texture
    normal_map = getattr(rig, "normal_map", None) if normal_map is None else normal_map
    if normal_map is not None and vn is not None:
        raise ValueError("export_glb: normals= cannot go with a normal map: NORMAL is then the face normal the tangent frame "
                         "is built on")
    atlases, pixels, corner, tangent = [a for a in (texture, normal_map) if a is not None], [], None, None
    for atlas in atlases:
        if atlas.num_triangles != len(f):
            raise ValueError(f"export_glb: the atlas was baked for {atlas.num_triangles} triangles, the mesh has {len(f)}")
        pixels.append(_host(atlas.texture, np.uint8))
        if pixels[-1].shape != (atlas.size, atlas.size, 4):
            raise ValueError(f"export_glb takes a ({atlas.size}, {atlas.size}, 4) uint8 texture, got {pixels[-1].shape}")
    if len(atlases) == 2 and texture.size != normal_map.size:
        raise ValueError(f"export_glb: the texture has {texture.size} texels a side, the normal map {normal_map.size}: both "
                         f"are read through one TEXCOORD_0")
    if normal_map is not None:
        from ..._nmap_lib import tangent_frames
        t_hat, _, n_hat, _ = tangent_frames(v, f)
        vn = np.repeat(n_hat.astype(np.float32), 3, axis=0)
        tangent = np.repeat(np.concatenate([t_hat, np.full((len(f), 1), -1.0)], 1).astype(np.float32), 3, axis=0)
    num_vertices = len(v)
    if atlases:
        corner = f.reshape(-1)                             # every corner a vertex of its own: its triangle's UV
        v, joints, weights = v[corner], joints[corner], weights[corner]
        if vn is not None and normal_map is None:          # with a normal map vn is already the face normal of every corner
            vn = vn[corner]
        f = np.arange(len(corner), dtype=np.int64).reshape(-1, 3)
    attributes = {"POSITION": add(v, "VEC3", FLOAT, ARRAY, bounds=len(v) > 0)}
    if vn is not None:
        attributes["NORMAL"] = add(vn, "VEC3", FLOAT, ARRAY)
    if tangent is not None:
        attributes["TANGENT"] = add(tangent, "VEC4", FLOAT, ARRAY)
    if atlases:
        attributes["TEXCOORD_0"] = add(atlas_uv(atlases[0].num_triangles, atlases[0].size).reshape(-1, 2), "VEC2", FLOAT, ARRAY)
    if texture is None and rig.colors is not None:
        c = np.clip(np.nan_to_num(_host(rig.colors, np.float32).reshape(-1, 3), nan=0.0), 0, 1)
        if corner is not None and len(c) == num_vertices:      # a normal map without a colour texture: colours per corner
            c = c[corner]
        if c.shape != v.shape:
            raise ValueError(f"export_glb takes ({len(v)}, 3) colors, got {c.shape}")
        attributes["COLOR_0"] = add(c, "VEC3", FLOAT, ARRAY)
    for s in range(K // 4):
        attributes[f"JOINTS_{s}"] = add(joints[:, 4 * s:4 * s + 4], "VEC4", UBYTE, ARRAY)
        attributes[f"WEIGHTS_{s}"] = add(weights[:, 4 * s:4 * s + 4], "VEC4", FLOAT, ARRAY)
    indices = add(f.astype(np.uint32).reshape(-1), "SCALAR", UINT, ELEMENT)
    ibm = add(inverse.transpose(0, 2, 1).astype(np.float32).reshape(P, 16), "MAT4", FLOAT)      # column-major
    quat = _quaternion(R)
    nodes = [{"name": f"part_{k}", "translation": [float(np.float32(x)) for x in t[k]],
              "rotation": [float(np.float32(x)) for x in quat[k]], "extras": {"bone_length": float(bone[k])}} for k in range(P)]
    nodes.append({"name": "skeleton", "children": list(range(P))})
    nodes.append({"name": "mesh", "mesh": 0, "skin": 0})
    primitive = {"attributes": attributes, "indices": indices, "mode": 4}
    extra = {}
    if atlases:
        images = []
        for px in pixels:                                  # the colour texture first, then the normal map
            png = _png_rgba(px)
            views.append({"buffer": 0, "byteOffset": sum(len(c) for c in chunks), "byteLength": len(png)})
            chunks.append(png + b"\0" * (-len(png) % 4))
            images.append({"bufferView": len(views) - 1, "mimeType": "image/png"})
        primitive["material"] = 0
        pbr = {"baseColorTexture": {"index": 0}} if texture is not None else {}
        material = {"pbrMetallicRoughness": {**pbr, "metallicFactor": 0.0, "roughnessFactor": 1.0}}
        if normal_map is not None:
            material["normalTexture"] = {"index": len(images) - 1}
        extra.update(materials=[material],
                     textures=[{"sampler": 0, "source": i} for i in range(len(images))],
                     samplers=[{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}],
                     images=images)
    if clips:
        animations = []
        for name, (times, poses, lengths) in clips.items():
            times = _host(times, np.float32).reshape(-1)
            poses = _host(poses, np.float64)
            F = len(times)
            if F < 1 or poses.shape != (F, P, 4, 4):
                raise ValueError(f"export_glb: clip {name!r} takes ({F}, {P}, 4, 4) poses for {F} >= 1 times, got {poses.shape}")
            lengths = _host(lengths, np.float64)
            if lengths.shape not in ((F, P, 1), (1, P, 1)):
                raise ValueError(f"export_glb: clip {name!r} takes ({F}, {P}, 1) or (1, {P}, 1) bone lengths, got {lengths.shape}")
            scale = np.broadcast_to(lengths[:, :, 0] / bone[None, :], (F, P))
            q = np.stack([_quaternion(poses[i, :, :3, :3]) for i in range(F)])                 # (F, P, 4)
            for i in range(1, F):                       # the shorter arc from key to key
                flip = np.einsum("pk,pk->p", q[i], q[i - 1]) < 0
                q[i, flip] = -q[i, flip]
            clock = add(times.reshape(-1, 1), "SCALAR", FLOAT, bounds=True)
            samplers, channels = [], []
            for k in range(P):
                keys = (("translation", poses[:, k, :3, 3].astype(np.float32), "VEC3"),
                        ("rotation", q[:, k].astype(np.float32), "VEC4"),
                        ("scale", np.repeat(scale[:, k, None], 3, axis=1).astype(np.float32), "VEC3"))
                for what, values, kind in keys:
                    samplers.append({"input": clock, "interpolation": "LINEAR", "output": add(values, kind, FLOAT)})
                    channels.append({"sampler": len(samplers) - 1, "target": {"node": k, "path": what}})
            animations.append({"name": str(name), "samplers": samplers, "channels": channels})
        extra["animations"] = animations
    doc = {"asset": {"version": "2.0", "generator": "enarf_gan_amd export_glb"}, "scene": 0,
           "scenes": [{"nodes": [P, P + 1]}], "nodes": nodes,
           "meshes": [{"primitives": [primitive]}],
           "skins": [{"joints": list(range(P)), "inverseBindMatrices": ibm, "skeleton": P}],
           "buffers": [{"byteLength": sum(len(c) for c in chunks)}], "bufferViews": views, "accessors": accessors, **extra}
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    binary = b"".join(chunks)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(text) + 8 + len(binary)))
        fh.write(struct.pack("<I4s", len(text), b"JSON") + text)
        fh.write(struct.pack("<I4s", len(binary), b"BIN\0") + binary)


def export_point_cloud(points, flags, path: str, colors=None, normals=None) -> None:
    """Binary little-endian PLY of the valid pixels of ops.geometry_buffers: `points` (..., 3) and `flags` (...) (bit 0 =
    valid) of one or several images; per vertex float x y z, with `normals` (..., 3) float nx ny nz, with `colors`
    (..., 3) - uint8 as the shape image holds them, or floats in [0, 1] - uchar red green blue; no faces."""
    import numpy as np
    p = _host(points, np.float32)
    keep = (_host(flags).astype(np.uint8) & 1).astype(bool)
    if p.shape[-1:] != (3,) or p.shape[:-1] != keep.shape:
        raise ValueError(f"export_point_cloud takes points (..., 3) and flags of the same leading shape, got {p.shape} and {keep.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {int(keep.sum())}",
              "property float x", "property float y", "property float z"]
    if normals is not None:
        n = _host(normals, np.float32)
        if n.shape != p.shape:
            raise ValueError(f"export_point_cloud takes normals of the points' shape {p.shape}, got {n.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        c = _host(colors)
        if c.shape != p.shape:
            raise ValueError(f"export_point_cloud takes colors of the points' shape {p.shape}, got {c.shape}")
        if c.dtype != np.uint8:
            with np.errstate(invalid="ignore"):
                c = np.floor(255 * np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0, 1)).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header.append("end_header")
    vert = np.zeros(int(keep.sum()), dtype=fields)
    vert["x"], vert["y"], vert["z"] = p[keep].T
    if normals is not None:
        vert["nx"], vert["ny"], vert["nz"] = n[keep].T
    if colors is not None:
        vert["red"], vert["green"], vert["blue"] = c[keep].T
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())


def rasterize_mesh(vertices: torch.Tensor, triangles: torch.Tensor, intrinsics, img_size: int, render_size: int = 512):
    """render_mesh_'s image (mesh_rendering.py:17-47) on the device (libenarf_raster.so), without pytorch3d.

    vertices (V, 3) fp32 in camera space and triangles (T, 3) int64 on the device, as extract_mesh returns them;
    intrinsics (3, 3) or (1, 3, 3) of an img_size x img_size image (fx, fy, cx, cy are used). Returns the namedtuple
    (image (R, R, 3) uint8, pix_to_face (R, R) int64, zbuf (R, R) fp32, bary (R, R, 3) fp32, normals (R, R, 3) fp32) of
    device tensors, R = render_size, in the orientation render_mesh_ returns (row 0 = the top of K's image). One fragment
    per pixel: the covering triangle (all 2-D barycentrics > 0 at the pixel centre, no culling) with the smallest
    view-space depth, then the smallest id; perspective-correct barycentrics; pytorch3d's default hard-Phong colours
    (ambient 0.5, diffuse 0.3, specular 0.2, shininess 64) with a white mesh and the light at the camera; background
    white. The full contract, and what is not drawn, is in include/enarf_raster.h. No CPU fallback."""
    return _raster_lib.rasterize_mesh(vertices, triangles, intrinsics, img_size, render_size)


def paint_mesh(vertices: torch.Tensor, triangles: torch.Tensor, intrinsics, img_size: int, render_size: int = 512,
               vertex_colors=None, vertex_labels=None, palette=None, lit: bool = True, normals: str = "mesh", field=None):
    """The mesh drawn in its vertex colours (V, 3) fp32 in [0, 1], or in the palette (P, 3) colours of its vertex labels
    (V,) int32: rasterize_mesh, then ops.shade_fragments on its fragment buffers (libenarf_paint.so, one launch more),
    with no host synchronisation. Returns (the RasterizedMesh of rasterize_mesh, the namedtuple (image (R, R, 3) uint8,
    albedo, shaded (R, R, 3) fp32) of shade_fragments). With `lit` the colours take the rasteriser's hard-Phong terms
    (white colours then give rasterize_mesh's own image); without, the image is the colour itself. normals="field" with
    field=(model, pose_to_camera, model_input) shades every covered pixel with the field's own normal at its surface point
    (pixel_field_normals: R^2 points, one gradient launch) instead of the interpolated face normal: per-pixel normal
    mapping without an atlas. No CPU fallback."""
    fragments = rasterize_mesh(vertices, triangles, intrinsics, img_size, render_size)
    painted = ops.shade_fragments(fragments.pix_to_face, fragments.bary,
                                  _shading_normals(fragments, vertices, triangles, normals, field), vertices, triangles,
                                  vertex_colors=vertex_colors, vertex_labels=vertex_labels, palette=palette, lit=lit)
    return fragments, painted


def paint_textured_mesh(vertices: torch.Tensor, triangles: torch.Tensor, atlas: TextureAtlas, intrinsics, img_size: int,
                        render_size: int = 512, lit: bool = True, use_float: bool = False, normals: str = "mesh", field=None):
    """The mesh drawn with its texture atlas: rasterize_mesh, then ops.shade_textured on its fragment buffers
    (libenarf_bake.so, one launch more), with no host synchronisation. Returns what paint_mesh returns: (the
    RasterizedMesh, the namedtuple (image (R, R, 3) uint8, albedo, shaded (R, R, 3) fp32)). The albedo is one bilinear tap
    of atlas.texture (of atlas.texture_f32 with `use_float`); the mesh may be posed (skin_mesh), the triangles are the
    atlas's. `normals` and `field` as in paint_mesh. No CPU fallback."""
    if atlas.num_triangles != triangles.shape[0]:
        raise ValueError(f"paint_textured_mesh: the atlas was baked for {atlas.num_triangles} triangles, the mesh has "
                         f"{triangles.shape[0]}")
    if use_float and atlas.texture_f32 is None:
        raise ValueError("paint_textured_mesh: use_float takes an atlas baked with want_float=True")
    fragments = rasterize_mesh(vertices, triangles, intrinsics, img_size, render_size)
    painted = ops.shade_textured(fragments.pix_to_face, fragments.bary,
                                 _shading_normals(fragments, vertices, triangles, normals, field), vertices, triangles,
                                 atlas.texture_f32 if use_float else atlas.texture, lit=lit)
    return fragments, painted


def paint_normal_mapped_mesh(vertices: torch.Tensor, triangles: torch.Tensor, normal_atlas: TextureAtlas, intrinsics,
                             img_size: int, render_size: int = 512, atlas: Optional[TextureAtlas] = None, base_color=1.0,
                             lit: bool = True, use_float: bool = False):
    """The mesh drawn with its tangent-space normal map: rasterize_mesh, then ops.shade_normal_mapped on its fragment
    buffers (libenarf_nmap.so, one launch more), with no host synchronisation. Returns (the RasterizedMesh, the namedtuple
    (image (R, R, 3) uint8, albedo, normal, shaded (R, R, 3) fp32)). The shading normal is one bilinear tap of
    normal_atlas.texture (of its texture_f32 with `use_float`) in the frame of the pixel's triangle, built from the
    vertices given - the mesh may be posed (skin_mesh), the triangles are the atlases'; the albedo one tap of `atlas` (a
    colour atlas of the same size; its texture_f32 with `use_float` when it has one) or the constant base_color. No CPU
    fallback."""
    for name, a in (("normal map", normal_atlas), ("colour atlas", atlas)):
        if a is not None and a.num_triangles != triangles.shape[0]:
            raise ValueError(f"paint_normal_mapped_mesh: the {name} was baked for {a.num_triangles} triangles, the mesh has "
                             f"{triangles.shape[0]}")
    if atlas is not None and atlas.size != normal_atlas.size:
        raise ValueError(f"paint_normal_mapped_mesh: the normal map has {normal_atlas.size} texels a side, the colour atlas "
                         f"{atlas.size}")
    if use_float and normal_atlas.texture_f32 is None:
        raise ValueError("paint_normal_mapped_mesh: use_float takes a normal map baked with want_float=True")
    fragments = rasterize_mesh(vertices, triangles, intrinsics, img_size, render_size)
    albedo = None if atlas is None else (atlas.texture_f32 if use_float and atlas.texture_f32 is not None else atlas.texture)
    painted = ops.shade_normal_mapped(fragments.pix_to_face, fragments.bary, fragments.normals, vertices, triangles,
                                      normal_atlas.texture_f32 if use_float else normal_atlas.texture, texture=albedo,
                                      base_color=base_color, lit=lit)
    return fragments, painted


def render_mesh_(meshes, intrinsics, img_size, render_size=512):
    """mesh_rendering.py:17-47: Phong-shaded rasterisation of (vertices, triangles, textures) with pytorch3d. The
    rasteriser is third-party and outside the hot path (out of scope); this raises ImportError where the
    reference's module import would."""
    try:
        import pytorch3d.renderer  # noqa: F401
    except ImportError as e:
        raise ImportError("render_mesh_ needs pytorch3d (as the reference does)") from e
    raise NotImplementedError("the pytorch3d rasteriser call is not rebuilt here (SURVEY.md §8, out of scope); "
                              "use create_mesh() / density_volume() and rasterise with pytorch3d directly")
