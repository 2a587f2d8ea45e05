"""`render` / `render_entire_img` with the reference's signatures (libraries/NeRF/rendering.py:227-427).

The whole body of the reference's render() - frustum range, coarse pass, importance sampling, fine pass,
compositing - is ONE launch of the fused HIP ray march (enarf_render_fwd); nothing is computed in torch
except packing the already-transformed part frames into the kernel's 16-float records.
"""
from typing import Dict, Optional

import torch

from ... import ops


def _parts_from_part_poses(model, pose_to_camera: torch.Tensor, bone_length: torch.Tensor) -> torch.Tensor:
    """(B, P, 4, 4) part frames (unscaled translation) -> the kernel's (B, P, 16) records.

    Same arithmetic as rendering.py:258-260 (t *= coordinate_scale) and narf.py:165 (cbl / bl / cs)."""
    B, P = pose_to_camera.shape[:2]
    cs = model.coordinate_scale
    parts = torch.zeros(B, P, 16, dtype=torch.float32, device=pose_to_camera.device)
    parts[:, :, :9] = pose_to_camera[:, :, :3, :3].reshape(B, P, 9)
    parts[:, :, 9:12] = pose_to_camera[:, :, :3, 3] * cs if cs != 1 else pose_to_camera[:, :, :3, 3]
    parts[:, :, 12] = (model.canonical_bone_length[:, None] / bone_length / cs)[:, :, 0]
    return parts


_MLP_LEAVES = ("conv.weight", "conv.modulation.weight", "conv.modulation.bias", "bias")


def semantic_palette(num_parts: int, device=None) -> torch.Tensor:
    """(num_parts, 3) fp32 colours in {-1, 0, 1}^3, the table of rendering.py:300-302: entry i is
    (i // 9, (i // 3) % 3, i % 3) - 1, then every even i takes the original entry E - i, E the largest even index below
    num_parts (seg_color[::2] = seg_color.flip(0)[1 - num_parts % 2::2]), which sets neighbouring parts apart."""
    i = torch.arange(num_parts)
    base = torch.stack([i // 9, (i // 3) % 3, i % 3], dim=1) - 1
    out = base.clone()
    even = i[::2]
    out[even] = base[(num_parts - 1) // 2 * 2 - even]
    return out.to(device=device, dtype=torch.float32)


def _render_semantic(model, image_coord, inv_intrinsics, parts, tri, feat_cl, pack, Nc, Nf, render_scale, bins, seed, flags):
    """render(semantic_map=True) without gradients: the march with its taps, the owner of every fine sample, and the
    labels composed with the march's weights (rendering.py:298-305, :316-335 with the palette in place of the colour)."""
    out = ops.render_fwd(image_coord, inv_intrinsics, parts, model.canonical_pose, tri, feat_cl, pack, Nc, Nf,
                         render_scale=render_scale, bins=bins, seed=seed, mlp_mode=model.mlp_mode, debug=True, **flags)
    t = out.taps
    seg = {k: v for k, v in flags.items() if k in ("clamp_mask", "uniform_part_weight")}
    labels, _, _ = ops.part_labels_on_rays(image_coord.float(), inv_intrinsics.float(), t["depth_min"], t["depth_max"],
                                           t["bins"], parts, model.canonical_pose, tri, **seg)
    color, part_map, part_mass = ops.semantic_composite(labels, out.fine_weights,
                                                        semantic_palette(parts.shape[1], labels.device))
    model.buffers_tensors.update(bins=t["bins"], fine_weights=out.fine_weights, fine_depth=out.fine_depth,
                                 depth_min=t["depth_min"], depth_max=t["depth_max"], part_labels=labels,
                                 part_map=part_map, part_mass=part_mass)
    return color, out.mask, out.disparity


class _RenderFunction(torch.autograd.Function):
    """Differentiable wrapper of the fused march: forward = enarf_prepare (MLP pack) + enarf_triplane_pack +
    enarf_render_fwd, backward = enarf_render_bwd + enarf_weight_grad (dW') + enarf_prepare_bwd + un-pack.
    Differentiable inputs: the tri-plane, z_rend and the 12 StyledMLP tensors (as in the reference, not the pose and
    not the importance samples)."""

    @staticmethod
    def forward(ctx, k, tri, z_rend, *params):
        mlp = {f"layers.{i}.{leaf}": params[4 * i + j] for i in range(3) for j, leaf in enumerate(_MLP_LEAVES)}
        tri_c = tri.detach().contiguous()
        feat_cl = ops.triplane_pack(tri_c)
        pack = k["pack_fn"](z_rend.detach(), {n: t.detach() for n, t in mlp.items()})
        out = ops.render_fwd(k["image_coord"], k["inv_intrinsics"], k["parts"], k["canonical_pose"], tri_c, feat_cl, pack,
                             k["Nc"], k["Nf"], render_scale=k["render_scale"], bins=k["bins"], seed=k["seed"],
                             mlp_mode=k["mlp_mode"], return_bins=True, **k["flags"])
        bins_used = out.taps["bins"]
        ctx.k = k
        ctx.save_for_backward(tri_c, feat_cl, pack, bins_used, z_rend.detach(), *[p.detach() for p in params])
        ctx.mark_non_differentiable(out.fine_weights, out.fine_depth, bins_used)
        return out.color, out.mask, out.disparity, out.fine_weights, out.fine_depth, bins_used

    @staticmethod
    def backward(ctx, g_color, g_mask, g_disp, _gfw, _gfd, _gb):
        k = ctx.k
        tri_c, feat_cl, pack, bins_used, z_rend = ctx.saved_tensors[:5]
        params = ctx.saved_tensors[5:]
        mlp = {f"layers.{i}.{leaf}": params[4 * i + j] for i in range(3) for j, leaf in enumerate(_MLP_LEAVES)}
        grad_tri, dW, db = ops.render_bwd(k["image_coord"], k["inv_intrinsics"], k["parts"], k["canonical_pose"], tri_c,
                                          feat_cl, pack, k["Nf"], bins_used, g_color, g_mask, g_disp,
                                          render_scale=k["render_scale"], **k["flags"])
        pg, dz = ops.prepare_bwd(z_rend, mlp, dW)
        grads = []
        for i in range(3):
            grads += [pg[f"layers.{i}.conv.weight"], pg[f"layers.{i}.conv.modulation.weight"],
                      pg[f"layers.{i}.conv.modulation.bias"], db[i].reshape(params[4 * i + 3].shape)]
        return (None, grad_tri, dz) + tuple(grads)


class _RenderFunctionCL(torch.autograd.Function):
    """The same march for producers that emit channel-last feature planes (the deformation-field warp): differentiable
    inputs are the NCHW tri-plane that holds the part-probability planes (1 or B images), the channel-last feature planes
    (B, 3, H, W, 32), z_rend and the StyledMLP tensors. No NCHW <-> channel-last copy in either direction."""

    @staticmethod
    def forward(ctx, k, tri, feat_cl, z_rend, *params):
        mlp = {f"layers.{i}.{leaf}": params[4 * i + j] for i in range(3) for j, leaf in enumerate(_MLP_LEAVES)}
        tri_c, feat_c = tri.detach().contiguous(), feat_cl.detach().contiguous()
        pack = k["pack_fn"](z_rend.detach(), {n: t.detach() for n, t in mlp.items()})
        out = ops.render_fwd(k["image_coord"], k["inv_intrinsics"], k["parts"], k["canonical_pose"], tri_c, feat_c, pack,
                             k["Nc"], k["Nf"], render_scale=k["render_scale"], bins=k["bins"], seed=k["seed"],
                             mlp_mode=k["mlp_mode"], return_bins=True, **k["flags"])
        bins_used = out.taps["bins"]
        ctx.k = k
        ctx.save_for_backward(tri_c, feat_c, pack, bins_used, z_rend.detach(), *[p.detach() for p in params])
        ctx.mark_non_differentiable(out.fine_weights, out.fine_depth, bins_used)
        return out.color, out.mask, out.disparity, out.fine_weights, out.fine_depth, bins_used

    @staticmethod
    def backward(ctx, g_color, g_mask, g_disp, _gfw, _gfd, _gb):
        k = ctx.k
        tri_c, feat_c, pack, bins_used, z_rend = ctx.saved_tensors[:5]
        params = ctx.saved_tensors[5:]
        mlp = {f"layers.{i}.{leaf}": params[4 * i + j] for i in range(3) for j, leaf in enumerate(_MLP_LEAVES)}
        grad_tri, dW, db, gfeat = ops.render_bwd(k["image_coord"], k["inv_intrinsics"], k["parts"], k["canonical_pose"],
                                                 tri_c, feat_c, pack, k["Nf"], bins_used, g_color, g_mask, g_disp,
                                                 render_scale=k["render_scale"], feat_grad_channel_last=True, **k["flags"])
        pg, dz = ops.prepare_bwd(z_rend, mlp, dW)
        grads = []
        for i in range(3):
            grads += [pg[f"layers.{i}.conv.weight"], pg[f"layers.{i}.conv.modulation.weight"],
                      pg[f"layers.{i}.conv.modulation.bias"], db[i].reshape(params[4 * i + 3].shape)]
        return (None, grad_tri, gfeat, dz) + tuple(grads)


def render(model, image_coord: torch.Tensor, pose_to_camera: torch.Tensor, inv_intrinsics: torch.Tensor,
           render_scale: float = 1, Nc: int = 64, Nf: int = 128, semantic_map: bool = False,
           return_intermediate: bool = False, camera_pose: Optional[torch.Tensor] = None,
           model_input: Dict = {}, _parts: Optional[torch.Tensor] = None, _pack: Optional[torch.Tensor] = None,
           bins: Optional[torch.Tensor] = None, seed: Optional[int] = None):
    """image_coord (B, 1, 3, n); pose_to_camera (B, P, 4, 4) part frames -> color (B,3,n), mask (B,n), disparity (B,n).

    Extra keyword arguments (not in the reference): `bins` (B, n, Nf) replays given importance samples;
    `seed` seeds the in-kernel Philox draw (default: a fresh 63-bit number from torch's CPU generator).

    semantic_map=True (the branch the reference leaves behind `assert False`, rendering.py:298-305) returns the part
    segmentation in place of the colour: every fine sample takes the palette colour of the part that owns it
    (semantic_palette, ops.part_labels_on_rays) and is composed with the march's weights; mask and disparity are those of
    the plain call. `part_map` (B, n) int32, `part_mass` (B, n) and `part_labels` (B, n, Nf) int32 are left in
    model.buffers_tensors. Labels carry no gradient: with gradients required it raises NotImplementedError."""
    if pose_to_camera.requires_grad:
        raise NotImplementedError("Currently pose should not be differentiable")   # rendering.py:216-217
    assert pose_to_camera.shape[1] == model.num_bone
    if not hasattr(model, "buffers_tensors"):
        model.buffers_tensors = {}
    if _parts is None:
        _parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"])
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    cfg = model.config
    mult_w = bool(cfg.multiply_density_with_triplane_wieght)
    z_rend = model_input["z_rend"]
    params = model.mlp.as_dict()
    needs_grad = False
    cl_route = bool(getattr(model, "uses_warp", False)) and model_input.get("tri_plane_feature") is None
    if torch.is_grad_enabled():
        if cl_route:     # the producer emits channel-last planes: (part-probability planes NCHW, feature planes channel-last)
            tri_graph, feat_graph = model._tri_plane_pair_graph(model_input)
            needs_grad = feat_graph.requires_grad
        else:
            tri_graph = model._tri_plane_graph(model_input)    # tri-plane as the autograd graph sees it
        needs_grad = (needs_grad or tri_graph.requires_grad or z_rend.requires_grad or
                      any(p.requires_grad for p in params.values()))
    if needs_grad and semantic_map:
        raise NotImplementedError("semantic_map=True is not differentiable (part labels carry no gradient); call it "
                                  "under torch.no_grad()")
    if needs_grad and return_intermediate:
        raise NotImplementedError("return_intermediate=True is served from the kernel's taps and is not differentiable; "
                                  "call it under torch.no_grad()")
    flags = model.kernel_flags() if hasattr(model, "kernel_flags") else dict(multiply_density_with_weight=mult_w)
    if needs_grad:
        k = dict(image_coord=image_coord.detach(), inv_intrinsics=inv_intrinsics.detach(), parts=_parts.detach(),
                 canonical_pose=model.canonical_pose, Nc=Nc, Nf=Nf, render_scale=float(render_scale), bins=bins, seed=seed,
                 mlp_mode=model.mlp_mode, pack_fn=model._mlp_pack_from, flags=flags)
        flat = [params[f"layers.{i}.{leaf}"] for i in range(3) for leaf in _MLP_LEAVES]
        if cl_route:
            color, mask, disparity, fw, fd, bins_used = _RenderFunctionCL.apply(k, tri_graph, feat_graph, z_rend, *flat)
            model.buffers_tensors.update(fine_weights=fw, fine_depth=fd, bins=bins_used, tri_plane_feature=None)
        else:
            color, mask, disparity, fw, fd, bins_used = _RenderFunction.apply(k, tri_graph, z_rend, *flat)
            model.buffers_tensors.update(fine_weights=fw, fine_depth=fd, bins=bins_used, tri_plane_feature=tri_graph)
        return color, mask, disparity
    tri, feat_cl = model._tri_plane_pair(model_input)
    if _pack is None:
        _pack = model._mlp_pack(z_rend)
    if semantic_map:
        if return_intermediate:
            raise NotImplementedError("semantic_map=True with return_intermediate=True")
        return _render_semantic(model, image_coord, inv_intrinsics, _parts, tri, feat_cl, _pack, Nc, Nf, render_scale, bins,
                                seed, flags)
    out = ops.render_fwd(image_coord, inv_intrinsics, _parts, model.canonical_pose, tri, feat_cl, _pack, Nc, Nf,
                         render_scale=render_scale, bins=bins, seed=seed, mlp_mode=model.mlp_mode,
                         return_bins=True, debug=return_intermediate, **flags)
    model.buffers_tensors["bins"] = out.taps["bins"]
    model.buffers_tensors["fine_weights"] = out.fine_weights      # (B, 1, n, Nf-1); zeros for dropped rays
    model.buffers_tensors["fine_depth"] = out.fine_depth          # (B, 1, n, Nf)
    if return_intermediate:
        # (fine_points (B, 3, n*Nf), fine_density (B, 1, n*Nf)) of rendering.py:291, for ALL n rays (the reference
        # compacts batch 1 to the rays that hit; dropped rays hold zero density here) - from the kernel's taps
        t = out.taps
        B, n = out.mask.shape
        coord = image_coord.reshape(B, 3, n).to(torch.float32)
        Ki = inv_intrinsics.to(torch.float32)
        if Ki.dim() == 2:
            Ki = Ki[None].expand(B, -1, -1)
        ray = torch.einsum("bij,bjn->bin", Ki, coord)
        b_ = t["bins"][:, None]                                                # (B, 1, n, Nf)
        start, end = (t["depth_min"][:, None] * ray)[..., None], (t["depth_max"][:, None] * ray)[..., None]
        fine_points = (start * (1 - b_) + end * b_).reshape(B, 3, n * Nf)
        fine_density = t["fine_density"].reshape(B, 1, n * Nf)
        model.buffers_tensors["fine_density"] = fine_density
        return out.color, out.mask, out.disparity, (fine_points, fine_density)
    return out.color, out.mask, out.disparity


def render_entire_img(model, pose_to_camera: torch.Tensor, inv_intrinsics: torch.Tensor,
                      camera_pose: Optional[torch.Tensor] = None, render_size: int = 128, Nc: int = 64,
                      Nf: int = 128, semantic_map: bool = False, use_normalized_intrinsics: bool = False,
                      no_grad: bool = True, model_input: Dict = {}, bbox=None):
    """Whole frame of image 0 (rendering.py:362-427) -> (3,H,W), (H,W), (H,W). One launch: the reference's
    render_bs chunk loop exists to bound its (B,P,3,n*N) temporaries, which the fused kernel never creates."""
    if bbox is not None:
        render_width, render_height = bbox[2] - bbox[0], bbox[3] - bbox[1]
        x_offset, y_offset = bbox[0], bbox[1]
    else:
        render_width, render_height = render_size, render_size
        x_offset, y_offset = 0, 0
    dev = pose_to_camera.device
    idx = torch.arange(render_width * render_height, device=dev)
    x = (idx % render_width + 0.5 + x_offset).float()
    y = (torch.div(idx, render_width, rounding_mode="floor") + 0.5 + y_offset).float()
    if use_normalized_intrinsics:
        x, y = x / render_size, y / render_size
    img_coord = torch.stack([x, y, torch.ones_like(x)], dim=0)[None, None]
    mi = dict(model_input)
    mi["bone_length"] = mi["bone_length"][:1]
    if mi.get("z_rend") is not None:
        mi["z_rend"] = mi["z_rend"][:1]
    if mi.get("tri_plane_feature") is not None:
        mi["tri_plane_feature"] = mi["tri_plane_feature"][:1]
    with torch.set_grad_enabled(not no_grad):
        color, mask, disparity = render(model, img_coord, pose_to_camera[:1], inv_intrinsics, Nc=Nc, Nf=Nf,
                                        semantic_map=semantic_map, camera_pose=camera_pose, model_input=mi)
    return (color.reshape(3, render_height, render_width), mask.reshape(render_height, render_width),
            disparity.reshape(render_height, render_width))


def composite_fine(density: torch.Tensor, color: torch.Tensor, depth: torch.Tensor, render_scale: float = 1.0):
    """The reference's alpha compositing of the fine samples (rendering.py:307-335) in torch, on any device and dtype:
    density (B, n, Nf), color (B, 3, n, Nf), depth (B, n, Nf) -> colour (B, 3, n), mask (B, n), disparity (B, n), weights
    (B, n, Nf - 1). The first Nf - 1 samples are integrated; sample i spans depth[i + 1] - depth[i]."""
    delta = depth[..., 1:] - depth[..., :-1]
    dd = density[..., :-1] * delta * render_scale
    transmittance = torch.exp(-(torch.cumsum(dd, dim=-1) - dd))
    w = transmittance * (1 - torch.exp(-dd))
    return (w[:, None] * color[..., :-1]).sum(dim=-1), w.sum(dim=-1), (w * 1 / depth[..., :-1]).sum(dim=-1), w


def _fixed_samples(model, image_coord, inv_intrinsics, parts, tri, feat_cl, pack, Nc, Nf, render_scale, bins, seed,
                   with_outputs=False):
    """The sample positions a posable render holds fixed, from one march with its taps (call under no_grad): image_coord
    (B, 1, 3, n) or (B, 3, n), inv_intrinsics (3, 3) or (B, 3, 3) -> (the march's taps, fine_points (B, 3, n Nf) formed from
    bins, depth_min and depth_max as return_intermediate forms them, fine_depth (B, n, Nf)); `with_outputs` adds the
    march's own RenderOutputs (colour, mask, disparity, fine_weights)."""
    B, n = image_coord.shape[0], image_coord.shape[-1]
    out = ops.render_fwd(image_coord, inv_intrinsics, parts, model.canonical_pose, tri, feat_cl, pack, Nc, Nf,
                         render_scale=render_scale, bins=bins, seed=seed, mlp_mode=model.mlp_mode, debug=True,
                         **model.kernel_flags())
    t = out.taps
    coord = image_coord.reshape(B, 3, n).to(torch.float32)
    Ki = inv_intrinsics.to(torch.float32)
    if Ki.dim() == 2:
        Ki = Ki[None].expand(B, -1, -1)
    ray = torch.einsum("bij,bjn->bin", Ki, coord)
    b_ = t["bins"][:, None]                                                # (B, 1, n, Nf)
    start, end = (t["depth_min"][:, None] * ray)[..., None], (t["depth_max"][:, None] * ray)[..., None]
    fine_points = (start * (1 - b_) + end * b_).reshape(B, 3, n * Nf)
    fine_depth = t["depth_min"][..., None] * (1 - t["bins"]) + t["depth_max"][..., None] * t["bins"]
    if with_outputs:
        return t, fine_points, fine_depth, out
    return t, fine_points, fine_depth


def _march_with_gradient(model, image_coord, inv_intrinsics, parts, pack, Nc, Nf, render_scale, model_input, bins, seed):
    """One march with its taps (_fixed_samples) and one ops.field_gradient launch on its fine points, under no_grad:
    (the march's RenderOutputs, gradient (B, 3, n Nf)). The seed is drawn as render() draws it."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    if not hasattr(model, "buffers_tensors"):
        model.buffers_tensors = {}
    with torch.no_grad():
        tri, feat_cl = model._tri_plane_pair(model_input)
        t, fine_points, _, out = _fixed_samples(model, image_coord, inv_intrinsics, parts, tri, feat_cl, pack, Nc, Nf,
                                                render_scale, bins, seed, with_outputs=True)
        density, gradient = ops.field_gradient(fine_points, parts, model.canonical_pose, tri, feat_cl, pack,
                                               **model.kernel_flags())
    model.buffers_tensors.update(bins=t["bins"], fine_weights=out.fine_weights, fine_depth=out.fine_depth,
                                 fine_points=fine_points, fine_gradient=gradient, fine_density=density[:, None])
    return out, gradient


def render_field_normals(model, image_coord: torch.Tensor, pose_to_camera: torch.Tensor, inv_intrinsics: torch.Tensor,
                         render_scale: float = 1, Nc: int = 64, Nf: int = 128, model_input: Dict = {},
                         bins: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                         _parts: Optional[torch.Tensor] = None, _pack: Optional[torch.Tensor] = None, **normal_kwargs):
    """render() with the field's own normal of every ray: image_coord (B, 1, 3, n); pose_to_camera (B, P, 4, 4) part
    frames -> (colour (B, 3, n), mask (B, n), disparity (B, n), the RayNormals of ops.ray_normals). One march with its taps
    (as render_posable's), one ops.field_gradient launch on its fine points, one ops.ray_normals launch: the normal is
    minus the density gradient composited with the march's own fine weights, in camera space. Colour, mask and disparity
    are render()'s on the same seed and bins. normal_kwargs go to ops.ray_normals (fallback, flags, points, shade,
    mask_threshold, min_gradient, background, want_magnitude). The fine points, their gradient and density are left in
    model.buffers_tensors (fine_points, fine_gradient, fine_density). Runs under no_grad; inputs that require a gradient
    raise NotImplementedError."""
    assert pose_to_camera.shape[1] == model.num_bone
    z_rend = model_input["z_rend"]
    if torch.is_grad_enabled() and (pose_to_camera.requires_grad or z_rend.requires_grad or
                                    model._tri_plane_graph(model_input).requires_grad or
                                    any(p.requires_grad for p in model.mlp.as_dict().values())):
        raise NotImplementedError("render_field_normals is not differentiable (no gradient flows through normals); call "
                                  "it under torch.no_grad()")
    with torch.no_grad():
        if _parts is None:
            _parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"])
        if _pack is None:
            _pack = model._mlp_pack(z_rend)
        out, gradient = _march_with_gradient(model, image_coord, inv_intrinsics, _parts, _pack, Nc, Nf, render_scale,
                                             model_input, bins, seed)
        normals = ops.ray_normals(gradient, out.fine_weights, out.mask, **normal_kwargs)
    return out.color, out.mask, out.disparity, normals


def render_posable(model, image_coord: torch.Tensor, pose_to_camera: torch.Tensor, inv_intrinsics: torch.Tensor,
                   render_scale: float = 1, Nc: int = 64, Nf: int = 128, model_input: Dict = {},
                   bins: Optional[torch.Tensor] = None, seed: Optional[int] = None):
    """render() for a pose that requires gradients: image_coord (B, 1, 3, n); pose_to_camera (B, P, 4, 4) part frames
    (translation not yet scaled, as render takes them); model_input["bone_length"] the parts' bone lengths ->
    (colour (B, 3, n), mask (B, n), disparity (B, n)), differentiable with respect to pose_to_camera and bone_length, and
    to the tri-plane, z_rend and the StyledMLP where they require gradients.

    Contract: the gradient is that of the image AT FIXED SAMPLE POSITIONS. One march under no_grad (the fused kernel, its
    taps) fixes every ray's depth range, its validity and its importance samples; the fine points are formed from them as
    return_intermediate forms them and are constants. model.query_posable at those points and the reference's compositing
    (composite_fine) carry the gradient. The reference detaches its importance samples as well; what is ignored here
    beyond that is the dependence of a ray's depth range on the pose. The forward values are those of
    render() on the same bins up to the rounding of the compositing sums. A ray the march drops (one image, no cube hit)
    is zero."""
    assert pose_to_camera.shape[1] == model.num_bone
    B, n = image_coord.shape[0], image_coord.shape[-1]
    cs = model.coordinate_scale
    z_rend = model_input["z_rend"]
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    with torch.no_grad():
        parts = _parts_from_part_poses(model, pose_to_camera.detach(), model_input["bone_length"].detach())
        mi = dict(model_input)
        tri, feat_cl = model._tri_plane_pair(mi)
        t, fine_points, fine_depth = _fixed_samples(model, image_coord, inv_intrinsics, parts, tri, feat_cl,
                                                    model._mlp_pack(z_rend.detach()), Nc, Nf, render_scale, bins, seed)
        live = t["ray_validity"].to(torch.float32) if B == 1 else None         # rendering.py:107-110
    frames = torch.cat([pose_to_camera[:, :, :3, :3], pose_to_camera[:, :, :3, 3:] * cs], dim=-1)
    density, color = model.query_posable(fine_points, frames, model_input)
    rc, rm, rd, w = composite_fine(density.reshape(B, n, Nf), color.reshape(B, 3, n, Nf), fine_depth, render_scale)
    if live is not None:
        rc, rm, rd = rc * live[:, None], rm * live, rd * live
    if not hasattr(model, "buffers_tensors"):
        model.buffers_tensors = {}
    model.buffers_tensors.update(bins=t["bins"], fine_depth=fine_depth[:, None], fine_weights=w.detach()[:, None],
                                 fine_points=fine_points)
    return rc, rm, rd


def _march_taps(model, image_coord, inv_intrinsics, parts, tri, feat_cl, pack, Nc, Nf, render_scale, seed, flags):
    """One renderer batch on the rays of one camera, with its taps: (fine_depth (B, n, Nf), fine_density (B, n, Nf),
    fine_color (B, 3, n, Nf), ray_validity (B, n) uint8, mask (B, n)) of the B images of `parts`."""
    B, n = parts.shape[0], image_coord.shape[-1]
    coord = image_coord.reshape(1, 3, n).expand(B, -1, -1)
    Ki = inv_intrinsics.reshape(-1, 3, 3)[:1].expand(B, -1, -1)
    out = ops.render_fwd(coord, Ki, parts, model.canonical_pose, tri, feat_cl, pack, Nc, Nf, render_scale=render_scale,
                         seed=seed, mlp_mode=model.mlp_mode, debug=True, **flags)
    t = out.taps
    return out.fine_depth[:, 0], t["fine_density"], t["fine_color"], t["ray_validity"], out.mask


def composite_marches(model, marches, axis: int, render_scale: float = 1, threshold: float = 0.5):
    """The taps of several `_march_taps` batches to one image per frame, in one ops.scene_composite launch. axis = 0: the
    batches are groups of avatars of one frame, joined along the avatars; axis = 1: batch k holds avatar k in every
    frame. Returns (colour (F, 3, n), mask (F, n), disparity (F, n)) and leaves instance_mass (F, K, n), instance (F, n),
    skipped (F, n) and avatar_masks (F, K, n), the avatars' own masks, in model.buffers_tensors. One batch of one frame is
    passed on as it is, without a copy."""
    if axis == 0:
        join = (lambda ts: ts[0][None]) if len(marches) == 1 else (lambda ts: torch.cat(ts, dim=0)[None])
    else:
        join = lambda ts: torch.stack(ts, dim=1)
    depth, density, color, valid, masks = (join([m[i] for m in marches]) for i in range(5))
    res = ops.scene_composite(depth, density, color, valid, render_scale=render_scale, threshold=threshold)
    if not hasattr(model, "buffers_tensors"):
        model.buffers_tensors = {}
    model.buffers_tensors.update(instance_mass=res.instance_mass, instance=res.instance, skipped=res.skipped,
                                 avatar_masks=masks)
    return res.color, res.mask, res.disparity


def render_scene(model, image_coord: torch.Tensor, pose_to_camera: torch.Tensor, inv_intrinsics: torch.Tensor,
                 render_scale: float = 1, Nc: int = 64, Nf: int = 128, model_input: Dict = {},
                 avatars_per_batch: Optional[int] = None, seed: Optional[int] = None, threshold: float = 0.5,
                 _parts: Optional[torch.Tensor] = None, _pack: Optional[torch.Tensor] = None):
    """K avatars in front of one camera: image_coord (1, 1, 3, n) or (1, 3, n), pose_to_camera (K, P, 4, 4) part frames,
    one inv_intrinsics ((3, 3) or (1, 3, 3)); model_input is batched over the avatars (z, z_rend, bone_length and, when
    given, tri_plane_feature of K entries) -> colour (1, 3, n), mask (1, n), disparity (1, n) of the scene.

    The avatars are marched on the same rays by the fused march with its taps (ops.render_fwd(debug=True)) under no_grad
    and on the same `seed`, avatars_per_batch at a time (default: all K in one renderer batch; a batch shares its near / far
    planes and numbers its rays batch-wide, so with avatars_per_batch=1 every avatar's samples are exactly those of its
    own render() call). One ops.scene_composite launch then integrates the sum of the K media over the merged samples
    of every ray (include/enarf_scene.h), where pasting the K images over each other by mask is wrong: bodies that
    interleave in depth, soft silhouettes. Each avatar keeps its own samples; no avatar is queried at another's.
    model.buffers_tensors gets instance_mass (1, K, n), the share of the mask each avatar carries, instance (1, n) int32,
    the avatar of the largest share where mask >= threshold (else -1), skipped (1, n) int32, a bit for every avatar whose
    samples were unusable on the ray, and avatar_masks (1, K, n), the avatars' own masks. No gradient flows."""
    assert pose_to_camera.shape[1] == model.num_bone
    K = pose_to_camera.shape[0]
    per = K if avatars_per_batch is None else int(avatars_per_batch)
    if per < 1:
        raise ValueError(f"render_scene: avatars_per_batch {avatars_per_batch} < 1")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    if not hasattr(model, "buffers_tensors"):
        model.buffers_tensors = {}
    flags = model.kernel_flags()
    with torch.no_grad():
        parts = _parts_from_part_poses(model, pose_to_camera, model_input["bone_length"]) if _parts is None else _parts
        marches = []
        for a in range(0, K, per):
            b = min(a + per, K)
            mi = {k: (v[a:b] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == K else v)
                  for k, v in model_input.items()}
            tri, feat_cl = model._tri_plane_pair(mi)
            pack = model._mlp_pack(mi["z_rend"]) if _pack is None else _pack[a:b]
            marches.append(_march_taps(model, image_coord, inv_intrinsics, parts[a:b], tri, feat_cl, pack, Nc, Nf,
                                       render_scale, seed, flags))
        return composite_marches(model, marches, 0, render_scale, threshold)


def render_scene_posable(model, image_coord: torch.Tensor, pose_to_camera: torch.Tensor, inv_intrinsics: torch.Tensor,
                         render_scale: float = 1, Nc: int = 64, Nf: int = 128, model_input: Dict = {},
                         avatars_per_batch: Optional[int] = None, seed: Optional[int] = None,
                         bins: Optional[torch.Tensor] = None):
    """render_scene for poses that require gradients: the arguments of render_scene, with pose_to_camera (K, P, 4, 4) part
    frames and model_input["bone_length"] that may require gradients; `bins` (K, n, Nf) gives the importance samples
    -> colour (1, 3, n), mask (1, n), disparity (1, n) of the scene, differentiable with respect to pose_to_camera and
    bone_length, and to the tri-planes, z_rend and the StyledMLP where they require gradients.

    Contract: render_posable's, the gradient of the image AT FIXED SAMPLE POSITIONS. The K avatars are marched on the same
    rays under no_grad (avatars_per_batch at a time, as render_scene marches them), which fixes every ray's depth
    range, its validity and its importance samples; every avatar's fine points and fine depths are formed from them as
    render_posable forms them and are constants. One model.query_posable call on the K avatars as a batch carries the
    gradient to the articulation, and ops.scene_composite_posable (the forward of render_scene's composite, its
    backward one launch of libenarf_sgrad.so) composes the K sample lists: where bodies interleave in depth, each
    avatar's gradient sees the other's occlusion. The forward values are render_scene's on the same seed up to the
    difference between the march's own taps and query_posable's outputs (fp32 rounding). model.buffers_tensors gets
    instance_mass (1, K, n), which carries the gradient as well, instance (1, n) int32 and skipped (1, n) int32 at a
    threshold of 0.5, fine_points (K, 3, n Nf), fine_depth (K, 1, n, Nf) and bins."""
    assert pose_to_camera.shape[1] == model.num_bone
    K, n = pose_to_camera.shape[0], image_coord.shape[-1]
    per = K if avatars_per_batch is None else int(avatars_per_batch)
    if per < 1:
        raise ValueError(f"render_scene_posable: avatars_per_batch {avatars_per_batch} < 1")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    cs = model.coordinate_scale
    coord = image_coord.reshape(1, 3, n)
    Ki = inv_intrinsics.reshape(-1, 3, 3)[:1]
    with torch.no_grad():
        parts = _parts_from_part_poses(model, pose_to_camera.detach(), model_input["bone_length"].detach())
        taps = []
        for a in range(0, K, per):
            b = min(a + per, K)
            mi = {k: (v.detach()[a:b] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == K else v)
                  for k, v in model_input.items()}
            tri, feat_cl = model._tri_plane_pair(mi)
            t, points, depth = _fixed_samples(model, coord.expand(b - a, -1, -1), Ki.expand(b - a, -1, -1), parts[a:b], tri,
                                              feat_cl, model._mlp_pack(mi["z_rend"]), Nc, Nf, render_scale,
                                              None if bins is None else bins[a:b], seed)
            taps.append((points, depth, t["ray_validity"], t["bins"]))
        fine_points, fine_depth, valid, bins_used = (torch.cat([t[i] for t in taps], dim=0) for i in range(4))
    frames = torch.cat([pose_to_camera[:, :, :3, :3], pose_to_camera[:, :, :3, 3:] * cs], dim=-1)
    density, color = model.query_posable(fine_points, frames, model_input)
    density, color = density.reshape(1, K, n, Nf), color.reshape(1, K, 3, n, Nf)
    rc, rm, rd, mass = ops.scene_composite_posable(fine_depth[None], density, color, valid[None], render_scale)
    with torch.no_grad():
        owner = ops.scene_composite(fine_depth[None], density.detach(), color.detach(), valid[None],
                                    render_scale=render_scale, want=("instance", "skipped"))
    if not hasattr(model, "buffers_tensors"):
        model.buffers_tensors = {}
    model.buffers_tensors.update(instance_mass=mass, instance=owner.instance, skipped=owner.skipped, bins=bins_used,
                                 fine_depth=fine_depth[:, None], fine_points=fine_points)
    return rc, rm, rd
