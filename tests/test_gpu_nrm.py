"""GPU tests of libenarf_nrm.so (nrm_gradient_kernel, nrm_ray_kernel) and the interface over it. The gradient is held to
the float64 referee of tests/pgrad_reference.py with the upstream gd = ones, gc = None (tests/nrm_reference.py), on the
scene and the points of tests/test_gpu_pgrad.py: Scene(32, 2), 23 parts, points drawn around the part centres; the bound
is tests/grad_referee.py's, every entry to its own scale, and the exclusion rule and its cap are pgrad_reference's. The
ray kernel is held to the float64 numpy restatement of its contract on seeded inputs. A referee is computed once per mode
and shared."""
import functools
import json
import struct

import numpy as np
import pytest
import torch

import geom_reference as GR
import nrm_reference as NR
import pgrad_reference as PR
from _helpers import DeviceScene, Scene, assert_close

pytestmark = pytest.mark.gpu
N_ALL = 1000
SIZES = (1, 64, 65, 300)            # a lone lane, a full wave, a wave and one lane, a ragged second workgroup


@functools.lru_cache(maxsize=None)
def _scene():
    sc = Scene(32, 2)
    return sc, DeviceScene(sc)


@functools.lru_cache(maxsize=None)
def _points():
    return PR.scene_points(_scene()[0], N_ALL)


@functools.lru_cache(maxsize=None)
def _referee(mode):
    return NR.gradient_referee(_scene()[0], _points(), mode)


def _kernel(mode, pts):
    from enarf_gan_amd import ops
    _, ds = _scene()
    out = ops.field_gradient(pts.contiguous().to(ds.dev), ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, **PR.MODES[mode][1])
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------- the gradient kernel
@pytest.mark.parametrize("mode,n", [(m, N_ALL) for m in PR.MODES] + [("default", n) for n in SIZES])
def test_gradient_matches_the_float64_referee(mode, n):
    ref, ones = _referee(mode)
    r = ref.grads(ones, None, n)
    density, gradient = _kernel(mode, _points()[:, :, :n])
    assert density.shape == (2, n) and gradient.shape == (2, 3, n) and gradient.dtype == torch.float32
    full = torch.zeros(2, 3, N_ALL)
    full[:, :, :n] = gradient.cpu() * ref.keep[:, None, :n]         # the referee's gradient is zero at an excluded point
    worst = PR.check({"g_points": full}, r, f"{mode}, N = {n}", ("g_points",))
    print(f"{mode}, N = {n}: excluded {ref.excluded * 100:.2f} %, worst ratio to the bound {worst}")
    assert float(gradient.abs().max()) > 0.0


@pytest.mark.parametrize("mode", list(PR.MODES))
def test_density_matches_query_fwd(mode):
    """the density returned beside the gradient is query_fwd's in mode f32, to the forward parity bound; where the query's
    density is zero the gradient is an exact zero (the density head is off there, or no cube holds the point)"""
    _, ds = _scene()
    density, gradient = _kernel(mode, _points())
    den, _ = ds.query(_points(), mlp_mode="f32", **PR.MODES[mode][1])
    torch.cuda.synchronize()
    assert float(den.max()) > 0.0
    assert_close(density.cpu(), den[:, 0].cpu(), f"density vs query_fwd, {mode}", 1e-4)
    off = (density == 0)[:, None].expand(-1, 3, -1)
    assert not bool(gradient[off].any())


def test_points_outside_every_cube_get_exact_zeros():
    from enarf_gan_amd import ops
    sc, ds = _scene()
    pts = PR.outside_points(sc, 300)
    assert not bool(PR.forward(sc, pts, torch.float32, "default")["decisions"]["valid"].any())
    for mode in PR.MODES:
        density, gradient = _kernel(mode, pts)
        assert not bool(density.any()) and not bool(gradient.any()), mode
        assert not bool(torch.signbit(gradient).any()), mode                                    # +0, not -0
    density, gradient = ops.field_gradient(pts[:, :, :0].to(ds.dev), ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack)
    assert density.shape == (2, 0) and gradient.shape == (2, 3, 0)                               # N = 0: no launch


def _ray_kernel(c, **kw):
    from enarf_gan_amd import ops
    d = lambda k: torch.from_numpy(np.array(c[k])).cuda()
    out = ops.ray_normals(d("gradient"), d("weights"), d("mask"), fallback=d("fallback"), flags=d("flags"), points=d("points"),
                          want_magnitude=True, **kw)
    torch.cuda.synchronize()
    return out


def test_two_runs_give_equal_bits():
    for mode in ("default", "multiply_density_with_weight"):
        a, b = _kernel(mode, _points()), _kernel(mode, _points())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), mode
    c = NR.ray_case(300, 64)
    a, b = _ray_kernel(c, shade="lit"), _ray_kernel(c, shade="lit")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------- the ray kernel
def _check_ray_normals(got, ref, n, shade, what):
    """a RayNormals (B = 2) against nrm_reference.ray_normals' dict; the magnitude unless the call left it out (`magnitude`
    None), the image when `shade` is given"""
    assert got.normals.shape == (2, n, 3) and got.flags.dtype == torch.uint8
    assert np.array_equal(got.flags.cpu().numpy(), ref["flags"]), what
    un = GR.ulps_from(got.normals.cpu().numpy(), ref["normals"])
    um = np.zeros(1) if got.magnitude is None else GR.ulps_from(got.magnitude.cpu().numpy(), ref["magnitude"])
    assert got.magnitude is None or got.magnitude.shape == (2, n)
    print(f"{what}: normals {un.max():.0f} ulp ({(un > 0).sum()} off), magnitude {um.max():.0f} ulp, "
          f"{int((ref['flags'] & 4 > 0).sum())} of {2 * n} field normals")
    assert un.max() <= 1 and um.max() <= 1, what
    if shade is None:
        assert got.image is None
        return
    d = np.abs(got.image.cpu().numpy().astype(np.int16) - ref["image"].astype(np.int16))
    assert got.image.dtype == torch.uint8 and d.max() <= 1, what


@pytest.mark.parametrize("n,Nf", NR.RAY_CASES)
def test_ray_normals_match_the_referee(n, Nf):
    """B = 2 on nrm_reference.ray_case's inputs: rays with all-zero weights, a zero gradient, a mask below the threshold and
    a fallback whose flag bit 1 is set or clear. min_gradient = 0 and every ray's |G| is either of order 1 or exactly 0, so
    no ray is borderline. Flags equal; normals and magnitude the referee rounded to fp32, or one step from it (the same
    fp64 operations in the same order on both sides; only the last place of one can differ and move one rounding); image
    within one level on every pixel, the rule tests/test_gpu_geom.py applies to geometry_buffers' image."""
    c = NR.ray_case(n, Nf)
    assert n == 1 or (all((c["kind"] == k).any() for k in range(5)) and len(set(c["flags"].reshape(-1).tolist())) == 3)
    for kw in (dict(shade="normal"), dict(shade="lit", background=(0.1, 0.2, 0.3)), dict(shade=None, mask_threshold=0.05)):
        got = _ray_kernel(c, **kw)
        ref = NR.ray_normals(c["gradient"], c["weights"], c["mask"], c["fallback"], c["flags"], c["points"], **kw)
        assert got.magnitude is not None
        _check_ray_normals(got, ref, n, kw["shade"], f"n = {n}, Nf = {Nf}, {kw}")
    field = (ref["flags"] & 4) > 0                           # the last setting: every mask passes, so the kinds decide
    assert np.array_equal(field, np.isin(c["kind"], (0, 3, 4)))
    # without a fallback the same rays have a field normal and the others are zeros
    from enarf_gan_amd import ops
    bare = ops.ray_normals(*(torch.from_numpy(np.array(c[k])).cuda() for k in ("gradient", "weights", "mask")), mask_threshold=0.05)
    assert np.array_equal(bare.flags.cpu().numpy(), field.astype(np.uint8) * 4) and bare.magnitude is None and bare.image is None
    assert not bool(bare.normals.cpu()[torch.from_numpy(~field)].any())


def test_ray_normals_take_the_shapes_of_a_march():
    """(B, 1, n, Nf - 1) weights as the march returns them and a (B, H, W) mask give (B, H, W[, 3]) outputs with the same bits"""
    from enarf_gan_amd import ops
    c = NR.ray_case(64, 33)
    d = lambda k: torch.from_numpy(np.array(c[k])).cuda()
    flat = ops.ray_normals(d("gradient"), d("weights"), d("mask"), shade="normal")
    grid = ops.ray_normals(d("gradient"), d("weights")[:, None], d("mask").reshape(2, 8, 8), shade="normal")
    assert grid.normals.shape == (2, 8, 8, 3) and grid.flags.shape == (2, 8, 8) and grid.image.shape == (2, 8, 8, 3)
    assert torch.equal(grid.normals.reshape(2, 64, 3), flat.normals) and torch.equal(grid.image.reshape(2, 64, 3), flat.image)
    empty = ops.ray_normals(d("gradient")[:, :, :0], d("weights")[:, :0], d("mask")[:, :0])           # n = 0: no launch
    assert empty.normals.shape == (2, 0, 3) and empty.flags.shape == (2, 0)


# ------------------------------------------------------------------------------------------------- the model's entry points
def _model():
    from test_gpu_paint import _model
    return _model()


def test_render_geometry_with_field_normals_is_its_four_launches():
    """32 x 32 at Nc 24 / Nf 32: normals="field" equals, bit for bit, _fixed_samples + ops.field_gradient +
    ops.geometry_buffers + ops.ray_normals called by hand on the same seed; colour, mask, depth and points are those of
    normals="stencil", which equals a call without the keyword"""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.rendering import _fixed_samples
    gen, s, z, pose, bl, K, _ = _model()
    nerf, S, psi = gen.nerf, gen.size, 0.4
    K_inv = torch.linalg.inv_ex(K.float()).inverse
    for shade, kw in (("normal", dict()), ("lit", dict(edge=0.1, background=0.0)), ("depth", dict(near=1.0, far=6.0))):
        torch.manual_seed(7)
        image, buffers, color, mask = gen.render_geometry(pose, bl, z, K_inv, truncation_psi=psi, shade=shade, normals="field", **kw)
        torch.manual_seed(7)
        s_image, s_buffers, s_color, s_mask = gen.render_geometry(pose, bl, z, K_inv, truncation_psi=psi, shade=shade,
                                                                  normals="stencil", **kw)
        torch.manual_seed(7)
        plain = gen.render_geometry(pose, bl, z, K_inv, truncation_psi=psi, shade=shade, **kw)
        assert torch.equal(plain[0], s_image) and torch.equal(plain[2], s_color) and torch.equal(plain[3], s_mask)
        assert all(torch.equal(getattr(plain[1], k), getattr(s_buffers, k)) for k in s_buffers._fields)
        assert torch.equal(color, s_color) and torch.equal(mask, s_mask)
        assert torch.equal(buffers.depth, s_buffers.depth) and torch.equal(buffers.points, s_buffers.points)
        assert image.data_ptr() == buffers.image.data_ptr() and image.shape == (1, S, S, 3) and image.dtype == torch.uint8

        torch.manual_seed(7)
        z_nerf, z_render, _ = gen._latent_parts(z)
        parts, pack = ops.prepare(pose, bl, nerf.canonical_bone_length, z_render, nerf.mlp.as_dict(), nerf.parent_id,
                                  nerf.origin_location, nerf.coordinate_scale)
        idx = torch.arange(S * S, device="cuda")
        x, y = (idx % S + 0.5).float(), (torch.div(idx, S, rounding_mode="floor") + 0.5).float()
        pixels = torch.stack([x, y, torch.ones_like(x)], dim=0)[None, None].contiguous()
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        with torch.no_grad():
            tri, feat_cl = nerf._tri_plane_pair({"z": z_nerf, "z_rend": z_render, "bone_length": bl, "truncation_psi": psi})
            _, fine_points, _, out = _fixed_samples(nerf, pixels, K_inv, parts, tri, feat_cl, pack, 24, 32, 1, None, seed,
                                                    with_outputs=True)
            _, gradient = ops.field_gradient(fine_points, parts, nerf.canonical_pose, tri, feat_cl, pack, **nerf.kernel_flags())
            want = ops.geometry_buffers(out.disparity * nerf.coordinate_scale, out.mask, K_inv, size=(S, S), shade=shade, **kw)
            bg = {k: kw[k] for k in ("background",) if k in kw}
            field = ops.ray_normals(gradient, out.fine_weights, out.mask.reshape(1, S, S), fallback=want.normals,
                                    flags=want.flags, points=want.points, shade=None if shade == "depth" else shade, **bg)
        assert torch.equal(out.color.reshape(1, 3, S, S), color) and torch.equal(out.mask.reshape(1, S, S), mask)
        assert torch.equal(buffers.depth, want.depth) and torch.equal(buffers.points, want.points)
        assert torch.equal(buffers.normals, field.normals) and torch.equal(buffers.flags, field.flags), shade
        assert torch.equal(image, want.image if shade == "depth" else field.image), shade
    flags = buffers.flags.cpu().numpy()
    has_field = (flags & 4) > 0
    assert has_field.sum() > 0.5 * (flags & 1).sum() > 0 and not (has_field & ((flags & 1) == 0)).any()
    n = buffers.normals.cpu().numpy()[has_field]
    assert np.allclose(np.linalg.norm(n, axis=-1), 1, rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="normals"):
        gen.render_geometry(pose, bl, z, K_inv, normals="mesh")
    with pytest.raises(ValueError, match="cannot be passed"):
        gen.render_geometry(pose, bl, z, K_inv, normals="field", want=("depth",))


def test_render_field_normals_and_the_model_gradient_entry_point():
    """render_field_normals: colour, mask and disparity are render()'s on the same seed; the normals are ray_normals of the
    buffers it leaves behind. TriPlaneNARF.field_gradient equals ops.field_gradient and refuses inputs that want a gradient."""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.rendering import render, render_field_normals
    sc, ds = _scene()
    from test_gpu_pgrad import _model as narf_model
    m = narf_model(sc)
    s = sc.raw
    coord = s["image_coord"][..., 32 * 13:32 * 13 + 64].contiguous().cuda()
    mi = {"z": None, "z_rend": s["z_rend"].cuda(), "bone_length": sc.bl_parts.cuda(), "tri_plane_feature": ds.tri}
    args = (m, coord, sc.pose_parts.cuda(), s["inv_intrinsics"].cuda())
    with torch.no_grad():
        c0, m0, d0 = render(*args, Nc=24, Nf=32, model_input=mi, seed=11)
        c1, m1, d1, nrm = render_field_normals(*args, Nc=24, Nf=32, model_input=mi, seed=11, shade="normal", want_magnitude=True)
    assert torch.equal(c0, c1) and torch.equal(m0, m1) and torch.equal(d0, d1) and float(m0.max()) > 0.5
    bt = m.buffers_tensors
    again = ops.ray_normals(bt["fine_gradient"], bt["fine_weights"], m1, shade="normal", want_magnitude=True)
    assert all(torch.equal(a, b) for a, b in zip(nrm, again)) and int((nrm.flags & 4 > 0).sum()) > 0
    with torch.no_grad():
        den, grad = m.field_gradient(bt["fine_points"], sc.pose_scaled.cuda(), mi)
    assert torch.equal(grad, bt["fine_gradient"]) and torch.equal(den[:, None], bt["fine_density"])
    assert not grad.requires_grad and any(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError):                      # with gradients enabled the field's parameters want one
        m.field_gradient(bt["fine_points"], sc.pose_scaled.cuda(), mi)
    with pytest.raises(NotImplementedError):
        render_field_normals(*args, Nc=24, Nf=32, model_input=mi)


def test_mesh_normals_paint_and_export(tmp_path):
    """on the small mesh of the paint tests: extract_mesh(return_normals=True) returns unit vectors (or zeros), equal to
    field_normals on the returned vertices, also after simplification; paint_mesh(normals="field") is shade_fragments fed
    the buffer built by hand; normals="mesh" is a call without the keyword; export_glb carries the normals"""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import export_glb, field_normals, paint_mesh
    gen, s, z, pose, bl, K, mesh = _model()
    nerf = gen.nerf
    z_nerf, z_render, _ = gen._latent_parts(z)
    field = nerf.mesh_field(pose, z_nerf, z_render, bl, 0.4)
    for extra in (dict(), dict(simplify_cell=0.1)):
        v, t, colors, normals = gen.extract_mesh(pose, z, bl, **mesh, **extra, return_colors=True, return_normals=True)
        pv, pt = gen.extract_mesh(pose, z, bl, **mesh, **extra)
        assert torch.equal(v, pv) and torch.equal(t, pt) and normals.shape == v.shape and normals.dtype == torch.float32
        length = torch.linalg.vector_norm(normals, dim=1)
        unit = length > 0
        assert float(unit.float().mean()) > 0.5 and float((length[unit] - 1).abs().max()) < 1e-5
        assert torch.equal(normals, field_normals(*field[:2], v, field[2]))
    fb = torch.nn.functional.normalize(torch.randn(len(v), 3, device="cuda"), dim=1)
    with_fb = field_normals(*field[:2], v, field[2], fallback=fb)
    assert torch.equal(with_fb[unit], normals[unit]) and torch.equal(with_fb[~unit], fb[~unit])
    all_fb = field_normals(*field[:2], v, field[2], fallback=fb, min_gradient=float("inf"))
    assert torch.equal(all_fb, fb)

    frag, painted = paint_mesh(v, t, K, gen.size, vertex_colors=colors, normals="field", field=field)
    covered = frag.pix_to_face >= 0
    points = (frag.bary[..., None] * v[t[frag.pix_to_face.clamp(min=0)]]).sum(dim=-2)
    hand = field_normals(*field[:2], points.reshape(-1, 3), field[2], fallback=frag.normals.reshape(-1, 3)).reshape(frag.normals.shape)
    hand = torch.where(covered[..., None], hand, frag.normals).contiguous()
    want = ops.shade_fragments(frag.pix_to_face, frag.bary, hand, v, t, vertex_colors=colors)
    assert torch.equal(painted.image, want.image) and bool(covered.any())      # (that the normals matter is shown below)
    _, by_mesh = paint_mesh(v, t, K, gen.size, vertex_colors=colors, normals="mesh")
    _, plain = paint_mesh(v, t, K, gen.size, vertex_colors=colors)
    assert torch.equal(by_mesh.image, plain.image) and not torch.equal(plain.image, painted.image)
    img, _ = gen.render_colored_mesh(pose, K, z, bl, **mesh, normals="field")
    img_mesh, _ = gen.render_colored_mesh(pose, K, z, bl, **mesh)
    assert img.shape == (512, 512, 3) and not np.array_equal(img, img_mesh)
    with pytest.raises(ValueError):
        paint_mesh(v, t, K, gen.size, vertex_colors=colors, normals="field")
    with pytest.raises(ValueError):
        paint_mesh(v, t, K, gen.size, vertex_colors=colors, normals="stencil")

    rig = gen.extract_rigged_mesh(pose, z, bl, **mesh)
    rn = field_normals(*field[:2], rig.vertices, field[2])
    a, b, c = (str(tmp_path / f"{k}.glb") for k in "abc")
    export_glb(rig, a)
    export_glb(rig, b, normals=None)
    export_glb(rig, c, normals=rn)
    assert open(a, "rb").read() == open(b, "rb").read()
    raw = open(c, "rb").read()
    n_json = struct.unpack("<I", raw[12:16])[0]
    doc, binary = json.loads(raw[20:20 + n_json]), raw[28 + n_json:]
    acc = doc["accessors"][doc["meshes"][0]["primitives"][0]["attributes"]["NORMAL"]]
    view = doc["bufferViews"][acc["bufferView"]]
    assert acc["count"] == len(rig.vertices) and acc["type"] == "VEC3"
    assert binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]] == rn.cpu().numpy().tobytes()


def test_the_other_entry_points_take_field_normals():
    """render_geometry_animation(normals="field") at frames_per_batch = 1 is render_geometry(normals="field") frame by frame,
    byte for byte; render_textured_mesh(normals="field") is paint_textured_mesh of its own pieces; the turntable takes the
    keyword and shades every frame differently from the mesh normals"""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import paint_textured_mesh
    from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle
    gen, s, z, pose, bl, K, mesh = _model()
    S, num, psi = gen.size, 2, 0.4
    first = s["pose_to_camera"][:1]
    keys = torch.cat([first, rotate_pose_by_angle(first, torch.tensor([0.7]))]).double().cuda()
    torch.manual_seed(5)
    frames, depth, poses = gen.render_geometry_animation(keys, bl, K, z, num=num, loop=False, truncation_psi=psi,
                                                         frames_per_batch=1, shade="lit", normals="field")
    assert frames.shape == (num, S, S, 3) and frames.dtype == torch.uint8 and depth.shape == (num, S, S)
    K_inv = torch.linalg.inv_ex(K.float()).inverse
    torch.manual_seed(5)
    for f in range(num):
        image, buffers, _, _ = gen.render_geometry(poses[f:f + 1].float(), bl, z, K_inv, truncation_psi=psi, shade="lit", normals="field")
        assert torch.equal(frames[f], image[0]) and torch.equal(depth[f], buffers.depth[0]), f"frame {f}"
    torch.manual_seed(5)
    stencil = gen.render_geometry_animation(keys, bl, K, z, num=num, loop=False, truncation_psi=psi, frames_per_batch=1, shade="lit")
    assert torch.equal(stencil[1], depth) and not torch.equal(stencil[0], frames)
    with pytest.raises(ValueError, match="normals"):
        gen.render_geometry_animation(keys, bl, K, z, num=num, loop=False, normals="mesh")

    img, (v, t, atlas) = gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=256, normals="field")
    img_mesh, (mv, mt, _) = gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=256)
    assert torch.equal(v, mv) and torch.equal(t, mt) and not np.array_equal(img, img_mesh)
    z_nerf, z_render, _ = gen._latent_parts(z)
    _, want = paint_textured_mesh(v, t, atlas, K, S, normals="field", field=gen.nerf.mesh_field(pose, z_nerf, z_render, bl, 0.4))
    assert np.array_equal(img, want.image.cpu().numpy())

    angles = [0.0, 0.9]
    by_field = gen.render_mesh_turntable(pose, K, z, bl, angles, **mesh, render_size=96, normals="field")
    by_mesh = gen.render_mesh_turntable(pose, K, z, bl, angles, **mesh, render_size=96)
    assert by_field.shape == by_mesh.shape == (2, 96, 96, 3) and by_field.dtype == torch.uint8
    assert not torch.equal(by_field[0], by_mesh[0]) and not torch.equal(by_field[1], by_mesh[1])
    assert torch.equal(by_field[:, 0, 0], by_mesh[:, 0, 0])                                     # the corner pixel: background
