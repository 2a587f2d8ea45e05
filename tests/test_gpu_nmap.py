"""GPU tests of the normal maps (libenarf_nmap.so): nmap_encode_kernel and nmap_shade_kernel against the float64 numpy
restatement of their contracts (tests/nmap_reference.py) on the hand meshes of tests/bake_cases.py, the hand fragment buffer
and the 33^3 sphere of tests/paint_cases.py; what the map exists for (a constant field comes back as itself from any pixel,
also on a rigidly moved mesh; a flat map is the face normal); determinism; the model-level entry points; and every launching
function on poisoned, guard-banded allocations (tests/nmap_poison_cases.py). The referee reads the very buffers the kernels
read, so no texel and no pixel is left out of any comparison. tests/test_nmap_cpu.py shows that the bounds used here see a
missing sign flip, a swapped bitangent and a decode without its shift."""
import contextlib

import numpy as np
import pytest
import torch

import bake_cases as BC
import nmap_cases as NC
import nmap_poison_cases as NP
import nmap_reference as NR
import paint_cases as PC
import poison_cases
from libraries import binding
from poison import poisoned
from test_gpu_bake import SPHERE_ATLAS, TEXTURE, _mesh_pieces, _sphere_atlas
from test_gpu_paint import _buffers, _check, _dev, _model

pytestmark = pytest.mark.gpu

GEO = ("pix_to_face", "bary", "normals", "vertices", "triangles")


def _np(t):
    return t.cpu().numpy()


def _encode(face, vec, v, t, **kw):
    from enarf_gan_amd import ops
    out = ops.encode_normal_map(_dev(face), _dev(vec), _dev(v), _dev(t), **kw)
    torch.cuda.synchronize()
    assert out._fields == ("texture", "texture_f32")
    return _np(out.texture), None if out.texture_f32 is None else _np(out.texture_f32)


def _shade(h, normal_texture, texture=None, **kw):
    from enarf_gan_amd import ops
    out = ops.shade_normal_mapped(*(_dev(h[k]) for k in GEO), _dev(normal_texture), None if texture is None else _dev(texture), **kw)
    torch.cuda.synchronize()
    assert out._fields == ("image", "albedo", "normal", "shaded")
    return {k: _np(getattr(out, k)) for k in out._fields}


# ------------------------------------------------------------------------------------------------- the kernels alone
def _check_encoded(tex, f32, ref, what):
    """encode's texture (and its fp32 map, or None) as numpy against nmap_reference.encode's: the bytes equal, the fp32 map
    the referee rounded to fp32 to within one fp32 step of 1"""
    shape = ref["flat"].shape
    assert tex.shape == shape + (4,) and tex.dtype == np.uint8 and (f32 is None or (f32.shape == shape + (3,) and f32.dtype == np.float32))
    d = np.zeros(1) if f32 is None else np.abs(f32.astype(np.float64) - ref["texture_f32"].astype(np.float32).astype(np.float64))
    print(f"{what}: {(tex != ref['texture']).sum()} bytes differ, fp32 map off by {d.max():.2e} at the most ({(d > 0).sum()} values)")
    assert np.array_equal(tex, ref["texture"])
    assert d.max() <= NC.F32_BOUND


@pytest.mark.parametrize("case", NC.ENCODE_CASES, ids=str)
def test_encode_matches_the_referee_on_every_texel(case):
    """every texel of (T, A) = (1, 6), (5, 21), (8, 12) and of the sphere at 380; vectors with NaN, +-inf, exact zeros and
    lengths on both sides of min_length; the 5-triangle mesh names vertex V and vertex -1. Both signs of `negate`."""
    (v, t), A = NC.mesh(case)
    face, vec = NC.texel_face(case), NC.vectors(case)
    for kw in (dict(min_length=NC.MIN_LENGTH), dict(negate=False)):
        tex, f32 = _encode(face, vec, v, t, want_float=True, **kw)
        ref = NR.encode(face, vec, v, t, **kw)
        _check_encoded(tex, f32, ref, f"{case} {kw}")
        assert (tex[face < 0] == [128, 128, 255, 0]).all() and (f32[face < 0] == [0, 0, 1]).all()
        assert (tex[ref["flat"]] == [128, 128, 255, 255]).all() and (f32[ref["flat"]] == [0, 0, 1]).all()
        assert (tex[face >= 0][:, 3] == 255).all() and ref["flat"].sum() > 0
    # owners a caller could hand over: T, beyond T, a triangle that names vertex V or -1
    if case == (5, 21):
        odd = np.array([[0, 5, 8, 3, 4, -1, 2]], np.int32)
        ones = np.ones((3, 7), np.float32)
        tex, f32 = _encode(odd, ones, v, t, want_float=True)
        _check_encoded(tex, f32, NR.encode(odd, ones, v, t), "owners outside the mesh")
        assert (tex[0, 1:5] == [128, 128, 255, 255]).all()


def test_encode_bands_stitch_count_zero_and_two_runs_agree():
    from enarf_gan_amd import ops
    for case, cuts in (((5, 21), (0, 7, 8, 21)), ("sphere", (0, 100, 101, 379, 380))):
        (v, t), A = NC.mesh(case)
        face, vec = NC.texel_face(case), NC.vectors(case)
        whole = _encode(face, vec, v, t, want_float=True, min_length=NC.MIN_LENGTH)
        again = _encode(face, vec, v, t, want_float=True, min_length=NC.MIN_LENGTH)
        assert whole[0].tobytes() == again[0].tobytes() and whole[1].tobytes() == again[1].tobytes()
        given = (torch.zeros(A, A, 4, dtype=torch.uint8, device="cuda"), torch.zeros(A, A, 3, device="cuda"))
        planes = vec.reshape(3, A, A)
        for a, b in zip(cuts[:-1], cuts[1:]):
            band = np.ascontiguousarray(planes[:, a:b].reshape(3, -1))
            back = ops.encode_normal_map(_dev(face[a:b]), _dev(band), _dev(v), _dev(t), min_length=NC.MIN_LENGTH,
                                         out=(given[0][a:b], given[1][a:b]))
            assert back.texture.data_ptr() == given[0][a:b].data_ptr()
        assert _np(given[0]).tobytes() == whole[0].tobytes() and _np(given[1]).tobytes() == whole[1].tobytes()
        assert _encode(face, vec, v, t)[1] is None
    # no texel: nothing is launched, nothing fails; no triangle: every texel of an atlas is empty
    v, t = BC.hand_mesh(5)
    none = ops.encode_normal_map(torch.zeros(0, 21, dtype=torch.int32, device="cuda"), torch.zeros(3, 0, device="cuda"), _dev(v),
                                 _dev(t), want_float=True)
    assert none.texture.shape == (0, 21, 4) and none.texture_f32.shape == (0, 21, 3)
    tex, f32 = _encode(np.full((3, 9), -1, np.int32), np.full((3, 27), np.nan, np.float32), np.zeros((0, 3), np.float32),
                       np.zeros((0, 3), np.int64), want_float=True)
    assert (tex == [128, 128, 255, 0]).all() and (f32 == [0, 0, 1]).all()
    tex, _ = _encode(np.zeros((3, 9), np.int32), np.ones((3, 27), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    assert (tex == [128, 128, 255, 255]).all()


def _check_shaded(got, ref, what):
    """albedo, shaded and image within test_gpu_paint._check's bounds; normal within two fp32 steps of 1 per component of
    the referee, NaN where the referee is (a stored normal the kernel passes through)"""
    _check(got, ref, what)
    assert got["normal"].dtype == np.float32 and got["normal"].shape == ref["normal"].shape
    nan = np.isnan(ref["normal"])
    assert np.array_equal(np.isnan(got["normal"]), nan), what
    d = np.abs(got["normal"].astype(np.float64) - ref["normal"])[~nan]
    print(f"{what}: normal off by {d.max():.2e} at the most, {ref['framed'].sum()} framed of {ref['drawn'].sum()} drawn pixels")
    assert d.max() <= NC.NORMAL_BOUND, what
    assert np.array_equal(got["normal"][~ref["drawn"]], ref["normal"][~ref["drawn"]].astype(np.float32), equal_nan=True)


def _albedos(tex8, tex32):
    return (("RGBA8 albedo", dict(texture=tex8)), ("fp32 albedo", dict(texture=tex32)),
            ("constant albedo", dict(base_color=(0.7, 0.6, 0.5))))


def test_hand_written_fragments_match_the_referee():
    """the 8 x 8 buffer of tests/paint_cases.py (face ids -1, T, T + 5, 2^40 and -7, triangles naming vertex V and vertex
    -1, a zero normal, a NaN barycentric) over random 16 x 16 normal maps of both kinds (the fp32 one with a zero cell, a
    NaN and an inf texel) x the three albedos, lit and not; and once more with a triangle that has no frame (|e1| = 0),
    whose pixels keep the stored normal"""
    h = PC.hand_buffer()
    geo = {k: h[k] for k in GEO}
    degenerate = dict(geo, triangles=np.array([[0, 1, 2], [3, 3, 5], [2, 1, 4], [0, 1, 6], [-1, 2, 3]], np.int64))
    for mesh, name in ((geo, "hand buffer"), (degenerate, "hand buffer, triangle 1 without a frame")):
        for nmap in NC.hand_normal_textures(16):
            for what, albedo in _albedos(*BC.hand_textures(16)):
                for lit in (True, False):
                    kw = dict(lit=lit, background=(0.1, 0.2, 0.3), **albedo)
                    got = _shade(mesh, nmap, **kw)
                    ref = NR.shade(**mesh, normal_texture=nmap, **kw)
                    assert ref["drawn"].sum() == 64 - 10
                    assert ref["framed"].sum() == (54 if mesh is geo else 54 - (mesh["pix_to_face"] == 1).sum())
                    _check_shaded(got, ref, f"{name}, {nmap.dtype} map, {what}, lit={lit}")
                    bg = np.float32([0.1, 0.2, 0.3])
                    assert (got["albedo"][~ref["drawn"]] == bg).all() and (got["image"][~ref["drawn"]] == [25, 51, 76]).all()
                    if "base_color" in albedo:
                        assert (got["albedo"][ref["drawn"]] == np.float32([0.7, 0.6, 0.5])).all()
    got = _shade(geo, NC.hand_normal_textures(16)[0])
    assert (got["albedo"][0, 0] == 1).all() and (got["image"][0, 0] == 255).all()                # the default background
    assert (got["albedo"][2, 0] == 1).all()                                                     # the default base colour


def test_unlit_normal_mapped_shade_equals_shade_textured_bit_for_bit():
    """nmap_shade_kernel and bake_shade_kernel find a fragment's texels through the one definition in csrc/enarf_shade.h
    (layout, uv, tap): on the 8 x 8 hand-written buffer, with the RGBA8 and the fp32 16 x 16 texture, an unlit
    shade_normal_mapped returns the image, albedo and shaded of shade_textured, bit for bit"""
    from enarf_gan_amd import ops
    h = PC.hand_buffer()
    geo = [_dev(h[k]) for k in GEO]
    nmap = _dev(NC.hand_normal_textures(16)[0])
    for tex in BC.hand_textures(16):
        kw = dict(lit=False, background=(0.1, 0.2, 0.3))
        mapped = ops.shade_normal_mapped(*geo, nmap, texture=_dev(tex), **kw)
        plain = ops.shade_textured(*geo, _dev(tex), **kw)
        torch.cuda.synchronize()
        for k in ("image", "albedo", "shaded"):
            a, b = _np(getattr(mapped, k)), _np(getattr(plain, k))
            print(f"{tex.dtype} texture, {k}: {(a.view(np.uint8) != b.view(np.uint8)).sum()} bytes differ")
            assert a.dtype == b.dtype and a.shape == b.shape == (8, 8, 3) and a.tobytes() == b.tobytes(), (tex.dtype, k)


def test_the_normal_mapped_sphere_matches_the_referee():
    """the rasterised sphere (R = 257: a partial last wavefront) at the atlas size tests/test_gpu_bake.py uses (510): random
    normal maps of both kinds x {RGBA8 albedo, fp32 albedo, constant}, lit and not, every pixel"""
    h = _buffers("sphere")
    _, tex8, tex32 = _sphere_atlas("sine")
    rng = np.random.default_rng(77)
    maps = (rng.integers(0, 256, (SPHERE_ATLAS, SPHERE_ATLAS, 4)).astype(np.uint8),
            rng.normal(0, 1, (SPHERE_ATLAS, SPHERE_ATLAS, 3)).astype(np.float32))
    for nmap in maps:
        for what, albedo in _albedos(tex8, tex32):
            for lit in (True, False):
                got = _shade(h, nmap, lit=lit, **albedo)
                ref = NR.shade(**h, normal_texture=nmap, lit=lit, **albedo)
                assert np.array_equal(ref["drawn"], h["pix_to_face"] >= 0) and ref["framed"].sum() == ref["drawn"].sum() > 10000
                _check_shaded(got, ref, f"sphere, {nmap.dtype} map, {what}, lit={lit}")
    again = _shade(h, maps[0], texture=tex8)
    assert all(again[k].tobytes() == _shade(h, maps[0], texture=tex8)[k].tobytes() for k in again)


# ------------------------------------------------------------------------------------------------- what the map is for
def _exact_motion(v):
    """tests/test_nmap_cpu.py's: a quarter turn about the camera's z axis and a step of -1/4 along z, exact in fp32 for
    vertices with 1 < z < 4, so the moved frame is the turned frame and not its fp32 rounding (a sliver's frame would
    otherwise turn by the rounding of its short edge, far above 1e-6)"""
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    moved = v.astype(np.float64) @ R.T + np.array([0.0, 0.0, -0.25])
    assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)
    return R, moved.astype(np.float32)


def test_a_constant_field_round_trips_on_the_device():
    """an fp32 map baked through bake_normal_map(normal_fn = a constant unit vector d) on the sphere: the normal output of
    every covered pixel is d within 1e-6; on rigidly moved vertices it is R d"""
    from enarf_gan_amd.libraries.NARF.mesh_rendering import bake_normal_map, paint_normal_mapped_mesh
    v, t = PC.sphere()
    d32 = NC.CONSTANT_D.astype(np.float32)
    field = lambda p: torch.from_numpy(d32).to(p.device).expand(p.shape[0], 3)
    atlas = bake_normal_map(None, None, _dev(v), _dev(t), size=SPHERE_ATLAS, normal_fn=field, want_float=True)
    assert (atlas.num_triangles, atlas.size, atlas.cell) == (len(t), SPHERE_ATLAS, 8) and atlas.texture_f32 is not None
    own = _np(atlas.texture[..., 3]) == 255
    assert own.mean() > 0.5 and (_np(atlas.texture)[~own] == [128, 128, 255, 0]).all()
    R = 257
    K, img = _dev(PC.intrinsics(R)).reshape(1, 3, 3), PC.CAMERAS[R][0]
    d = d32.astype(np.float64)
    d /= np.linalg.norm(d)
    Rm, moved = _exact_motion(v)
    for verts, want in ((v, d), (moved, Rm @ d)):
        frag, out = paint_normal_mapped_mesh(_dev(verts), _dev(t), atlas, K, img, R, lit=False, use_float=True)
        cov = _np(frag.pix_to_face) >= 0
        err = np.abs(_np(out.normal).astype(np.float64)[cov] - want).max()
        print(f"constant field on the sphere: {cov.sum()} covered pixels, normal off by {err:.2e} at the most")
        assert cov.sum() > 10000 and err < 1e-6
        assert torch.equal(out.normal[~torch.from_numpy(cov).cuda()], frag.normals[~torch.from_numpy(cov).cuda()])
        assert (_np(out.albedo)[cov] == 1).all()
    # the 8-bit map of the same field: within the quantisation of a byte, 1 / 255 a component before the renormalisation
    frag, out = paint_normal_mapped_mesh(_dev(v), _dev(t), atlas, K, img, R, lit=False)
    cov = _np(frag.pix_to_face) >= 0
    assert np.abs(_np(out.normal).astype(np.float64)[cov] - d).max() < 3 / 255          # |q - d| <= sqrt(3) / 255, then unit()


def test_a_flat_map_gives_the_face_normal():
    """the fp32 map (0, 0, 1) everywhere (the 8-bit flat value decodes to 1/255, not 0): the normal of every covered pixel
    is the unit face normal of the pixel's triangle within 1e-6"""
    h = _buffers("sphere")
    flat = np.zeros((SPHERE_ATLAS, SPHERE_ATLAS, 3), np.float32)
    flat[..., 2] = 1
    got = _shade(h, flat, lit=True)
    f = h["pix_to_face"]
    cov = f >= 0
    p = h["vertices"].astype(np.float64)[h["triangles"][f[cov]]]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    err = np.abs(got["normal"].astype(np.float64)[cov] - n).max()
    print(f"flat map on the sphere: {cov.sum()} covered pixels, normal off by {err:.2e} from the face normal")
    assert cov.sum() > 10000 and err < 1e-6


# ------------------------------------------------------------------------------------------------- the model's entry points
def test_bake_normal_map_is_its_launches_by_hand():
    """bake_points, field_gradient with field_normals' scaling, encode_normal_map: bit for bit, in one piece or in bands"""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import bake_normal_map
    from enarf_gan_amd.libraries.NeRF.rendering import _parts_from_part_poses
    gen, s, z, pose, bl, K, mesh = _model()
    _, pose_parts, model_input, v, t = _mesh_pieces()
    atlas = gen.bake_normal_map(pose, z, bl, v, t, size=TEXTURE, want_float=True)
    assert atlas.texture.shape == (TEXTURE, TEXTURE, 4) and atlas.texture.dtype == torch.uint8
    assert (atlas.num_triangles, atlas.size, atlas.cell) == (len(t), TEXTURE, ops.bake_layout(len(t), TEXTURE).cell)
    nerf, cs = gen.nerf, gen.nerf.coordinate_scale
    baked = ops.bake_points(v, t, TEXTURE)
    parts = _parts_from_part_poses(nerf, pose_parts, model_input["bone_length"])
    tri, feat_cl = nerf._tri_plane_pair(model_input)
    _, gradient = ops.field_gradient((baked.points * cs)[None].contiguous(), parts, nerf.canonical_pose, tri, feat_cl,
                                     nerf._mlp_pack(model_input["z_rend"]), **nerf.kernel_flags())
    want = ops.encode_normal_map(baked.texel_face, gradient[0], v, t, negate=True, want_float=True)
    own = baked.texel_face >= 0
    bent = own & (atlas.texture[..., :3] != torch.tensor([128, 128, 255], dtype=torch.uint8, device="cuda")).any(-1)
    assert int(own.sum()) > 1000 and int(bent.sum()) > int(own.sum()) // 2
    assert torch.equal(atlas.texture, want.texture)
    assert _np(atlas.texture_f32).tobytes() == _np(want.texture_f32).tobytes()
    banded = bake_normal_map(nerf, pose_parts, v, t, model_input, size=TEXTURE, band_rows=300)
    assert torch.equal(banded.texture, atlas.texture) and banded.texture_f32 is None
    # the map agrees with field_normals at the texel points: decoded in the frame it is that normal to a byte's quantisation
    from enarf_gan_amd.libraries.NARF.mesh_rendering import field_normals
    some = torch.nonzero(bent.reshape(-1))[:4096, 0]
    fn = field_normals(nerf, pose_parts, baked.points.t()[some].contiguous(), model_input)
    tg, bt, nr, _ = NR.frames(_np(v), _np(t))
    k = _np(baked.texel_face.reshape(-1)[some])
    q = _np(atlas.texture_f32.reshape(-1, 3)[some]).astype(np.float64)
    world = q[:, :1] * tg[k] + q[:, 1:2] * bt[k] + q[:, 2:] * nr[k]
    assert np.abs(world - _np(fn)).max() < 1e-5
    # a larger min_gradient flattens texels
    high = gen.bake_normal_map(pose, z, bl, v, t, size=TEXTURE, min_gradient=1e30)
    assert (high.texture[own] == torch.tensor([128, 128, 255, 255], dtype=torch.uint8, device="cuda")).all()


def test_extract_rigged_mesh_fills_the_normal_map():
    gen, s, z, pose, bl, K, mesh = _model()
    h = 2 * mesh["voxel_size"]
    A = 256
    rig = gen.extract_rigged_mesh(pose, z, bl, **mesh, simplify_cell=h, normal_map_size=A)
    sv, st = gen.extract_mesh(pose, z, bl, **mesh, simplify_cell=h)
    assert torch.equal(rig.vertices, sv) and torch.equal(rig.triangles, st) and rig.texture is None
    assert (rig.normal_map.num_triangles, rig.normal_map.size) == (len(st), A) and rig.normal_map.texture.shape == (A, A, 4)
    assert torch.equal(rig.normal_map.texture, gen.bake_normal_map(pose, z, bl, sv, st, size=A).texture)
    both = gen.extract_rigged_mesh(pose, z, bl, **mesh, simplify_cell=h, normal_map_size=A, texture_size=A)
    assert torch.equal(both.normal_map.texture, rig.normal_map.texture) and both.texture.size == A
    plain = gen.extract_rigged_mesh(pose, z, bl, **mesh, simplify_cell=h)
    assert plain.normal_map is None and torch.equal(plain.vertices, sv) and torch.equal(plain.joints, rig.joints)


def _keys(s):
    from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle
    first = s["pose_to_camera"][:1]
    return torch.cat([first, rotate_pose_by_angle(first, torch.tensor([0.7]))]).double().cuda()


def test_a_frame_of_the_normal_mapped_animation_is_skin_mesh_and_paint():
    from enarf_gan_amd.libraries.NARF.mesh_rendering import paint_normal_mapped_mesh, skin_mesh
    gen, s, z, pose, bl, K, mesh = _model()
    A = TEXTURE
    rig = gen.extract_rigged_mesh(pose, z, bl, **mesh, texture_size=A, normal_map_size=A)
    keys = _keys(s)
    R, num = 96, 3
    frames, poses = gen.render_textured_mesh_animation(rig, keys, bl, K, num=num, loop=False, render_size=R, frames_per_batch=2,
                                                       normal_map=True)
    white, _ = gen.render_mesh_animation(rig, keys, bl, K, num=num, loop=False, render_size=R, color=None, normal_map=True)
    assert frames.shape == (num, R, R, 3) and frames.dtype == torch.uint8 and frames.is_cuda and poses.shape[0] == num
    for i in (0, 2):
        pose_parts, bone = gen.nerf.transform_pose(poses[i:i + 1].float(), bl.float())
        posed = skin_mesh(gen.nerf, rig, pose_parts, bone)[0]
        want = paint_normal_mapped_mesh(posed, rig.triangles, rig.normal_map, K, gen.size, R, atlas=rig.texture)[1].image
        assert torch.equal(frames[i], want), f"frame {i}"
        want = paint_normal_mapped_mesh(posed, rig.triangles, rig.normal_map, K, gen.size, R)[1].image
        assert torch.equal(white[i], want), f"white frame {i}"
    plain, _ = gen.render_textured_mesh_animation(rig, keys, bl, K, num=num, loop=False, render_size=R, frames_per_batch=2)
    assert not torch.equal(frames, plain) and not torch.equal(frames[0], frames[2])
    bare = gen.extract_rigged_mesh(pose, z, bl, **mesh, texture_size=A)
    with pytest.raises(ValueError, match="normal_map_size"):
        gen.render_textured_mesh_animation(bare, keys, bl, K, num=num, normal_map=True)
    with pytest.raises(ValueError, match="color=None"):
        gen.render_mesh_animation(rig, keys, bl, K, num=num, color="parts", normal_map=True)
    # the still image: the same pieces
    img, (v, t, atlas, nmap) = gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=A, normal_map=True)
    assert torch.equal(nmap.texture, gen.bake_normal_map(pose, z, bl, v, t, size=A).texture)
    assert np.array_equal(img, _np(paint_normal_mapped_mesh(v, t, nmap, K, gen.size, atlas=atlas)[1].image))
    with pytest.raises(ValueError, match="two sources"):
        gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=A, normal_map=True, normals="field")


def test_the_defaults_of_the_touched_entry_points_are_what_they_were(tmp_path):
    """without the new keywords, and with them at their defaults, every touched entry point gives the result of the pieces
    it was made of before: the rig record, the textured still, both animations, the GLB"""
    from enarf_gan_amd.libraries.NARF.mesh_rendering import export_glb, paint_textured_mesh, skin_mesh
    gen, s, z, pose, bl, K, mesh = _model()
    A = TEXTURE
    rig = gen.extract_rigged_mesh(pose, z, bl, **mesh, texture_size=A, return_colors=True)
    same = gen.extract_rigged_mesh(pose, z, bl, **mesh, texture_size=A, return_colors=True, normal_map_size=None)
    assert rig.normal_map is None and same.normal_map is None
    for k in ("vertices", "triangles", "joints", "weights", "kept_mass", "colors"):
        assert torch.equal(getattr(rig, k), getattr(same, k)), k
    assert torch.equal(rig.texture.texture, same.texture.texture)
    img, (v, t, atlas) = gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=A)
    img2, pieces = gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=A, normal_map=False)
    assert len(pieces) == 3 and np.array_equal(img, img2)
    assert np.array_equal(img, _np(paint_textured_mesh(v, t, atlas, K, gen.size)[1].image))
    keys = _keys(s)
    R, num = 96, 3
    for fn, kw in ((gen.render_textured_mesh_animation, {}), (gen.render_mesh_animation, dict(color="field")),
                   (gen.render_mesh_animation, dict(color=None))):
        a, _ = fn(rig, keys, bl, K, num=num, loop=False, render_size=R, **kw)
        b, _ = fn(rig, keys, bl, K, num=num, loop=False, render_size=R, normal_map=False, **kw)
        assert torch.equal(a, b)
    frames, poses = gen.render_textured_mesh_animation(rig, keys, bl, K, num=num, loop=False, render_size=R)
    pose_parts, bone = gen.nerf.transform_pose(poses[2:3].float(), bl.float())
    posed = skin_mesh(gen.nerf, rig, pose_parts, bone)[0]
    assert torch.equal(frames[2], paint_textured_mesh(posed, rig.triangles, rig.texture, K, gen.size, R)[1].image)
    paths = [str(tmp_path / f"{i}.glb") for i in range(2)]
    export_glb(rig, paths[0])
    export_glb(rig, paths[1], normal_map=None)
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()


# ------------------------------------------------------------------------------------------------- poisoned allocations
WORDS = (0xFFFFFFFF, 0x7F7F7F7F)


@contextlib.contextmanager
def _recorded(calls):
    """wrap the function attributes of the loaded library: `calls` collects the names of the functions called"""
    mod = binding(NP.STEM)
    lib, undo = mod.load(), []
    for name in mod.SIGNATURES:
        fn = getattr(lib, name)

        def wrapper(*a, _fn=fn, _name=name):
            calls.add(_name)
            return _fn(*a)
        setattr(lib, name, wrapper)
        undo.append((name, fn))
    try:
        yield
    finally:
        for name, fn in undo:
            setattr(lib, name, fn)


def _bytes(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy()


def _run(name, word):
    """one run of the case, as tests/test_gpu_poison.py runs its own: the outputs on the host"""
    from enarf_gan_amd import _lib
    calls = set()
    poison_cases.SNAPSHOT.clear()
    with _recorded(calls), (poisoned(word) if word is not None else contextlib.nullcontext()) as p:
        inputs, outputs, check = getattr(NP, name)()
        torch.cuda.synchronize()
        assert _lib.device_status(clear=True) == 0, f"{name}: device status after the run"
        if p is not None:
            p.check()
            assert p.records, f"{name}: no allocation of the run was served poisoned"
            for k, t in outputs.items():
                assert any(buf.data_ptr() <= t.data_ptr() < buf.data_ptr() + buf.numel() for _, buf, *_ in p.records), \
                    f"{name}: output {k} was not served by the shim"
    assert set(poison_cases.SNAPSHOT) == set(inputs), f"{name}: the case did not snapshot its inputs before the call"
    for k, t in inputs.items():
        assert np.array_equal(_bytes(t), _bytes(poison_cases.SNAPSHOT[k])), f"{name}: input {k} was written"
    check(outputs)
    missing = {fn for fn, cases in NP.POISON_CASES.items() if name in cases} - calls
    assert not missing, f"{name} is listed under {sorted(missing)} but did not call them"
    return {k: v.detach().cpu() for k, v in outputs.items()}


@pytest.mark.parametrize("name", NP.CASE_NAMES)
def test_entry_point_on_poisoned_memory(name):
    """three runs - the allocator's own memory, every allocation of the package filled with 0xFFFFFFFF, with 0x7F7F7F7F -:
    equal bits, the inputs unwritten, the guard bands intact"""
    clean = _run(name, None)
    for word in WORDS:
        out = _run(name, word)
        assert set(out) == set(clean), name
        for k, t in out.items():
            assert t.shape == clean[k].shape and t.dtype == clean[k].dtype, f"{name} under {word:#x}: {k}"
            same = _bytes(t) == _bytes(clean[k])
            assert same.all(), f"{name} under {word:#x}: {k}: {int((~same).sum())} bytes differ from the clean run"
