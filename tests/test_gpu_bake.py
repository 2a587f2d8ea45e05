"""GPU tests of the texture atlas (libenarf_bake.so): bake_points_kernel, bake_resolve_kernel and bake_shade_kernel against
the float64 numpy restatement of their contracts (tests/bake_reference.py) on hand-written inputs and on the 33^3 sphere of
tests/paint_cases.py, the properties the atlas exists for (no colour bleeds between faces, an affine colour is reproduced up
to the edges, a texture resolves detail vertex colours cannot), determinism, the empty mesh, and the model-level entry
points. The referee reads the very buffers the kernels read, so no texel and no pixel is left out of any comparison.

The sphere has 7688 triangles: 62 cells a row, all of them full. An atlas of 256 cannot hold it (the layout asks for
6 x 62 = 372), so the sphere is baked at 380 (cell 6, 63 cells a row, a margin of two texels) where only the kernel is
compared, and at 510 (cell 8, a leg of four texels, 63 cells a row, a margin of six) where the texture is looked at."""
import functools

import numpy as np
import pytest
import torch

import bake_cases as BC
import bake_reference as BR
import paint_cases as PC
from test_gpu_paint import _buffers, _check, _dev, _model

pytestmark = pytest.mark.gpu

GEO = ("pix_to_face", "bary", "normals", "vertices", "triangles")
SPHERE_SMALL, SPHERE_ATLAS = 380, 510


def _np(t):
    return t.cpu().numpy()


def _points(v, t, A, rows=None):
    from enarf_gan_amd import ops
    out = ops.bake_points(_dev(v), _dev(t), A, rows=rows)
    torch.cuda.synchronize()
    assert out._fields == ("points", "texel_face")
    return {k: _np(getattr(out, k)) for k in out._fields}


def _shade(h, texture, **kw):
    from enarf_gan_amd import ops
    out = ops.shade_textured(*(_dev(h[k]) for k in GEO), _dev(texture), **kw)
    torch.cuda.synchronize()
    assert out._fields == ("image", "albedo", "shaded")
    return {k: _np(getattr(out, k)) for k in out._fields}


def _torch_fn(fn):
    """a numpy colour function of points (M, 3) as bake_texture's color_fn"""
    return lambda p: torch.from_numpy(np.asarray(fn(_np(p)), np.float64)).to(p.device)


@functools.lru_cache(maxsize=None)
def _sphere_atlas(kind):
    """the sphere's TextureAtlas at SPHERE_ATLAS with the fp32 texture, baked through mesh_rendering.bake_texture with a
    colour function; (atlas, texture uint8 numpy, texture_f32 numpy)"""
    from enarf_gan_amd.libraries.NARF.mesh_rendering import bake_texture
    fn = {"sine": BC.fine_sine, "affine": BC.affine_color}[kind]
    v, t = PC.sphere()
    atlas = bake_texture(None, None, _dev(v), _dev(t), size=SPHERE_ATLAS, color_fn=_torch_fn(fn), want_float=True)
    torch.cuda.synchronize()
    assert (atlas.num_triangles, atlas.size, atlas.cell) == (len(t), SPHERE_ATLAS, 8)
    return atlas, _np(atlas.texture), _np(atlas.texture_f32)


# ------------------------------------------------------------------------------------------------- the kernels alone
def _check_points(got, ref, A, what):
    """bake_points' two outputs (numpy) against bake_reference.points' -> the map of owned texels"""
    assert got["points"].shape == (3, A * A) and got["points"].dtype == np.float32
    assert got["texel_face"].shape == (A, A) and got["texel_face"].dtype == np.int32
    assert np.array_equal(got["texel_face"], ref["texel_face"])
    u = BR.ulps_from(got["points"], ref["points"])
    own = ref["texel_face"] >= 0
    print(f"{what}: {own.sum()} owned texels of {own.size}, points {u.max():.0f} ulp ({(u > 0).sum()} values off)")
    assert u.max() <= 1
    assert (got["points"].reshape(3, A, A)[:, ~own] == 0).all()
    return own


@pytest.mark.parametrize("case", [(1, 6), (5, 16), (5, 21), (8, 12), "sphere"])
def test_bake_points_match_the_referee_on_every_texel(case):
    """texel_face equal, points the referee rounded to fp32 or one step from it. (5, .) is the hand mesh whose triangle 3
    names vertex V and whose triangle 4 names vertex -1: they own nothing."""
    (v, t), A = (PC.sphere(), SPHERE_SMALL) if case == "sphere" else (BC.hand_mesh(case[0]), case[1])
    if case == "sphere":
        with pytest.raises(NotImplementedError, match="at least 372"):
            _points(v, t, 256)
        assert BR.layout(len(t), A) == (6, 63)
    else:
        assert BR.layout(len(t), A)[0] == BC.LAYOUTS[case]
    got, ref = _points(v, t, A), BR.points(v, t, A)
    own = _check_points(got, ref, A, case)
    owned = set(np.unique(ref["texel_face"][own]).tolist())
    assert owned == (set(range(len(t))) - {3, 4} if case in ((5, 16), (5, 21)) else set(range(len(t))))


def test_bands_of_rows_stitch_to_the_whole_atlas():
    for (v, t), A, cuts in ((BC.hand_mesh(5), 21, (0, 7, 8, 21)), (PC.sphere(), SPHERE_SMALL, (0, 100, 101, 379, 380))):
        whole = _points(v, t, A)
        bands = [_points(v, t, A, rows=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        for band, a, b in zip(bands, cuts[:-1], cuts[1:]):
            assert band["points"].shape == (3, (b - a) * A) and band["texel_face"].shape == (b - a, A)
        assert np.concatenate([b["texel_face"] for b in bands]).tobytes() == whole["texel_face"].tobytes()
        assert np.concatenate([b["points"] for b in bands], axis=1).tobytes() == whole["points"].tobytes()


def _check_resolved(tex, f32, ref, face, what):
    """bake_resolve's texture (and its fp32 texture, or None) as numpy against bake_reference.resolve's"""
    assert tex.shape == face.shape + (4,) and tex.dtype == np.uint8 and (f32 is None or f32.shape == face.shape + (3,))
    u = np.zeros(1) if f32 is None else BR.ulps_from(f32, ref["texture_f32"])
    print(f"{what}: {(tex != ref['texture']).sum()} bytes differ, fp32 texture {u.max():.0f} ulp")
    assert np.array_equal(tex, ref["texture"]) and u.max() <= 1


def test_bake_resolve_matches_the_referee():
    """colours with NaN, +-inf and values outside [-1, 1], labels -1, P and beyond, empty texels (whose colour is a NaN that
    is never read): the bytes equal the referee's, the fp32 texture within one step."""
    from enarf_gan_amd import ops
    face, color, labels, palette = BC.resolve_inputs()
    fill, neutral = (0.2, 0.4, 0.6), (0.6, 0.5, 0.4)
    modes = [("colours", dict(color=color), dict()), ("unit colours", dict(color=color), dict(unit=True)),
             ("labels", dict(labels=labels, palette=palette), dict(neutral=neutral))]
    for what, data, kw in modes:
        out = ops.bake_resolve(_dev(face), **{k: _dev(a) for k, a in data.items()}, fill=fill, want_float=True, **kw)
        torch.cuda.synchronize()
        ref = BR.resolve(face, **data, fill=fill, **kw)
        tex, f32 = _np(out.texture), _np(out.texture_f32)
        _check_resolved(tex, f32, ref, face, what)
        empty = face < 0
        assert empty.sum() > 5 and (tex[empty] == [51, 102, 153, 0]).all() and (tex[~empty][:, 3] == 255).all()
        assert (f32[empty] == np.float32(fill)).all()
        # the same call without the fp32 texture, and into given tensors
        assert ops.bake_resolve(_dev(face), **{k: _dev(a) for k, a in data.items()}, fill=fill, **kw).texture_f32 is None
        given = (torch.zeros(face.shape + (4,), dtype=torch.uint8, device="cuda"), torch.zeros(face.shape + (3,), device="cuda"))
        back = ops.bake_resolve(_dev(face), **{k: _dev(a) for k, a in data.items()}, fill=fill, out=given, **kw)
        assert back.texture is given[0] and torch.equal(given[0], out.texture)
        assert _np(given[1]).tobytes() == f32.tobytes()
    # the defaults: black transparent fill, grey for a label outside the palette
    out = ops.bake_resolve(_dev(face), labels=_dev(labels), palette=_dev(palette))
    tex = _np(out.texture).reshape(-1, 4)
    assert (tex[0] == 0).all() and (tex[1] == [127, 127, 127, 255]).all() and (tex[6] == [127, 127, 127, 255]).all()


def test_hand_written_fragments_match_the_referee():
    """the 8 x 8 buffer of tests/paint_cases.py (face ids -1, T, T + 5, 2^40 and -7, triangles naming vertex V and vertex
    -1, a zero normal, a NaN barycentric) over random 16 x 16 textures of both kinds, lit and not"""
    h = PC.hand_buffer()
    geo = {k: h[k] for k in GEO}
    for texture in BC.hand_textures(16):
        for lit in (True, False):
            kw = dict(lit=lit, background=(0.1, 0.2, 0.3))
            got, ref = _shade(h, texture, **kw), BR.shade(**geo, texture=texture, **kw)
            assert ref["drawn"].sum() == 64 - 10
            _check(got, ref, f"hand buffer, {texture.dtype} texture, lit={lit}")
            bg = np.float32([0.1, 0.2, 0.3])
            assert (got["albedo"][~ref["drawn"]] == bg).all() and (got["shaded"][~ref["drawn"]] == bg).all()
            assert (got["image"][~ref["drawn"]] == [25, 51, 76]).all()
            assert np.isnan(got["albedo"][4, 2]).all() and (got["image"][4, 2] == 0).all()      # the NaN barycentric
    got = _shade(h, BC.hand_textures(16)[0])
    assert (got["albedo"][0, 0] == 1).all() and (got["image"][0, 0] == 255).all()                # the default background


def test_the_textured_sphere_matches_the_referee():
    """the rasterised sphere (R = 257: a partial last wavefront) with the texture bake_texture made of a fine sine pattern:
    both texture kinds, lit and not, every pixel"""
    h = _buffers("sphere")
    _, tex8, tex32 = _sphere_atlas("sine")
    assert (tex8[..., 3] == 255).mean() > 0.5 and len(np.unique(tex8[..., :3])) > 200
    for texture in (tex8, tex32):
        for lit in (True, False):
            got, ref = _shade(h, texture, lit=lit), BR.shade(**h, texture=texture, lit=lit)
            assert np.array_equal(ref["drawn"], h["pix_to_face"] >= 0) and ref["drawn"].sum() > 10000
            _check(got, ref, f"sphere, {texture.dtype} texture, lit={lit}")
            assert len(np.unique(got["image"][ref["drawn"]])) > 50


# ------------------------------------------------------------------------------------------------- what the atlas is for
def test_no_colour_bleeds_from_one_face_to_another():
    """Every face in a colour of its own, any two at least 1/64 apart: every owned texel of the texture holds its face's
    colour, and every covered pixel of the rasterised sphere then shows the colour of its own pix_to_face - one fp32 step
    at the most, since the four weights of a tap sum to one only to fp64 rounding."""
    from enarf_gan_amd import ops
    v, t = PC.sphere()
    A, T = SPHERE_ATLAS, len(t)
    colors = BC.face_colors(T)
    baked = ops.bake_points(_dev(v), _dev(t), A)
    face = _np(baked.texel_face)
    per_texel = np.where(face[..., None] >= 0, colors[np.clip(face, 0, T - 1)], np.nan).reshape(-1, 3).T.astype(np.float32)
    out = ops.bake_resolve(baked.texel_face, color=_dev(np.ascontiguousarray(per_texel)), unit=True, want_float=True)
    tex8, tex32 = _np(out.texture), _np(out.texture_f32)
    own = face >= 0
    assert set(np.unique(face[own]).tolist()) == set(range(T))
    assert np.array_equal(tex32[own], colors[face[own]].astype(np.float32)) and (tex32[~own] == 0).all()
    assert np.array_equal(tex8[own][:, :3], np.floor(255 * colors[face[own]]).astype(np.uint8))
    h = _buffers("sphere")
    cov = h["pix_to_face"] >= 0
    want = colors[h["pix_to_face"][cov]]
    for texture, truth in ((tex32, want), (tex8, np.floor(255 * want) / 255.0)):
        got = _shade(h, texture, lit=False)
        u = BR.ulps_from(got["albedo"][cov], truth)
        wrong = (np.abs(got["albedo"][cov] - truth) > 1 / 128).any(-1).sum()
        print(f"{texture.dtype} texture: {cov.sum()} covered pixels, albedo {u.max():.0f} ulp from the face's own colour, "
              f"{wrong} pixels off by more than 1/128")
        assert u.max() <= 1


def test_an_affine_colour_is_reproduced_up_to_the_edges():
    """A colour that is an affine function of position, G p + o: the guard texels hold its affine continuation, so a
    bilinear tap of the fp32 texture anywhere in a triangle gives the function itself, and the textured albedo is
    paint_mesh's albedo with the function at the vertices.

    The bound, with g the largest absolute row sum of G, s the sum of a pixel's stored barycentrics and ds the largest
    |s - 1| in the buffer (the rasteriser's fp32 rounding; measured from the buffer, not from the code under test):
      texels       a texel's point is stored in fp32, components below 4: off by 2^-23 at the most, the colour by g 2^-23;
                   the colour function's fp32 result (below 1) by 2^-25; a tap is a convex mix of such texels;
      outputs      both albedos are rounded to fp32 once: 2^-25 each; paint_mesh's vertex colours are fp32: 2^-25;
      s != 1       paint_mesh mixes colours, G p' + o s with p' = sum b'k v[ik]; the texture is read at uv = sum b'k Uk, whose
                   affine coordinates are b'k + (s - 1) U0 / L for k = 1, 2 (U0 <= A the corner in atlas texels, L = c - 4
                   the leg): the colour there is G p' + o + (1 - s) colour(v[i0]) + G ((s - 1) U0 / L) (e1 + e2) with e the
                   triangle's edges, components at most E. Colours are at most 1: ds (1 + 2 g E A / L).
    bound = g 2^-23 + 4 2^-25 + ds (1 + 2 g E A / L). Measured on the MI355X: 1.8e-07 against a bound of 5.1e-07 (ds = 4.5e-08, E = 0.056)."""
    from enarf_gan_amd.libraries.NARF.mesh_rendering import paint_mesh, paint_textured_mesh
    v, t = PC.sphere()
    atlas, _, tex32 = _sphere_atlas("affine")
    R = 257
    K, img = _dev(PC.intrinsics(R)).reshape(1, 3, 3), PC.CAMERAS[R][0]
    frag, textured = paint_textured_mesh(_dev(v), _dev(t), atlas, K, img, R, lit=False, use_float=True)
    vertex_colors = BC.affine_color(v).astype(np.float32)
    _, painted = paint_mesh(_dev(v), _dev(t), K, img, R, vertex_colors=_dev(vertex_colors), lit=False)
    cov = _np(frag.pix_to_face) >= 0
    bary = _np(frag.bary).astype(np.float64)[cov]
    G, _ = BC.affine_gradient()
    g = np.abs(G).sum(1).max()
    ds = np.abs((bary[:, 0] + bary[:, 1]) + bary[:, 2] - 1).max()
    tri = v.astype(np.float64)[t]
    E = max(np.abs(tri[:, 1] - tri[:, 0]).max(), np.abs(tri[:, 2] - tri[:, 0]).max())
    assert np.abs(v).max() < 4 and 0 < vertex_colors.min() and vertex_colors.max() < 1
    bound = g * 2.0 ** -23 + 4 * 2.0 ** -25 + ds * (1 + 2 * g * E * atlas.size / (atlas.cell - 4))
    d = np.abs(_np(textured.albedo).astype(np.float64) - _np(painted.albedo).astype(np.float64))[cov].max()
    print(f"affine colour: textured against vertex-colour albedo {d:.3e}, bound {bound:.3e} (ds = {ds:.2e}, E = {E:.3f}) "
          f"over {cov.sum()} pixels")
    assert cov.sum() > 10000 and d <= bound
    assert (_np(textured.albedo)[~cov] == 1).all()


def test_a_texture_resolves_detail_vertex_colours_cannot():
    """The point of the feature. A sine pattern whose wavelengths (0.112, 0.071, 0.060) are near the sphere's edge length
    (0.056): the truth is the pattern at every covered pixel's surface point sum b'k v[ik]. The mean absolute error of
    the textured albedo (RGBA8 texture, cell 8: a leg of 4 texels) must be below that of the vertex-colour albedo - an
    ordering, not a threshold. Measured on the MI355X: 0.032 against 0.248."""
    from enarf_gan_amd.libraries.NARF.mesh_rendering import paint_mesh, paint_textured_mesh
    v, t = PC.sphere()
    atlas, _, _ = _sphere_atlas("sine")
    assert atlas.cell - 4 >= 4
    R = 257
    K, img = _dev(PC.intrinsics(R)).reshape(1, 3, 3), PC.CAMERAS[R][0]
    frag, textured = paint_textured_mesh(_dev(v), _dev(t), atlas, K, img, R, lit=False)
    _, painted = paint_mesh(_dev(v), _dev(t), K, img, R, vertex_colors=_dev(BC.fine_sine(v)), lit=False)
    f = _np(frag.pix_to_face)
    cov = f >= 0
    b = _np(frag.bary).astype(np.float64)[cov]
    corner = v.astype(np.float64)[t[f[cov]]]
    truth = BC.fine_sine((b[:, 0, None] * corner[:, 0] + b[:, 1, None] * corner[:, 1]) + b[:, 2, None] * corner[:, 2]).astype(np.float64)
    e_tex = np.abs(_np(textured.albedo)[cov] - truth).mean()
    e_vert = np.abs(_np(painted.albedo)[cov] - truth).mean()
    print(f"fine sine on the sphere ({len(t)} triangles, atlas {atlas.size}, cell {atlas.cell}): mean absolute error of the "
          f"textured albedo {e_tex:.4f}, of the vertex-colour albedo {e_vert:.4f}")
    assert e_tex < e_vert


# ------------------------------------------------------------------------------------------------- robustness
def test_two_calls_are_bit_identical_and_an_empty_mesh_is_empty():
    from enarf_gan_amd import ops
    v, t = PC.sphere()
    a, b = _points(v, t, SPHERE_ATLAS), _points(v, t, SPHERE_ATLAS)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    colors = _dev(BC.fine_sine(a["points"].T).T.copy())
    face = _dev(a["texel_face"])
    r = [ops.bake_resolve(face, color=colors, unit=True, want_float=True) for _ in range(2)]
    assert torch.equal(r[0].texture, r[1].texture) and _np(r[0].texture_f32).tobytes() == _np(r[1].texture_f32).tobytes()
    h = _buffers("sphere")
    s = [_shade(h, _np(r[0].texture)) for _ in range(2)]
    assert all(s[0][k].tobytes() == s[1][k].tobytes() for k in s[0])
    # no triangle: nothing owns a texel, the texture is the fill, the image the background
    for V in (0, 5):
        ev, et = np.ones((V, 3), np.float32), np.zeros((0, 3), np.int64)
        e = _points(ev, et, 9)
        assert (e["texel_face"] == -1).all() and (e["points"] == 0).all()
        tex = ops.bake_resolve(_dev(e["texel_face"]), color=torch.full((3, 81), float("nan"), device="cuda"), fill=(1.0, 0.5, 0.0))
        assert (_np(tex.texture) == [255, 127, 0, 0]).all()
        R = 16
        eh = dict(pix_to_face=np.full((R, R), -1, np.int64), bary=np.full((R, R, 3), -1, np.float32),
                  normals=np.zeros((R, R, 3), np.float32), vertices=ev, triangles=et)
        eh["pix_to_face"][0, :4] = [0, 1, 2 ** 31, -5]
        got = _shade(eh, _np(tex.texture), background=(1.0, 0.5, 0.0))
        assert (got["albedo"] == [1.0, 0.5, 0.0]).all() and (got["image"] == [255, 127, 0]).all()
    # an atlas too small for the mesh
    hv, ht = BC.hand_mesh(5)
    nine = np.tile(ht[:1], (9, 1))
    with pytest.raises(NotImplementedError, match="at least 18"):
        _points(hv, nine, 12)
    with pytest.raises(NotImplementedError, match="at least 18"):
        hb = PC.hand_buffer()
        _shade({**{k: hb[k] for k in GEO}, "triangles": nine}, np.zeros((12, 12, 4), np.uint8))


# ------------------------------------------------------------------------------------------------- the model's entry points
TEXTURE = 1024


def _mesh_pieces():
    """the small generator of test_gpu_paint._model(), its mesh, and what mesh_rendering's functions take for it"""
    gen, s, z, pose, bl, K, mesh = _model()
    z_nerf, z_render, _ = gen._latent_parts(z)
    _, pose_parts, model_input = gen.nerf._mesh_inputs(pose, z_nerf, z_render, bl, 0.4)
    v, t = gen.extract_mesh(pose, z, bl, **mesh)
    assert 0 < len(t) <= 2 * (TEXTURE // 6) ** 2
    return gen, pose_parts, model_input, v, t


def test_bake_texture_of_the_field_is_the_query_at_the_texel_points():
    """the same kernels on the same inputs: bit for bit the resolve of the model's own query at bake_points' points; in
    bands of 300 rows or in one piece"""
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import bake_texture
    gen, s, z, pose, bl, K, mesh = _model()
    _, pose_parts, model_input, v, t = _mesh_pieces()
    atlas = gen.bake_texture(pose, z, bl, v, t, size=TEXTURE, want_float=True)
    assert atlas.texture.shape == (TEXTURE, TEXTURE, 4) and atlas.texture.dtype == torch.uint8
    assert (atlas.num_triangles, atlas.size, atlas.cell) == (len(t), TEXTURE, ops.bake_layout(len(t), TEXTURE).cell)
    baked = ops.bake_points(v, t, TEXTURE)
    nerf, cs = gen.nerf, gen.nerf.coordinate_scale
    scaled = pose_parts.clone()
    scaled[:, :, :3, 3] *= cs
    with torch.no_grad():
        _, col = nerf.calc_density_and_color_from_camera_coord_v2((baked.points * cs)[None].contiguous(), scaled, None, model_input)
    want = ops.bake_resolve(baked.texel_face, color=col[0].contiguous(), want_float=True)
    own = baked.texel_face >= 0
    assert int(own.sum()) > 1000 and float(atlas.texture_f32[own].std()) > 0.01
    assert torch.equal(atlas.texture, want.texture)
    assert _np(atlas.texture_f32).tobytes() == _np(want.texture_f32).tobytes()
    banded = bake_texture(nerf, pose_parts, v, t, model_input, size=TEXTURE, band_rows=300)
    assert torch.equal(banded.texture, atlas.texture) and banded.texture_f32 is None


def test_bake_texture_of_the_parts_is_part_labels_through_the_palette():
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import point_part_labels
    from enarf_gan_amd.libraries.NeRF.rendering import semantic_palette
    gen, s, z, pose, bl, K, mesh = _model()
    _, pose_parts, model_input, v, t = _mesh_pieces()
    atlas = gen.bake_texture(pose, z, bl, v, t, size=TEXTURE, color="parts")
    baked = ops.bake_points(v, t, TEXTURE)
    labels = point_part_labels(gen.nerf, pose_parts, baked.points[None], model_input)[0][0]
    palette = (semantic_palette(gen.nerf.num_bone, v.device) + 1) / 2
    want = ops.bake_resolve(baked.texel_face, labels=labels, palette=palette)
    assert torch.equal(atlas.texture, want.texture)
    assert len(torch.unique(atlas.texture[baked.texel_face >= 0][:, :3], dim=0)) >= 3
    with pytest.raises(ValueError):
        gen.bake_texture(pose, z, bl, v, t, size=TEXTURE, color="texture")


def test_render_textured_mesh_is_paint_textured_mesh_of_its_own_pieces():
    from enarf_gan_amd.libraries.NARF.mesh_rendering import paint_textured_mesh, rasterize_mesh
    gen, s, z, pose, bl, K, mesh = _model()
    for lit in (True, False):
        img, (v, t, atlas) = gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=TEXTURE, lit=lit)
        assert isinstance(img, np.ndarray) and img.shape == (512, 512, 3) and img.dtype == np.uint8
        ev, et = gen.extract_mesh(pose, z, bl, **mesh)
        assert torch.equal(v, ev) and torch.equal(t, et)
        assert torch.equal(atlas.texture, gen.bake_texture(pose, z, bl, v, t, size=TEXTURE).texture)
        frag, painted = paint_textured_mesh(v, t, atlas, K, gen.size, lit=lit)
        assert np.array_equal(img, _np(painted.image))
        assert torch.equal(frag.image, rasterize_mesh(v, t, K, gen.size).image)
        cov = _np(frag.pix_to_face) >= 0
        assert cov.sum() > 1000 and (img[~cov] == 255).all() and len(np.unique(img[cov].reshape(-1, 3), axis=0)) > 3
    # the existing entry points keep their colour modes: the textured path has its own
    with pytest.raises(ValueError):
        gen.render_colored_mesh(pose, K, z, bl, **mesh, color="texture")
    with pytest.raises(ValueError):
        gen.render_textured_mesh(pose, K, z, bl, **mesh, texture_size=TEXTURE, color="texture")


def test_a_frame_of_the_textured_animation_is_skin_mesh_and_paint_textured_mesh():
    from enarf_gan_amd.libraries.NARF.mesh_rendering import paint_textured_mesh, skin_mesh
    from enarf_gan_amd.libraries.NARF.pose_utils import rotate_pose_by_angle
    gen, s, z, pose, bl, K, mesh = _model()
    rig = gen.extract_rigged_mesh(pose, z, bl, **mesh, texture_size=TEXTURE)
    assert rig.texture is not None and rig.colors is None
    assert torch.equal(rig.texture.texture, gen.bake_texture(pose, z, bl, rig.vertices, rig.triangles, size=TEXTURE).texture)
    first = s["pose_to_camera"][:1]
    keys = torch.cat([first, rotate_pose_by_angle(first, torch.tensor([0.7]))]).double().cuda()
    R, num = 96, 3
    frames, poses = gen.render_textured_mesh_animation(rig, keys, bl, K, num=num, loop=False, render_size=R, frames_per_batch=2)
    assert frames.shape == (num, R, R, 3) and frames.dtype == torch.uint8 and frames.is_cuda and poses.shape[0] == num
    for i in (0, 2):
        pose_parts, bone = gen.nerf.transform_pose(poses[i:i + 1].float(), bl.float())
        posed = skin_mesh(gen.nerf, rig, pose_parts, bone)[0]
        want = paint_textured_mesh(posed, rig.triangles, rig.texture, K, gen.size, R)[1].image
        assert torch.equal(frames[i], want), f"frame {i}"
    assert not torch.equal(frames[0], frames[2]) and (frames[0] != 255).any()
    plain = gen.extract_rigged_mesh(pose, z, bl, **mesh)
    assert plain.texture is None
    with pytest.raises(ValueError):
        gen.render_textured_mesh_animation(plain, keys, bl, K, num=num)
    with pytest.raises(ValueError):
        gen.render_mesh_animation(rig, keys, bl, K, num=num, color="texture")
