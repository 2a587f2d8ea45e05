"""CPU checks of the coloured-mesh path (libenarf_paint.so's host side, the referee of the GPU tests, the exporters): no
GPU. The library checks of the `paint` row (header against exports and SIGNATURES, ABI version, kernel inventory against
tests/paint_kernel_coverage.py, tracked headers, disjoint kernels) are tests/test_side_libraries_cpu.py's."""
import re

import numpy as np
import pytest
import torch

import paint_cases as PC
import paint_reference as PR
import raster_reference as RR
from enarf_gan_amd import ops
from enarf_gan_amd._loader import EnarfHipError
from enarf_gan_amd.libraries.NARF.mesh_rendering import export_obj, export_ply


# ------------------------------------------------------------------------------------------------------------- referee
@pytest.mark.parametrize("R", sorted(PC.CAMERAS))
def test_referee_with_white_colours_gives_the_rasteriser_image(R):
    """The deferred shading of the rasteriser's own buffers, rounded to fp32 as the kernel stores them, with white vertex
    colours: the rasteriser's hard-Phong image, to one level (the rounding of b' and the normal may move a floor)."""
    verts, tris = PC.sphere()
    assert 7000 <= len(tris) <= 8500, len(tris)
    ref = RR.rasterize(verts, tris, PC.intrinsics(R), PC.CAMERAS[R][0], R)
    got = PR.shade(ref["pix_to_face"], ref["bary"].astype(np.float32), ref["normals"].astype(np.float32), verts, tris,
                   vertex_colors=np.ones((len(verts), 3), np.float32))
    cov = ref["pix_to_face"] >= 0
    assert cov.mean() > 0.1 and np.array_equal(got["drawn"], cov)
    d = np.abs(got["image"].astype(np.int16) - ref["image"].astype(np.int16))
    print(f"R = {R}: {cov.sum()} covered pixels, largest difference {d[cov].max()} levels, {(d[cov] > 0).sum()} pixels differ")
    assert d[cov].max() <= 1
    # white texels are the sum of the three stored b': 1 to three fp32 roundings (3 x 2^-25)
    assert (got["image"][~cov] == 255).all() and np.abs(got["albedo"][cov] - 1).max() <= 3 * 2.0 ** -25 and (got["albedo"][~cov] == 1).all()
    # unlit: the image is the colour
    flat = PR.shade(ref["pix_to_face"], ref["bary"].astype(np.float32), ref["normals"].astype(np.float32), verts, tris,
                    vertex_colors=PC.sine_colors(verts), lit=False, background=(0.0, 0.5, 1.0))
    assert np.array_equal(flat["albedo"], flat["shaded"]) and (flat["image"][~cov] == [0, 127, 255]).all()
    assert 0 <= flat["albedo"][cov].min() and flat["albedo"][cov].max() <= 1 and flat["albedo"][cov].std() > 0.1


def test_label_mode_rules_on_hand_buffers():
    h = PC.hand_buffer()
    geo = {k: h[k] for k in ("pix_to_face", "bary", "normals", "vertices", "triangles")}
    out = PR.shade(**geo, vertex_labels=h["vertex_labels"], palette=h["palette"], lit=False, background=(0.1, 0.2, 0.3),
                   neutral=(0.6, 0.5, 0.4))
    pal = h["palette"].astype(np.float64)
    bg, nt = np.float32([0.1, 0.2, 0.3]).astype(np.float64), np.float32([0.6, 0.5, 0.4]).astype(np.float64)
    a = out["albedo"]
    # row 0: face ids -1, T, T + 5, 2^40 and -7 are background
    assert out["drawn"][0].tolist() == [False, False, False, False, True, True, True, False]
    assert all((a[0, c] == bg).all() for c in (0, 1, 2, 3, 7))
    # row 1: triangle 3 names vertex V, triangle 4 vertex -1
    assert out["drawn"][1].tolist() == [False, False, False, False, True, True, True, False]
    # row 2: ties go to the lower corner. faces 0, 1, 2, 0, 1, 2, 0, 1 = vertices (0 1 2), (3 4 5), (2 1 4); labels 0 1 2 -1 P 1
    #   (.5 .5 0) f0 -> corner 0 = vertex 0, label 0;   (.25 .25 .5) f1 -> corner 2 = vertex 5, label 1
    #   (.4 .4 .2) f2 -> corner 0 = vertex 2, label 2;   (.2 .4 .4) f0 -> corner 1 = vertex 1, label 1
    #   (.4 .2 .4) f1 -> corner 0 = vertex 3, label -1;  (1/3 1/3 1/3) f2 -> corner 0 = vertex 2, label 2
    #   (0 .5 .5) f0 -> corner 1 = vertex 1, label 1;    (.5 0 .5) f1 -> corner 0 = vertex 3, label -1
    want = [pal[0], pal[1], pal[2], pal[1], nt, pal[2], pal[1], nt]
    for c, w in enumerate(want):
        assert (a[2, c] == w).all(), c
    # row 3: labels -1 and P give neutral; (.45 .45 .1) on triangle 1 ties to corner 0 = vertex 3 = -1
    #   triangle 2 = vertices (2 1 4): (.1 .1 .8) -> vertex 4 = P; (.1 .8 .1) -> vertex 1; triangle 0: vertex 0, vertex 2
    want = [nt, nt, pal[1], nt, nt, pal[1], pal[0], pal[2]]
    for c, w in enumerate(want):
        assert (a[3, c] == w).all(), c
    # a NaN first barycentric never loses to a later corner: corner 0 of triangle 2 = vertex 2 = label 2
    assert (a[4, 2] == pal[2]).all()
    assert np.array_equal(out["albedo"], out["shaded"])
    # lit, colour mode: a zero normal gives the ambient term alone, a normal facing away too; a NaN barycentric a NaN -> 0
    lit = PR.shade(**geo, vertex_colors=h["vertex_colors"])
    assert np.allclose(lit["shaded"][4, 0], 0.5 * lit["albedo"][4, 0], rtol=1e-15, atol=0)
    assert np.allclose(lit["shaded"][4, 1], 0.5 * lit["albedo"][4, 1], rtol=1e-15, atol=0)
    assert np.isnan(lit["shaded"][4, 2]).all() and (lit["image"][4, 2] == 0).all()
    assert (lit["shaded"][5:] > 0.5 * lit["albedo"][5:]).mean() > 0.8                           # mostly facing the light


# ----------------------------------------------------------------------------------------------------------- exporters
def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, element = {}, {}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            element = w[1]
            counts[element], props[element] = int(w[2]), []
        elif w[:1] == ["property"]:
            props[element].append(tuple(w[1:]))
    kind = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    vdt = np.dtype([(p[1], kind[p[0]]) for p in props["vertex"]])
    assert props["face"] == [("list", "uchar", "int", "vertex_indices")]
    vert = np.frombuffer(raw, vdt, counts["vertex"], end)
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    face = np.frombuffer(raw, fdt, counts["face"], end + vert.nbytes)
    assert end + vert.nbytes + face.nbytes == len(raw)
    return vert, face


@pytest.mark.parametrize("with_colors,with_labels", [(True, False), (False, True), (False, False), (True, True)])
def test_ply_round_trip(tmp_path, with_colors, with_labels):
    rng = np.random.default_rng(2)
    v = rng.normal(0, 1, (11, 3)).astype(np.float32)
    f = rng.integers(0, 11, (7, 3)).astype(np.int64)
    c = rng.uniform(0, 1, (11, 3)).astype(np.float32)
    c[0], c[1] = [0.0, 1.0, 0.5], [-0.2, 1.3, 1 / 255]
    lab = rng.integers(-1, 23, 11).astype(np.int32)
    path = str(tmp_path / "m.ply")
    export_ply(torch.from_numpy(v), torch.from_numpy(f), path, colors=torch.from_numpy(c) if with_colors else None,
               labels=torch.from_numpy(lab) if with_labels else None)
    vert, face = _read_ply(path)
    names = ["x", "y", "z"] + (["red", "green", "blue"] if with_colors else []) + (["part"] if with_labels else [])
    assert list(vert.dtype.names) == names
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), v)
    assert (face["n"] == 3).all() and np.array_equal(face["v"], f)
    if with_colors:
        rgb = np.stack([vert["red"], vert["green"], vert["blue"]], 1)
        assert np.array_equal(rgb, np.floor(255 * np.clip(c.astype(np.float64), 0, 1)).astype(np.uint8))
        assert rgb[0].tolist() == [0, 255, 127] and rgb[1].tolist() == [0, 255, 1]
    if with_labels:
        assert np.array_equal(vert["part"], lab)
    with pytest.raises(ValueError):
        export_ply(v, f, path, colors=c[:5])
    with pytest.raises(ValueError):
        export_ply(v, f, path, labels=lab[:5])
    export_ply(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), path)                 # an empty mesh is a header
    vert, face = _read_ply(path)
    assert len(vert) == 0 and len(face) == 0


def test_export_obj_keeps_its_bytes_and_takes_colours(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, (9, 3)).astype(np.float32)
    f = rng.integers(0, 9, (5, 3)).astype(np.int64)
    c = rng.uniform(0, 1, (9, 3)).astype(np.float32)
    plain, coloured = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
    export_obj(torch.from_numpy(v), torch.from_numpy(f), plain)
    # what export_obj wrote before it took colours, restated
    want = "".join("v %r %r %r\n" % (float(x[0]), float(x[1]), float(x[2])) for x in v)
    want += "".join("f %d %d %d\n" % (t[0], t[1], t[2]) for t in f + 1)
    assert open(plain).read() == want
    export_obj(v, f, plain, colors=None)
    assert open(plain).read() == want
    export_obj(torch.from_numpy(v), torch.from_numpy(f), coloured, colors=torch.from_numpy(c))
    lines = open(coloured).read().splitlines()
    vl = [ln.split() for ln in lines if ln.startswith("v ")]
    assert len(vl) == 9 and all(len(w) == 7 for w in vl)
    assert np.array_equal(np.array([[float(x) for x in w[1:]] for w in vl], np.float32), np.concatenate([v, c], 1))
    assert [ln for ln in lines if ln.startswith("f ")] == [ln for ln in want.splitlines() if ln.startswith("f ")]
    with pytest.raises(ValueError):
        export_obj(v, f, coloured, colors=c[:4])


# ------------------------------------------------------------------------------------------------ host-side rejections
def _args(R=4, V=5, T=3):
    return dict(pix_to_face=torch.zeros(R, R, dtype=torch.int64), bary=torch.zeros(R, R, 3), normals=torch.zeros(R, R, 3),
                vertices=torch.zeros(V, 3), triangles=torch.zeros(T, 3, dtype=torch.int64))


def test_host_side_rejections():
    """every ValueError of the binding is raised from shapes and dtypes alone, before any device is asked for; what passes
    them on CPU tensors meets 'no CPU fallback'"""
    a, V = _args(), 5
    colors, labels, pal = torch.zeros(V, 3), torch.zeros(V, dtype=torch.int32), torch.zeros(3, 3)
    with pytest.raises(ValueError, match="both"):
        ops.shade_fragments(**a, vertex_colors=colors, vertex_labels=labels, palette=pal)
    with pytest.raises(ValueError, match="neither"):
        ops.shade_fragments(**a)
    with pytest.raises(ValueError, match="palette"):
        ops.shade_fragments(**a, vertex_labels=labels)
    with pytest.raises(ValueError, match="palette"):
        ops.shade_fragments(**a, vertex_colors=colors, palette=pal)
    bad = [dict(pix_to_face=torch.zeros(4, 4, dtype=torch.int32)), dict(pix_to_face=torch.zeros(4, 5, dtype=torch.int64)),
           dict(pix_to_face=torch.zeros(16, dtype=torch.int64)), dict(bary=torch.zeros(4, 4, 2)), dict(bary=torch.zeros(5, 5, 3)),
           dict(bary=torch.zeros(4, 4, 3, dtype=torch.float64)), dict(normals=torch.zeros(4, 4)),
           dict(normals=torch.zeros(4, 4, 3, dtype=torch.float16)), dict(vertices=torch.zeros(V, 4)),
           dict(vertices=torch.zeros(V, 3, dtype=torch.float64)), dict(triangles=torch.zeros(3, 3, dtype=torch.int32)),
           dict(triangles=torch.zeros(3, 4, dtype=torch.int64)), dict(vertex_colors=torch.zeros(V + 1, 3)),
           dict(vertex_colors=torch.zeros(V, 4)), dict(vertex_colors=torch.zeros(V, 3, dtype=torch.float64)),
           dict(vertex_colors=np.zeros((V, 3), np.float32))]
    for b in bad:
        with pytest.raises(ValueError):
            ops.shade_fragments(**{**a, "vertex_colors": colors, **b})
    bad = [dict(vertex_labels=torch.zeros(V, dtype=torch.int64)), dict(vertex_labels=torch.zeros(V + 1, dtype=torch.int32)),
           dict(vertex_labels=torch.zeros(V, 1, dtype=torch.int32)), dict(palette=torch.zeros(3, 4)), dict(palette=torch.zeros(0, 3)),
           dict(palette=torch.zeros(3)), dict(palette=torch.zeros(3, 3, dtype=torch.float64))]
    for b in bad:
        with pytest.raises(ValueError):
            ops.shade_fragments(**{**a, "vertex_labels": labels, "palette": pal, **b})
    with pytest.raises(ValueError, match=r"outside \[1, 4096\]"):                             # R = 0
        ops.shade_fragments(**_args(R=0), vertex_colors=colors)
    with pytest.raises(ValueError, match=r"outside \[1, 4096\]"):
        ops.shade_fragments(pix_to_face=torch.zeros(1, dtype=torch.int64).expand(4097, 4097), bary=a["bary"],
                            normals=a["normals"], vertices=a["vertices"], triangles=a["triangles"], vertex_colors=colors)
    for kw in (dict(background=(1.0, 0.5)), dict(neutral="grey"), dict(background=(0, 0, 0, 0))):
        with pytest.raises(ValueError):
            ops.shade_fragments(**a, vertex_colors=colors, **kw)
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.shade_fragments(**a, vertex_colors=colors)
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.shade_fragments(**a, vertex_labels=labels, palette=pal, lit=False)
    with pytest.raises(EnarfHipError, match="no CPU fallback"):                                # T = 0 and V = 0 are sizes it takes
        ops.shade_fragments(**_args(V=0, T=0), vertex_colors=torch.zeros(0, 3))


def test_model_entry_points_reject_an_unknown_colour_source():
    from enarf_gan_amd.models.narf import TriPlaneNARF
    assert re.search(r"color=\"field\"", TriPlaneNARF.render_colored_mesh.__doc__)
    with pytest.raises(ValueError, match="'field'"):
        TriPlaneNARF._colored_mesh(None, None, None, None, None, 0.1, 15, 0.4, "texture")
