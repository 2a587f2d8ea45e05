"""CPU checks of the normal maps (libenarf_nmap.so's host side, the tangent frame, export_glb with a normal map, the referee
of the GPU tests): no GPU. The row `nmap` of build.LATE_LIBRARIES gets the per-row checks tests/test_side_libraries_cpu.py
makes for the side rows; every argument check raises before a device is touched; the handedness of the frame is derived
from _bake_lib.atlas_corners; the referee round-trips a constant field; three planted mistakes move the referee by more
than the GPU test's bounds on that test's inputs; a GLB with a normal map is parsed back."""
import ast
import ctypes as C
import hashlib
import importlib
import inspect
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import bake_cases as BC
import bake_reference as BR
import libraries as L
import nmap_cases as NC
import nmap_reference as NR
import paint_cases as PC
from enarf_gan_amd import _nmap_lib, build, ops
from enarf_gan_amd._bake_lib import atlas_corners
from enarf_gan_amd.libraries.NARF.mesh_rendering import RiggedMesh, TextureAtlas, export_glb

STEM = "nmap"
HEADER = os.path.join(L.ROOT, "include", build.LATE_LIBRARIES[STEM][1])


# ------------------------------------------------------------------------------------------------- the row of the build table
def test_the_late_table_leaves_the_other_tables_alone_and_build_walks_it():
    assert list(build.LATE_LIBRARIES) == [STEM] and not set(build.LATE_LIBRARIES) & set(build.ALL_LIBRARIES)
    assert list(build.ALL_LIBRARIES) == list(build.LIBRARIES) + list(build.SIDE_LIBRARIES)
    assert list(build.EVERY_LIBRARY) == list(build.ALL_LIBRARIES) + [STEM]
    L.library("hip")                                      # build() makes every row of every table
    assert os.path.exists(build.lib_path(STEM)) and build.binding(STEM) == "enarf_gan_amd._nmap_lib"


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(enarf_nmap_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound_and_abi_version():
    lib = C.CDLL(L.library(STEM))
    declared = _declared()
    assert declared and set(_nmap_lib.SIGNATURES) == set(declared)
    for fn in declared:
        assert hasattr(lib, fn), f"{fn} declared in enarf_nmap.h but not exported"
    assert _nmap_lib.load().enarf_nmap_abi_version() == _nmap_lib.ABI_VERSION == 1
    assert re.search(rf"#define\s+ENARF_NMAP_ABI_VERSION\s+{_nmap_lib.ABI_VERSION}\s", open(HEADER).read())


def test_kernels_equal_the_registry_and_each_has_gpu_tests():
    registry = importlib.import_module("nmap_kernel_coverage")
    kernel_tests, module = registry.NMAP_KERNEL_TESTS, registry.GPU_TEST_MODULE
    built = L.kernels(STEM)
    assert built == set(kernel_tests) and sorted(re.findall(r"nmap_[a-z]+_kernel", " ".join(built))) == \
        ["nmap_encode_kernel", "nmap_shade_kernel"]
    tree = ast.parse(open(os.path.join(L.TESTS, module + ".py")).read())
    functions = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    for kernel, tests in kernel_tests.items():
        assert tests, f"{kernel}: no test"
        for t in tests:
            assert t.split("::")[0] == module and t.split("::")[1] in functions, f"{kernel}: {t} does not exist in {module}"


def test_build_tracks_every_included_header():
    tracked = {os.path.basename(h) for h in build.lib_deps(STEM)}
    seen, todo = set(), list(build.LATE_LIBRARIES[STEM][0])
    while todo:
        f = todo.pop()
        path = os.path.join(build.CSRC, f) if os.path.exists(os.path.join(build.CSRC, f)) else os.path.join(L.ROOT, "include", f)
        for inc in re.findall(r'#include\s+"([^"]+)"', open(path).read()):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert "enarf_nmap.h" in seen and seen <= tracked, seen - tracked


def test_no_kernel_is_shared_with_any_other_library():
    mine = L.kernels(STEM)
    assert mine
    for other in build.ALL_LIBRARIES:
        assert not mine & L.kernels(other), f"a kernel of {build.lib_path(STEM)} inside {build.lib_path(other)}"


def test_every_declared_function_has_a_poison_case_or_a_reason():
    import nmap_poison_cases as NP
    declared = set(_declared())
    assert set(NP.POISON_CASES) | set(NP.HOST_ONLY) == declared and not set(NP.POISON_CASES) & set(NP.HOST_ONLY)
    for fn, cases in NP.POISON_CASES.items():
        assert len(cases) >= 2, f"{fn}: one case with every optional output and one bare"
        for c in cases:
            f = getattr(NP, c, None)
            assert inspect.isfunction(f) and not inspect.signature(f).parameters, f"{fn}: {c} is not a case"
    defined = {n for n, f in vars(NP).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == NP.__name__
               and not inspect.signature(f).parameters}
    assert defined == set(NP.CASE_NAMES)


# ------------------------------------------------------------------------------------------------- argument checks
def _encode_inputs():
    (v, t), A = NC.mesh((5, 21))
    return dict(texel_face=torch.from_numpy(np.array(NC.texel_face((5, 21)))), vectors=torch.from_numpy(np.array(NC.vectors((5, 21)))),
                vertices=torch.from_numpy(np.array(v)), triangles=torch.from_numpy(np.array(t)))


def _shade_inputs():
    h = PC.hand_buffer()
    a = {k: torch.from_numpy(np.array(h[k])) for k in ("pix_to_face", "bary", "normals", "vertices", "triangles")}
    a["normal_texture"] = torch.from_numpy(np.array(NC.hand_normal_textures(16)[0]))
    return a


ENCODE_ERRORS = [
    (dict(texel_face=lambda a: a["texel_face"].long()), "int32"),
    (dict(texel_face=lambda a: a["texel_face"].reshape(-1)), "rows, A"),
    (dict(vectors=lambda a: a["vectors"].t().contiguous()), "three planes"),
    (dict(vectors=lambda a: a["vectors"].double()), "float32"),
    (dict(vectors=lambda a: a["vectors"].numpy()), "tensors"),
    (dict(vertices=lambda a: a["vertices"][:, :2]), r"\(V, 3\)"),
    (dict(triangles=lambda a: a["triangles"].int()), "int64"),
    (dict(triangles=lambda a: a["triangles"].reshape(-1)), r"\(T, 3\)"),
    (dict(min_length=lambda a: -1.0), "min_length"),
    (dict(min_length=lambda a: float("nan")), "min_length"),
    (dict(min_length=lambda a: "x"), "min_length"),
    (dict(out=lambda a: (torch.zeros(21, 21, 3, dtype=torch.uint8), None)), "uint8 texture"),
    (dict(out=lambda a: (torch.zeros(21, 21, 4, dtype=torch.uint8), torch.zeros(21, 21, 4))), "fp32 texture"),
    (dict(out=lambda a: torch.zeros(21, 21, 4, dtype=torch.uint8)), "out as"),
    (dict(), "device tensors"),                                  # everything right, on the CPU: no fallback
]


@pytest.mark.parametrize("change,match", ENCODE_ERRORS)
def test_encode_argument_checks_raise_before_a_device_is_touched(change, match, monkeypatch):
    monkeypatch.setattr(_nmap_lib, "load", lambda: pytest.fail("the library was loaded"))
    a = _encode_inputs()
    kw = {k: f(a) for k, f in change.items()}
    args = {**a, **{k: kw.pop(k) for k in list(kw) if k in a}}
    with pytest.raises(ValueError, match=match):
        ops.encode_normal_map(**args, **kw)


SHADE_ERRORS = [
    (dict(pix_to_face=lambda a: a["pix_to_face"].int()), "int64"),
    (dict(pix_to_face=lambda a: a["pix_to_face"][:, :7]), r"\(R, R\)"),
    (dict(bary=lambda a: a["bary"][:7]), "bary"),
    (dict(normals=lambda a: a["normals"].double()), "float32"),
    (dict(vertices=lambda a: a["vertices"].reshape(-1)), r"\(V, 3\)"),
    (dict(normal_texture=lambda a: a["normal_texture"].int()), "normal_texture"),
    (dict(normal_texture=lambda a: a["normal_texture"][..., :3]), "normal_texture"),
    (dict(normal_texture=lambda a: a["normal_texture"][:, :8]), "normal_texture"),
    (dict(normal_texture=lambda a: None), "normal_texture"),
    (dict(texture=lambda a: torch.zeros(16, 16, 4)), "texture"),
    (dict(texture=lambda a: torch.zeros(20, 20, 3)), "one atlas, one size"),
    (dict(base_color=lambda a: (1.0, 0.5)), "base_color"),
    (dict(background=lambda a: "white"), "background"),
    (dict(), "device tensors"),
]


@pytest.mark.parametrize("change,match", SHADE_ERRORS)
def test_shade_argument_checks_raise_before_a_device_is_touched(change, match, monkeypatch):
    monkeypatch.setattr(_nmap_lib, "load", lambda: pytest.fail("the library was loaded"))
    a = _shade_inputs()
    kw = {k: f(a) for k, f in change.items()}
    args = {**a, **{k: kw.pop(k) for k in list(kw) if k in a}}
    with pytest.raises(ValueError, match=match):
        ops.shade_normal_mapped(**args, **kw)


def test_an_atlas_too_small_for_the_mesh_and_the_c_abi_checks():
    a = _shade_inputs()
    a["triangles"] = a["triangles"][:1].repeat(9, 1)
    with pytest.raises(NotImplementedError, match="at least 18"):
        ops.shade_normal_mapped(**{**a, "normal_texture": torch.zeros(12, 12, 4, dtype=torch.uint8)})
    lib = _nmap_lib.load()                                       # the C side rejects on the host as well: no device here
    assert lib.enarf_nmap_encode(None, None) == -1 and lib.enarf_nmap_shade(None, None) == -1
    e = _nmap_lib.EncodeArgs()
    e.count = -1
    assert lib.enarf_nmap_encode(C.byref(e), None) == -1 and b"texels" in lib.enarf_nmap_last_error()
    e.count = 0
    assert lib.enarf_nmap_encode(C.byref(e), None) == 0          # nothing to do, nothing launched
    e.count = 4
    assert lib.enarf_nmap_encode(C.byref(e), None) == -1 and b"null" in lib.enarf_nmap_last_error()
    s = _nmap_lib.ShadeArgs()
    s.R, s.A = 8, 16
    assert lib.enarf_nmap_shade(C.byref(s), None) == -1 and b"exactly one" in lib.enarf_nmap_last_error()
    s.A = 5
    assert lib.enarf_nmap_shade(C.byref(s), None) == -1 and b"atlas size" in lib.enarf_nmap_last_error()
    s.A, s.T = 12, 9
    assert lib.enarf_nmap_shade(C.byref(s), None) == -2


# ------------------------------------------------------------------------------------------------- the frame
@pytest.mark.parametrize("T,A", [(2, 6), (8, 12), (5, 21), (200, 128)])
def test_the_handedness_of_the_frame_follows_from_atlas_corners(T, A):
    """[e1; e2] = [dU1; dU2] [dP/du; dP/dv] solved for random triangles with U from atlas_corners, both halves: t^ is
    unit(dP/du), b^ = t^ x n^ is -dP/dv orthogonalised against t^, and glTF's cross(n^, t^) w is b^ for w = -1."""
    rng = np.random.default_rng(T)
    v = rng.normal(0, 1, (3 * T, 3)).astype(np.float32)
    t = np.arange(3 * T, dtype=np.int64).reshape(T, 3)
    U = atlas_corners(T, A)
    P = v.astype(np.float64)[t]
    E = np.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], 1)                     # (T, 2, 3)
    dU = np.stack([U[:, 1] - U[:, 0], U[:, 2] - U[:, 0]], 1)                    # (T, 2, 2)
    J = np.linalg.solve(dU, E)                                                  # rows dP/du, dP/dv
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    for frames in (NR.frames(v, t), _nmap_lib.tangent_frames(v, t)):
        tg, bt, n, valid = frames
        assert valid.all() and {0, 1} <= set((np.arange(T) % 2).tolist())
        assert np.abs(tg - unit(J[:, 0])).max() < 1e-12
        down = -J[:, 1]
        assert np.abs(bt - unit(down - (down * tg).sum(-1, keepdims=True) * tg)).max() < 1e-12
        assert np.abs(n - unit(np.cross(E[:, 0], E[:, 1]))).max() < 1e-12
        w = np.sign((np.cross(n, tg) * bt).sum(-1))
        assert (w == -1).all()
        assert np.abs(np.cross(n, tg) * -1.0 - bt).max() < 1e-12
        for a, b in ((tg, bt), (tg, n), (bt, n)):
            assert np.abs((a * b).sum(-1)).max() < 1e-12
        assert np.abs(np.linalg.norm(bt, axis=-1) - 1).max() < 1e-12


def test_a_triangle_without_a_frame():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [np.inf, 1, 1], [3e38, 0, 0], [-3e38, 0, 0]], np.float32)
    t = np.array([[0, 1, 2], [0, 0, 2], [0, 1, 3], [0, 1, 4], [0, 5, 2], [0, 1, 8], [-1, 1, 2], [6, 7, 2]], np.int64)
    for frames in (NR.frames(v, t), _nmap_lib.tangent_frames(v, t)):
        assert frames[3].tolist() == [True, False, False, False, False, False, False, True]
    tg, bt, n, _ = _nmap_lib.tangent_frames(v, t)
    assert (tg[1:7] == [1, 0, 0]).all() and (n[1:7] == [0, 0, 1]).all() and (bt[1:7] == [0, -1, 0]).all()
    assert (tg[0] == [1, 0, 0]).all() and (n[0] == [0, 0, 1]).all() and (bt[0] == [0, -1, 0]).all()


# ------------------------------------------------------------------------------------------------- the referee
def _probe(T, seed, n=400):
    """n (face, barycentric) probes over the triangles, corners and edges among them"""
    rng = np.random.default_rng(seed)
    face = rng.integers(0, T, n)
    b = rng.uniform(0, 1, (n, 3))
    b /= b.sum(-1, keepdims=True)
    b[:6] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]]
    face[:12] = np.repeat(np.arange(2) % T, 6)
    b[6:12] = b[:6]
    return face, b.astype(np.float32)


def _exact_motion(v):
    """a rigid motion whose fp32 result is exact for camera-space vertices with 1 < z < 4: a quarter turn about the
    camera's z axis (a signed permutation) and a step of -1/4 along z (toward finer fp32 spacing): the moved fp32 vertices
    are the moved float64 ones, so the posed frame is the turned rest frame to float64 rounding, not to fp32's"""
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tau = np.array([0.0, 0.0, -0.25])
    moved = v.astype(np.float64) @ R.T + tau
    assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved) and np.linalg.det(R) == 1
    return R, tau, moved.astype(np.float32)


@pytest.mark.parametrize("T,A", [(1, 6), (8, 12), (8, 40)])
def test_a_constant_field_round_trips_through_the_referee(T, A):
    """encode a constant unit field d into the unrounded float map, tap anywhere in a triangle (corners and edges
    included), decode: Ns = d within 1e-12 for both halves; on rigidly moved vertices it is R d"""
    v, t = BC.hand_mesh(T)
    d = NC.CONSTANT_D
    assert abs(np.linalg.norm(d) - 1) < 1e-15
    face = BR.points(v, t, A)["texel_face"]
    enc = NR.encode(face, np.repeat(d.astype(np.float32)[:, None], A * A, 1), v, t, negate=False)
    d32 = d.astype(np.float32).astype(np.float64)
    d32 /= np.linalg.norm(d32)                              # the field the kernel sees: d rounded to fp32
    assert not enc["flat"].any()
    f, b = _probe(T, A)
    n = len(f)
    R_ = int(np.ceil(np.sqrt(n)))
    pix = np.full(R_ * R_, -1, np.int64)
    pix[:n] = f
    bary = np.zeros((R_ * R_, 3), np.float32)
    bary[:n] = b
    stored = np.zeros((R_, R_, 3), np.float32)
    Rm, tau, moved = _exact_motion(v)
    for verts, want in ((v, d32), (moved, Rm @ d32)):
        out = NR.shade(pix.reshape(R_, R_), bary.reshape(R_, R_, 3), stored, verts, t, enc["texture_f32"], lit=False)
        got = out["normal"].reshape(-1, 3)[:n]
        assert out["framed"].reshape(-1)[:n].all() and {0, 1} <= set((f % 2).tolist()) | ({1} if T == 1 else set())
        assert np.abs(got - want).max() < 1e-12, np.abs(got - want).max()


def test_the_lighting_is_paint_reference_s_on_stored_normals():
    """NR.lighting restates lines of paint_reference.shade / bake_reference.shade: on the hand buffer with the stored
    normals it gives bake_reference.shade's `shaded` bit for bit"""
    h = PC.hand_buffer()
    geo = {k: h[k] for k in ("pix_to_face", "bary", "normals", "vertices", "triangles")}
    tex = BC.hand_textures(16)[1]
    ref = BR.shade(**geo, texture=tex, lit=True)
    drawn = ref["drawn"]
    b = h["bary"].astype(np.float64)[drawn]
    p = h["vertices"].astype(np.float64)[h["triangles"][h["pix_to_face"][drawn]]]
    point = (b[:, 0, None] * p[:, 0] + b[:, 1, None] * p[:, 1]) + b[:, 2, None] * p[:, 2]
    got = NR.lighting(ref["albedo"][drawn], NR.stored_unit(h["normals"].astype(np.float64)[drawn]), point)
    assert drawn.sum() == 54 and np.array_equal(got, ref["shaded"][drawn], equal_nan=True)
    # and with a flat fp32 map on a mesh whose every face has a frame the albedo and the background are bake_reference's
    flat = np.zeros((16, 16, 3), np.float32)
    flat[..., 2] = 1
    mine = NR.shade(**geo, normal_texture=flat, texture=tex, lit=True, background=(0.1, 0.2, 0.3))
    theirs = BR.shade(**geo, texture=tex, lit=True, background=(0.1, 0.2, 0.3))
    assert np.array_equal(mine["albedo"], theirs["albedo"], equal_nan=True) and np.array_equal(mine["drawn"], theirs["drawn"])
    assert np.array_equal(mine["shaded"][~drawn], theirs["shaded"][~drawn])


@pytest.mark.parametrize("case", NC.ENCODE_CASES, ids=str)
def test_no_level_of_the_encode_cases_lies_at_a_rounding_boundary(case):
    """The GPU test asks for equal bytes. The byte is floor(x), x = 255 clamp((c + 1) / 2) + 0.5: the seeded vectors must
    leave no x of a texel that was encoded from a vector within 1e-9 of an integer (a flat or empty texel is the constant
    (0, 0, 1): its x are 128 and 255.5 by construction, computed from constants on both sides)."""
    (v, t), A = NC.mesh(case)
    face, vec = NC.texel_face(case), NC.vectors(case)
    for kw in (dict(min_length=NC.MIN_LENGTH), dict(negate=False)):
        ref = NR.encode(face, vec, v, t, **kw)
        coded = (face >= 0) & ~ref["flat"]
        x = ref["levels"][coded]
        assert coded.sum() > 0 and np.abs(x - np.round(x)).min() > 1e-9
        assert ref["flat"].sum() >= (4 if case != (1, 6) else 1)
        assert (ref["texture"][face < 0] == [128, 128, 255, 0]).all() and (ref["texture"][ref["flat"]] == [128, 128, 255, 255]).all()
    if case in ((5, 21),):
        own = set(np.unique(face[face >= 0]).tolist())
        assert own == {0, 1, 2}                                  # triangles 3 and 4 name vertex V and -1: they own nothing
    ref = NR.encode(face, vec, v, t, min_length=NC.MIN_LENGTH)
    longer = NR.encode(face, vec, v, t, min_length=0.0)
    assert (ref["flat"] & ~longer["flat"]).sum() > 0             # lengths on both sides of min_length


def test_an_owner_outside_the_mesh_is_flat():
    """texel_face as a caller could hand it over: owners T, T + 3 and one whose triangle names vertex V and -1"""
    v, t = BC.hand_mesh(5)
    face = np.array([[0, 5, 8, 3, 4, -1, 2]], np.int32)
    vec = np.ones((3, 7), np.float32)
    ref = NR.encode(face, vec, v, t)
    assert ref["flat"].tolist() == [[False, True, True, True, True, False, False]]
    assert (ref["texture"][0, 1:5] == [128, 128, 255, 255]).all() and (ref["texture"][0, 5] == [128, 128, 255, 0]).all()


@pytest.mark.parametrize("bug", NR.BUGS[1:])
def test_a_planted_bug_moves_the_referee_by_more_than_the_gpu_bounds(bug):
    """no sign flip for odd triangles, b^ = n^ x t^, decode without the -1: on the GPU test's own inputs each changes bytes
    of an encoded map or moves a shading normal by more than NORMAL_BOUND, so the GPU test can see it"""
    seen = []
    if bug != "decode_without_shift":
        for case in ((5, 21), (8, 12)):
            (v, t), A = NC.mesh(case)
            good = NR.encode(NC.texel_face(case), NC.vectors(case), v, t, min_length=NC.MIN_LENGTH)
            bad = NR.encode(NC.texel_face(case), NC.vectors(case), v, t, min_length=NC.MIN_LENGTH, bug=bug)
            seen.append((good["texture"] != bad["texture"]).sum())
            assert seen[-1] > 0 and np.abs(good["texture_f32"] - bad["texture_f32"]).max() > NC.F32_BOUND
    h = PC.hand_buffer()
    geo = {k: h[k] for k in ("pix_to_face", "bary", "normals", "vertices", "triangles")}
    for tex in NC.hand_normal_textures(16):
        if bug == "decode_without_shift" and tex.dtype != np.uint8:
            continue
        good, bad = NR.shade(**geo, normal_texture=tex), NR.shade(**geo, normal_texture=tex, bug=bug)
        moved = np.abs(good["normal"] - bad["normal"])[good["framed"]].max()
        assert moved > 1000 * NC.NORMAL_BOUND
        assert np.abs(good["image"].astype(int) - bad["image"].astype(int)).max() > 1


# ------------------------------------------------------------------------------------------------- glTF
def _rig(colors=False):
    v, t = BC.hand_mesh(8)
    V = len(v)
    joints = np.tile(np.array([[0, 1, -1, -1]], np.int32), (V, 1))
    w = np.tile(np.array([[0.75, 0.25, 0, 0]], np.float32), (V, 1))
    rest = np.tile(np.eye(4, dtype=np.float32), (1, 2, 1, 1))
    rest[0, 1, :3, 3] = [0.1, 0.2, 0.3]
    c = torch.from_numpy(PC.sine_colors(v)) if colors else None
    return RiggedMesh(torch.from_numpy(np.array(v)), torch.from_numpy(np.array(t)), torch.from_numpy(joints), torch.from_numpy(w),
                      torch.ones(V), torch.from_numpy(rest), torch.ones(1, 2, 1), c)


def _normal_atlas(A=24):
    v, t = BC.hand_mesh(8)
    face = BR.points(v, t, A)["texel_face"]
    rng = np.random.default_rng(3)
    ref = NR.encode(face, rng.normal(0, 1, (3, A * A)).astype(np.float32), v, t)
    return TextureAtlas(torch.from_numpy(ref["texture"].copy()), None, len(t), A, BR.layout(len(t), A)[0])


def _colour_atlas(A=24):
    rng = np.random.default_rng(4)
    return TextureAtlas(torch.from_numpy(rng.integers(0, 256, (A, A, 4)).astype(np.uint8)), None, 8, A, BR.layout(8, A)[0])


def _parse(path):
    data = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<4sII", data, 0)
    assert (magic, version, total) == (b"glTF", 2, len(data))
    n, kind = struct.unpack_from("<I4s", data, 12)
    assert kind == b"JSON"
    doc = json.loads(data[20:20 + n])
    m, kind = struct.unpack_from("<I4s", data, 20 + n)
    assert kind == b"BIN\0"
    return doc, data[28 + n:28 + n + m]


def _accessor(doc, blob, index):
    acc = doc["accessors"][index]
    view = doc["bufferViews"][acc["bufferView"]]
    width = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}[acc["type"]]
    dtype = {5126: np.float32, 5121: np.uint8, 5125: np.uint32}[acc["componentType"]]
    return np.frombuffer(blob, dtype, acc["count"] * width, view["byteOffset"]).reshape(acc["count"], width)


def _png(blob, view):
    data = blob[view["byteOffset"]:view["byteOffset"] + view["byteLength"]]
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack_from(">I4s", data, at)
        body = data[at + 8:at + 8 + n]
        if kind == b"IHDR":
            w, h, depth, colour = struct.unpack_from(">IIBB", body)
            assert (depth, colour) == (8, 6)
            size = (h, w)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], 1 + 4 * size[1])
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(size[0], size[1], 4)


@pytest.mark.parametrize("how", ["map only", "map and texture", "map and vertex colours", "map on the rig"])
def test_export_glb_with_a_normal_map(tmp_path, how):
    rig, nmap = _rig(colors=how == "map and vertex colours"), _normal_atlas()
    colour = _colour_atlas() if how == "map and texture" else None
    path = str(tmp_path / "mesh.glb")
    if how == "map on the rig":
        rig.normal_map = nmap
        export_glb(rig, path)
    else:
        export_glb(rig, path, texture=colour, normal_map=nmap)
    doc, blob = _parse(path)
    prim = doc["meshes"][0]["primitives"][0]
    att = prim["attributes"]
    T = rig.triangles.shape[0]
    pos, nrm, tan, uv = (_accessor(doc, blob, att[k]) for k in ("POSITION", "NORMAL", "TANGENT", "TEXCOORD_0"))
    assert pos.shape == (3 * T, 3) and nrm.shape == (3 * T, 3) and tan.shape == (3 * T, 4) and uv.shape == (3 * T, 2)
    assert doc["accessors"][att["TANGENT"]]["type"] == "VEC4" and doc["accessors"][att["TANGENT"]]["componentType"] == 5126
    assert np.array_equal(_accessor(doc, blob, prim["indices"]).reshape(-1), np.arange(3 * T))
    v, t = rig.vertices.numpy(), rig.triangles.numpy()
    assert np.array_equal(pos, v[t.reshape(-1)])
    assert (tan[:, 3] == -1).all() and np.abs(np.linalg.norm(tan[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
    # NORMAL is the face normal, from POSITION alone
    P = pos.astype(np.float64).reshape(T, 3, 3)
    E = np.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], 1)
    face_n = np.cross(E[:, 0], E[:, 1])
    face_n /= np.linalg.norm(face_n, axis=1, keepdims=True)
    assert np.abs(nrm.reshape(T, 3, 3) - face_n[:, None]).max() < 1e-6
    assert (np.abs(tan.reshape(T, 3, 4) - tan.reshape(T, 3, 4)[:, :1]).max() == 0)          # one frame a triangle
    # the viewer's bitangent cross(NORMAL, TANGENT.xyz) w points along decreasing v, the tangent along increasing u
    U = uv.astype(np.float64).reshape(T, 3, 2)
    J = np.linalg.solve(np.stack([U[:, 1] - U[:, 0], U[:, 2] - U[:, 0]], 1), E)
    tg = tan.reshape(T, 3, 4)[:, 0, :3].astype(np.float64)
    bit = np.cross(nrm.reshape(T, 3, 3)[:, 0].astype(np.float64), tg) * tan.reshape(T, 3, 4)[:, 0, 3:4]
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    down = -J[:, 1]
    assert ((bit * down).sum(-1) > 0).all() and ((tg * J[:, 0]).sum(-1) > 0).all()
    assert np.abs(tg - unit(J[:, 0])).max() < 1e-5
    assert np.abs(bit - unit(down - (down * tg).sum(-1, keepdims=True) * tg)).max() < 1e-5
    # the material
    mat = doc["materials"][prim["material"]]
    tex = doc["textures"][mat["normalTexture"]["index"]]
    assert tex["sampler"] == 0 and len(doc["samplers"]) == 1
    pixels = _png(blob, doc["bufferViews"][doc["images"][tex["source"]]["bufferView"]])
    assert np.array_equal(pixels, nmap.texture.numpy())
    if colour is not None:
        base = doc["textures"][mat["pbrMetallicRoughness"]["baseColorTexture"]["index"]]
        assert base["source"] != tex["source"] and base["sampler"] == 0 and len(doc["images"]) == 2
        assert np.array_equal(_png(blob, doc["bufferViews"][doc["images"][base["source"]]["bufferView"]]), colour.texture.numpy())
        assert "COLOR_0" not in att
    else:
        assert "baseColorTexture" not in mat["pbrMetallicRoughness"] and len(doc["images"]) == 1
        assert mat["pbrMetallicRoughness"] == {"metallicFactor": 0.0, "roughnessFactor": 1.0}
    if how == "map and vertex colours":
        assert np.array_equal(_accessor(doc, blob, att["COLOR_0"]), rig.colors.numpy()[t.reshape(-1)])
    else:
        assert "COLOR_0" not in att
    for k in ("JOINTS_0", "WEIGHTS_0"):
        assert len(_accessor(doc, blob, att[k])) == 3 * T


def test_export_glb_rejects_what_does_not_fit_a_normal_map(tmp_path):
    rig, nmap, path = _rig(), _normal_atlas(), str(tmp_path / "x.glb")
    with pytest.raises(ValueError, match="normals="):
        export_glb(rig, path, normal_map=nmap, normals=torch.zeros(6, 3))
    with pytest.raises(ValueError, match="baked for 9 triangles"):
        export_glb(rig, path, normal_map=TextureAtlas(nmap.texture, None, 9, 24, 8))
    with pytest.raises(ValueError, match="uint8 texture"):
        export_glb(rig, path, normal_map=TextureAtlas(nmap.texture[:20], None, 8, 24, 8))
    with pytest.raises(ValueError, match="one TEXCOORD_0"):
        export_glb(rig, path, texture=_colour_atlas(30), normal_map=nmap)


def test_a_triangle_without_a_frame_gets_the_fixed_tangent(tmp_path):
    rig, nmap, path = _rig(), _normal_atlas(), str(tmp_path / "x.glb")
    tri = rig.triangles.clone()
    tri[3] = torch.tensor([2, 2, 4])                               # |e1| = 0
    rig.triangles = tri
    export_glb(rig, path, normal_map=nmap)
    doc, blob = _parse(path)
    att = doc["meshes"][0]["primitives"][0]["attributes"]
    assert (_accessor(doc, blob, att["TANGENT"])[9:12] == [1, 0, 0, -1]).all()
    assert (_accessor(doc, blob, att["NORMAL"])[9:12] == [0, 0, 1]).all()


def test_export_glb_without_a_normal_map_writes_the_bytes_it_wrote(tmp_path):
    """the keyword absent, None, and a rig record without the field's value: one file; the file of the dyadic rig of
    tests/test_bake_cpu.py still has the sha256 recorded there before export_glb took a texture"""
    import test_bake_cpu as TB
    read = lambda p: open(p, "rb").read()
    for rig, kw in ((_rig(), {}), (_rig(colors=True), {}), (_rig(), dict(texture=_colour_atlas())),
                    (_rig(colors=True), dict(normals=torch.ones(6, 3)))):
        a, b = str(tmp_path / "a.glb"), str(tmp_path / "b.glb")
        export_glb(rig, a, **kw)                                   # the call every caller made before the keyword existed
        export_glb(rig, b, normal_map=None, **kw)
        assert rig.normal_map is None and read(a) == read(b)
        doc, _ = _parse(a)
        assert "TANGENT" not in doc["meshes"][0]["primitives"][0]["attributes"]
        assert "normalTexture" not in json.dumps(doc)
    old = [getattr(TB, n) for n in dir(TB) if isinstance(getattr(TB, n), str) and re.fullmatch(r"[0-9a-f]{64}", getattr(TB, n))]
    assert len(old) == 1
    path = str(tmp_path / "old.glb")
    export_glb(TB._dyadic_rig(), path)
    assert hashlib.sha256(read(path)).hexdigest() == old[0]


def test_the_rig_record_and_the_entry_points_took_the_new_keywords_last():
    import dataclasses
    from enarf_gan_amd.libraries.NARF import mesh_rendering as MR
    from enarf_gan_amd.models.generator import TriNARFGenerator
    from enarf_gan_amd.models.narf import TriPlaneNARF
    fields = [f.name for f in dataclasses.fields(RiggedMesh)]
    assert fields[-2:] == ["texture", "normal_map"] and RiggedMesh.__dataclass_fields__["normal_map"].default is None
    for fn in (MR.extract_rigged_mesh, TriPlaneNARF.extract_rigged_mesh, TriNARFGenerator.extract_rigged_mesh):
        assert "normal_map_size" not in inspect.signature(inspect.unwrap(fn)).parameters
        assert list(inspect.signature(inspect.unwrap(fn)).parameters)[-1] == "simplify_cell"
    for fn in (TriPlaneNARF.render_textured_mesh, TriNARFGenerator.render_textured_mesh):
        assert "normal_map" not in inspect.signature(inspect.unwrap(fn)).parameters
    for fn in (TriNARFGenerator.render_textured_mesh_animation, TriNARFGenerator.render_mesh_animation):
        assert inspect.signature(fn).parameters["normal_map"].default is False
    assert list(inspect.signature(export_glb).parameters)[-1] == "normal_map"
    p = inspect.signature(MR.bake_normal_map).parameters
    assert list(p) == ["model", "pose_to_camera", "vertices", "triangles", "model_input", "size", "normal_fn", "min_gradient",
                       "want_float", "band_rows"]
    p = inspect.signature(MR.paint_normal_mapped_mesh).parameters
    assert list(p) == ["vertices", "triangles", "normal_atlas", "intrinsics", "img_size", "render_size", "atlas", "base_color",
                       "lit", "use_float"]
