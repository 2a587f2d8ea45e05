"""CPU checks of the texture atlas (libenarf_bake.so's host side, the layout, atlas_uv, export_glb with a texture and with
animation clips): no GPU. The layout is restated three times - ops.bake_layout, the library's enarf_bake_layout and the
downward search of tests/bake_reference.py - and all three must agree."""
import ctypes as C
import hashlib
import struct
import zlib

import numpy as np
import pytest
import torch

import bake_cases as BC
import bake_reference as BR
import skin_reference as SK
from test_skin_cpu import _accessor, _parse_glb, _quat_matrix, _rig
from enarf_gan_amd import ops
from enarf_gan_amd.libraries.NARF.mesh_rendering import RiggedMesh, TextureAtlas, atlas_uv, export_glb


# --------------------------------------------------------------------------------------------------------------- the layout
def test_the_layout_of_the_issue_cases_and_of_an_empty_mesh():
    for (T, A), cell in BC.LAYOUTS.items():
        lay = ops.bake_layout(T, A)
        assert lay.cell == cell and lay.cells_per_row == A // cell and lay.capacity == 2 * (A // cell) ** 2 >= T
        assert (lay.cell, lay.cells_per_row) == BR.layout(T, A)
    with pytest.raises(NotImplementedError, match="at least 18"):
        ops.bake_layout(*BC.UNSUPPORTED)
    with pytest.raises(BR.Unsupported):
        BR.layout(*BC.UNSUPPORTED)
    assert tuple(ops.bake_layout(0, 7)) == (7, 1, 2) and BR.layout(0, 7) == (7, 1)
    for bad in ((1, 5), (1, 8193), (-1, 64), (2 ** 31, 64), ("x", 64)):
        with pytest.raises(ValueError):
            ops.bake_layout(*bad)


def test_three_statements_of_the_layout_agree():
    from enarf_gan_amd import _bake_lib
    lib = _bake_lib.load()
    rng = np.random.default_rng(2)
    cases = [(T, A) for A in (6, 7, 11, 12, 13, 36, 100, 1024) for T in (0, 1, 2, 3, 8, 9, 50, 51, 2 * (A // 6) ** 2, 2 * (A // 6) ** 2 + 1)]
    cases += [(int(T), int(A)) for T, A in zip(rng.integers(0, 40000, 60), rng.integers(6, 900, 60))]
    cases += [(2 * 1365 ** 2, 8192), (2 * 1365 ** 2 + 1, 8192), (2 ** 31 - 1, 8192)]
    for T, A in cases:
        c, n = C.c_int32(), C.c_int32()
        rc = lib.enarf_bake_layout(T, A, C.byref(c), C.byref(n))
        try:
            want = BR.layout(T, A)
        except BR.Unsupported:
            assert rc == -2, (T, A)
            with pytest.raises(NotImplementedError):
                ops.bake_layout(T, A)
            continue
        assert rc == 0 and (c.value, n.value) == want == tuple(ops.bake_layout(T, A))[:2], (T, A)
    assert lib.enarf_bake_layout(1, 5, None, None) == -1 and lib.enarf_bake_layout(-1, 64, None, None) == -1


@pytest.mark.parametrize("T,A", [(1, 6), (5, 16), (5, 21), (8, 12), (31, 40), (200, 97)])
def test_every_texel_of_every_cell_has_exactly_one_owner(T, A):
    c, n = BR.layout(T, A)
    slot, i, j, h = BR.owners(T, A)
    inside = slot >= 0
    assert inside.sum() == (n * c) ** 2 and not inside[n * c:].any() and not inside[:, n * c:].any()
    counts = np.bincount(slot[inside], minlength=2 * n * n)
    assert len(counts) == 2 * n * n
    assert (counts[0::2] == c * (c + 1) // 2).all() and (counts[1::2] == c * (c - 1) // 2).all()      # together c c a cell
    # the owner is the half the texel centre lies in: below the anti-diagonal of the cell or on it, else above
    assert np.array_equal(h[inside] == 0, (i + j + 1 <= c)[inside])
    # texel_face of a mesh: the slots below T, and a triangle with a bad index owns nothing
    v, t = np.zeros((4, 3), np.float32), np.tile(np.array([0, 1, 2], np.int64), (T, 1))
    if T > 2:
        t[1, 2], t[2, 0] = 4, -1
    face = BR.points(v, t, A)["texel_face"]
    bad = (1, 2) if T > 2 else ()
    assert np.array_equal(face, np.where((slot >= 0) & (slot < T) & ~np.isin(slot, bad), slot, -1))


@pytest.mark.parametrize("c", [6, 7, 8, 9, 13, 24, 39])
def test_a_bilinear_tap_inside_a_triangle_reads_only_its_own_texels(c):
    """The footprint property the corner offsets exist for, on the taps exactly as the contract forms them (bake_reference
    .tap's index arithmetic): random barycentrics, the corners, points on the edges, and fp32 barycentrics whose sum is
    one only to rounding, as the rasteriser stores them."""
    rng = np.random.default_rng(c)
    b = rng.dirichlet([1, 1, 1], 4000)
    edge = rng.random(600)
    zero = np.zeros(600)
    b = np.concatenate([b, np.eye(3), np.stack([edge, 1 - edge, zero], -1), np.stack([edge, zero, 1 - edge], -1),
                        np.stack([zero, edge, 1 - edge], -1), np.array([[0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])])
    b = np.concatenate([b, b.astype(np.float32).astype(np.float64)])
    for h in (0, 1):
        U = BR.local_corners(c)[h]
        u = (b[:, 0] * U[0, 0] + b[:, 1] * U[1, 0]) + b[:, 2] * U[2, 0]
        w = (b[:, 0] * U[0, 1] + b[:, 1] * U[1, 1]) + b[:, 2] * U[2, 1]
        x0, x1, wx0, wx1 = BR._axis(u, 10 ** 6)                 # no clamp: the taps themselves must stay in the cell
        y0, y1, wy0, wy1 = BR._axis(w, 10 ** 6)
        for x, y, weight in ((x0, y0, wx0 * wy0), (x1, y0, wx1 * wy0), (x0, y1, wx0 * wy1), (x1, y1, wx1 * wy1)):
            assert x.min() >= 0 and y.min() >= 0 and x.max() <= c - 1 and y.max() <= c - 1
            own = (x + y + 1 <= c) if h == 0 else (x + y + 1 > c)
            # barycentrics that sum to one only to rounding can put a point a rounding error outside the hypotenuse: the
            # neighbour's diagonal texel then enters with the square of that error as its weight, far below any level
            assert (own | (weight <= 1e-12)).all()
        # and the usable leg is c - 4 texels
        assert abs(U[1, 0] - U[0, 0]) == c - 4 and abs(U[2, 1] - U[0, 1]) == c - 4


def test_atlas_uv_is_the_referee_layout():
    for T, A in list(BC.LAYOUTS) + [(7692, 1024), (0, 9)]:
        uv = atlas_uv(T, A)
        assert uv.shape == (T, 3, 2) and uv.dtype == np.float32
        assert np.array_equal(uv, BR.uv(T, A).astype(np.float32))
        if T:
            assert uv.min() > 0 and uv.max() < 1
            e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
            assert (np.sign(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) == 1).all()       # one winding for both halves
    with pytest.raises(NotImplementedError):
        atlas_uv(*BC.UNSUPPORTED)


# ------------------------------------------------------------------------------------------------------------ host checks
def test_argument_checks_raise_before_any_device_is_touched():
    """CPU tensors throughout: every rejection below comes from the host checks, in the order shapes and dtypes, the
    layout, the device."""
    v, t = (torch.from_numpy(np.array(a)) for a in BC.hand_mesh(5))
    with pytest.raises(ValueError, match="device tensors"):
        ops.bake_points(v, t, 16)
    with pytest.raises(NotImplementedError, match="at least 18"):
        ops.bake_points(v, torch.zeros(9, 3, dtype=torch.int64), 12)
    for bad in (dict(vertices=v.double()), dict(triangles=t.int()), dict(vertices=v[:, :2]), dict(triangles=t.reshape(-1)),
                dict(size=5), dict(size=8193), dict(rows=(3, 3)), dict(rows=(-1, 4)), dict(rows=(0, 17)), dict(rows=4),
                dict(vertices=v.numpy())):
        with pytest.raises(ValueError):
            ops.bake_points(**{**dict(vertices=v, triangles=t, size=16), **bad})
    face = torch.zeros(4, 16, dtype=torch.int32)
    col, lab, pal = torch.zeros(3, 64), torch.zeros(64, dtype=torch.int32), torch.zeros(3, 3)
    with pytest.raises(ValueError, match="device tensors"):
        ops.bake_resolve(face, color=col)
    with pytest.raises(ValueError, match="device tensors"):
        ops.bake_resolve(face, labels=lab, palette=pal)
    for bad in (dict(), dict(color=col, labels=lab, palette=pal), dict(color=col, palette=pal), dict(labels=lab),
                dict(color=col[:, :63]), dict(color=col.double()), dict(labels=lab.long(), palette=pal),
                dict(labels=lab[:5], palette=pal), dict(labels=lab, palette=pal[:0]), dict(labels=lab, palette=pal[:, :2]),
                dict(color=col, fill=(1, 2)), dict(color=col, neutral="grey"),
                dict(color=col, out=(torch.zeros(4, 16, 3, dtype=torch.uint8), None)),
                dict(color=col, out=(torch.zeros(4, 16, 4, dtype=torch.uint8), torch.zeros(4, 16, 4)))):
        with pytest.raises(ValueError):
            ops.bake_resolve(face, **bad)
    with pytest.raises(ValueError):
        ops.bake_resolve(face.long(), color=col)
    R = 8
    f, b, n = torch.zeros(R, R, dtype=torch.int64), torch.zeros(R, R, 3), torch.zeros(R, R, 3)
    tex8, tex32 = torch.zeros(16, 16, 4, dtype=torch.uint8), torch.zeros(16, 16, 3)
    ok = dict(pix_to_face=f, bary=b, normals=n, vertices=v, triangles=t, texture=tex8)
    for tex in (tex8, tex32):
        with pytest.raises(ValueError, match="device tensors"):
            ops.shade_textured(**{**ok, "texture": tex})
    with pytest.raises(NotImplementedError):
        ops.shade_textured(**{**ok, "triangles": torch.zeros(9, 3, dtype=torch.int64), "texture": tex8[:12, :12]})
    for bad in (dict(texture=tex8[..., :3]), dict(texture=tex32[:, :15]), dict(texture=tex8.int()), dict(texture=tex8[:5, :5]),
                dict(pix_to_face=f.int()), dict(pix_to_face=f[:7]), dict(bary=b[:7]), dict(normals=n[..., :2]),
                dict(vertices=v.double()), dict(triangles=t[:, :2]), dict(background=(1, 2)), dict(texture=None)):
        with pytest.raises(ValueError):
            ops.shade_textured(**{**ok, **bad})


# --------------------------------------------------------------------------------------------------------------- export_glb
def _dyadic_rig(K=4):
    """a rig whose every number is a short binary fraction and whose rest rotations are signed permutations: the bytes
    export_glb writes for it involve no library routine whose last bit could differ from one machine to the next"""
    P, V, T = 5, 12, 7
    grid = np.arange(V * 3).reshape(V, 3)
    v = ((grid * 37 % 64) / 32.0 - 1.0).astype(np.float32)
    tris = np.array([[(5 * i + k * (i % 3 + 1)) % V for k in range(3)] for i in range(T)], np.int64)
    joints = np.array([[(i + 2 * k) % P for k in range(K)] for i in range(V)], np.int32)
    w = np.tile(np.array([0.5, 0.25, 0.125, 0.125] + [0.0] * (K - 4), np.float32), (V, 1))
    joints[::4, 3] = -1
    w[::4] = np.array([0.5, 0.25, 0.25] + [0.0] * (K - 3), np.float32)
    rots = [np.eye(3), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, -1, 0], [0, 0, -1]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]],
            [[-1, 0, 0], [0, 0, 1], [0, 1, 0]]]
    rest = np.tile(np.eye(4, dtype=np.float32), (P, 1, 1))
    rest[:, :3, :3] = np.array(rots, np.float32)
    rest[:, :3, 3] = (np.arange(P * 3).reshape(P, 3) * 11 % 16) / 8.0 - 1.0
    bl = (np.arange(P).reshape(1, P, 1) / 4.0 + 0.5).astype(np.float32)
    colors = ((grid * 13 % 32) / 32.0).astype(np.float32)
    return RiggedMesh(torch.from_numpy(v), torch.from_numpy(tris), torch.from_numpy(joints), torch.from_numpy(w), torch.ones(V),
                      torch.from_numpy(rest)[None], torch.from_numpy(bl), colors=torch.from_numpy(colors))


# sha256 of the file export_glb wrote for _dyadic_rig() before it took a texture or clips
OLD_GLB_SHA256 = "bad80c1adda389c224dde2d252abd8b054103ae1e27645ed98569930cbdc8978"


def test_export_glb_without_texture_or_clips_writes_the_old_bytes(tmp_path):
    rig = _dyadic_rig()
    paths = [str(tmp_path / f"{i}.glb") for i in range(3)]
    export_glb(rig, paths[0])                                                # the call every earlier caller makes
    export_glb(rig, paths[1], None, None)
    export_glb(rig, paths[2], texture=None, clips={})
    raw = [open(p, "rb").read() for p in paths]
    assert raw[0] == raw[1] == raw[2]
    assert hashlib.sha256(raw[0]).hexdigest() == OLD_GLB_SHA256
    doc, _ = _parse_glb(paths[0])
    assert not {"animations", "materials", "textures", "samplers", "images"} & set(doc)
    assert "COLOR_0" in doc["meshes"][0]["primitives"][0]["attributes"]


def _decode_png(raw):
    """an 8-bit RGBA PNG without filtering -> (H, W, 4) uint8; every chunk's CRC is checked"""
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        n, kind = struct.unpack_from(">I4s", raw, at)
        data = raw[at + 8:at + 8 + n]
        assert struct.unpack_from(">I", raw, at + 8 + n)[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        chunks.append((kind, data))
        at += 12 + n
    assert at == len(raw) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, kind, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, kind, comp, filt, lace) == (8, 6, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT")), np.uint8).reshape(h, 1 + 4 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 4)


@pytest.mark.parametrize("how", ["argument", "rig"])
def test_export_glb_with_a_texture(tmp_path, how):
    rig = _dyadic_rig()
    T, A = len(rig.triangles), 21
    rng = np.random.default_rng(4)
    pixels = rng.integers(0, 256, (A, A, 4)).astype(np.uint8)
    atlas = TextureAtlas(torch.from_numpy(pixels), None, T, A, ops.bake_layout(T, A).cell)
    path = str(tmp_path / "textured.glb")
    if how == "argument":
        export_glb(rig, path, texture=atlas)
    else:
        rig.texture = atlas
        export_glb(rig, path)
    doc, blob = _parse_glb(path)
    prim = doc["meshes"][0]["primitives"][0]
    att = prim["attributes"]
    assert sorted(att) == ["JOINTS_0", "POSITION", "TEXCOORD_0", "WEIGHTS_0"] and prim["material"] == 0
    corner = rig.triangles.numpy().reshape(-1)
    assert np.array_equal(_accessor(doc, blob, att["POSITION"]), rig.vertices.numpy()[corner])
    assert doc["accessors"][att["POSITION"]]["count"] == 3 * T
    idx = _accessor(doc, blob, prim["indices"]).reshape(-1)
    assert np.array_equal(idx, np.arange(3 * T))
    uv_acc = doc["accessors"][att["TEXCOORD_0"]]
    assert uv_acc["type"] == "VEC2" and uv_acc["componentType"] == 5126 and uv_acc["count"] == 3 * T
    view = doc["bufferViews"][uv_acc["bufferView"]]
    uv = np.frombuffer(blob, "<f4", 6 * T, view["byteOffset"]).reshape(T, 3, 2)
    assert np.array_equal(uv, atlas_uv(T, A)) and np.array_equal(uv, BR.uv(T, A).astype(np.float32))
    joints, weights = rig.joints.numpy(), rig.weights.numpy()
    assert np.array_equal(_accessor(doc, blob, att["JOINTS_0"]), np.where(joints >= 0, joints, 0)[corner])
    assert np.array_equal(_accessor(doc, blob, att["WEIGHTS_0"]), np.where(joints >= 0, weights, 0)[corner])
    assert doc["materials"] == [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0,
                                                          "roughnessFactor": 1.0}}]
    assert doc["samplers"] == [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
    assert doc["textures"] == [{"sampler": 0, "source": 0}]
    assert len(doc["images"]) == 1 and doc["images"][0]["mimeType"] == "image/png"
    view = doc["bufferViews"][doc["images"][0]["bufferView"]]
    assert view["byteOffset"] % 4 == 0 and "target" not in view
    png = blob[view["byteOffset"]:view["byteOffset"] + view["byteLength"]]
    assert np.array_equal(_decode_png(png), pixels)
    from PIL import Image
    import io
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGBA")), pixels)
    with pytest.raises(ValueError):
        export_glb(rig, path, texture=TextureAtlas(atlas.texture, None, T + 1, A, 6))
    with pytest.raises(ValueError):
        export_glb(rig, path, texture=TextureAtlas(atlas.texture[:20], None, T, A, 10))


def _turn(axis, angle):
    """Rodrigues' rotation about a unit axis, float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def test_export_glb_with_a_clip_reproduces_the_skinning_at_every_key(tmp_path):
    """A viewer that plays the clip sets node k to the key's (translation, rotation, scale); with the file's own joints,
    weights and inverse bind matrices, vertex = sum_j w_j G_j (IBM_j v), which must be the referee's linear-blend skinning
    (tests/skin_reference.py) of the float64 poses the clip was made from.

    The bound. eps = 2^-24 is the relative rounding of one stored fp32 component; the weights and positions are fp32 to
    begin with, so they are stored exactly. With |.| the Euclidean norm, Vmax the largest |v|, Ta and Tb the largest rest
    and key translations, rho the largest scale and Y = Vmax + Ta >= |IBM v|:
      y = IBM v        rows of R^T and the offset -R^T t each off by eps relative: |dy|_inf <= eps (sqrt3 Vmax + Ta) =: e_y
      R(q) y           an entry of R(q) is 1 - 2 (a a + b b) or 2 (a b +- c d) of the unit quaternion's components, each off
                       by eps relative: an entry is off by at most 4 eps, so |dR y|_inf <= 4 eps |y|_1 <= 4 sqrt3 eps Y
      R dy             |R dy|_inf <= |dy| <= sqrt3 e_y
      scale            off by eps relative: eps rho Y;   translation: eps Tb
    summed with weights that add up to one: bound = rho (sqrt3 e_y + 4 sqrt3 eps Y + eps Y) + eps Tb, times 1.01 for the
    second-order terms and the float64 arithmetic on both sides. Measured: 2.8e-07 against a bound of 3.9e-06."""
    rng = np.random.default_rng(3)
    P, V, K, F = 6, 120, 4, 9
    v, joints, w = _rig(rng, V=V, P=P, K=K)
    v32, w32 = v.astype(np.float32), w.astype(np.float32)
    tris = rng.integers(0, V, (30, 3))
    rest = np.tile(np.eye(4), (P, 1, 1))
    rest[:, :3, :3] = [_turn(rng.standard_normal(3), rng.uniform(0, 3)) for _ in range(P)]
    rest[:, :3, 3] = rng.standard_normal((P, 3)) * 0.5
    bl = rng.random((1, P, 1)) + 0.5
    # every part turns through 1.8 pi about its own axis over the clip: w = cos(angle / 2) of the key's quaternion changes
    # sign on the way, so _quaternion's w >= 0 convention alone would make consecutive keys jump
    axes = rng.standard_normal((P, 3))
    poses = np.tile(rest, (F, 1, 1, 1))
    for i in range(F):
        for k in range(P):
            poses[i, k, :3, :3] = _turn(axes[k], 1.8 * np.pi * i / (F - 1)) @ rest[k, :3, :3]
        poses[i, :, :3, 3] += 0.1 * i * rng.standard_normal((P, 3))
    lengths = bl * (1 + 0.3 * rng.random((F, P, 1)))
    times = np.arange(F) / 4.0
    rig = RiggedMesh(torch.from_numpy(v32), torch.from_numpy(tris), torch.from_numpy(joints), torch.from_numpy(w32),
                     torch.ones(V), torch.from_numpy(rest)[None], torch.from_numpy(bl))
    path = str(tmp_path / "clip.glb")
    export_glb(rig, path, clips={"walk": (times, poses, lengths), "still": (times[:1], poses[:1], bl)})
    doc, blob = _parse_glb(path)
    assert [a["name"] for a in doc["animations"]] == ["walk", "still"]
    att = doc["meshes"][0]["primitives"][0]["attributes"]
    pos = _accessor(doc, blob, att["POSITION"]).astype(np.float64)
    gj, gw = _accessor(doc, blob, att["JOINTS_0"]), _accessor(doc, blob, att["WEIGHTS_0"]).astype(np.float64)
    skin = doc["skins"][0]
    ibm = _accessor(doc, blob, skin["inverseBindMatrices"]).reshape(P, 4, 4).transpose(0, 2, 1).astype(np.float64)
    walk = doc["animations"][0]
    assert len(walk["channels"]) == 3 * P == len(walk["samplers"])
    keys = {}
    for ch in walk["channels"]:
        s = walk["samplers"][ch["sampler"]]
        assert s["interpolation"] == "LINEAR"
        clock = doc["accessors"][s["input"]]
        assert clock["min"] == [0.0] and clock["max"] == [float(times[-1])] and clock["count"] == F
        assert np.array_equal(_accessor(doc, blob, s["input"]).reshape(-1), times.astype(np.float32))
        keys[ch["target"]["node"], ch["target"]["path"]] = _accessor(doc, blob, s["output"]).astype(np.float64)
    assert sorted(keys) == sorted((skin["joints"][k], p) for k in range(P) for p in ("translation", "rotation", "scale"))
    flips = 0
    for k in range(P):
        q = keys[k, "rotation"]
        assert q.shape == (F, 4) and np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-6
        assert ((q[1:] * q[:-1]).sum(-1) >= 0).all(), f"node {k}: a key turns the long way round"
        flips += int((q[:, 3] < 0).sum())
        s = keys[k, "scale"]
        assert (s[:, 0] == s[:, 1]).all() and (s[:, 0] == s[:, 2]).all()
        assert np.array_equal(s[:, 0], (lengths[:, k, 0] / bl[0, k, 0]).astype(np.float32).astype(np.float64))
    assert flips > 0                                        # the sign rule was needed
    eps = 2.0 ** -24
    Vmax, Ta = np.linalg.norm(v32, axis=1).max(), np.linalg.norm(rest[:, :3, 3], axis=1).max()
    Tb, rho = np.linalg.norm(poses[:, :, :3, 3], axis=-1).max(), (lengths / bl).max()
    Y = Vmax + Ta
    e_y = eps * (np.sqrt(3) * Vmax + Ta)
    bound = 1.01 * (rho * (np.sqrt(3) * e_y + 4 * np.sqrt(3) * eps * Y + eps * Y) + eps * Tb)
    want = SK.pose(v32, joints, w32, SK.records(rest[None], bl), SK.records(poses, lengths))
    vh = np.concatenate([pos, np.ones((V, 1))], axis=1)
    worst = 0.0
    for i in range(F):
        G = np.tile(np.eye(4), (P, 1, 1))
        for k in range(P):
            G[k, :3, :3] = _quat_matrix(keys[k, "rotation"][i]) * keys[k, "scale"][i, 0]
            G[k, :3, 3] = keys[k, "translation"][i]
        M = G @ ibm
        viewer = np.einsum("vk,vkij,vj->vi", gw, M[gj], vh)[:, :3]
        worst = max(worst, np.abs(viewer - want[i]).max())
    print(f"clip keys against the referee's LBS: {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    # the one-key clip, and what a clip must look like
    still = doc["animations"][1]
    assert doc["accessors"][still["samplers"][0]["input"]]["count"] == 1
    for bad in ((times, poses[:-1], lengths), (times, poses, lengths[:3]), (times[:0], poses[:0], bl), (times, poses[:, :5], bl)):
        with pytest.raises(ValueError):
            export_glb(rig, path, clips={"bad": bad})
