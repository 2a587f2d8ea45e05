"""CPU checks of the rigged meshes (libenarf_skin.so's host side, export_glb, the referee of the GPU tests): no GPU. The
library checks of the `skin` row (header against exports and SIGNATURES, ABI version, kernel inventory against
tests/skin_kernel_coverage.py, tracked headers, disjoint kernels) are tests/test_side_libraries_cpu.py's."""
import json
import math
import struct

import numpy as np
import pytest
import torch

import skin_reference as SK
from _helpers import Scene
from enarf_gan_amd import build, ops
from enarf_gan_amd._loader import EnarfHipError
from enarf_gan_amd.libraries.NARF.mesh_rendering import RiggedMesh, export_glb

TOL = 1e-12            # float64 properties, relative to the mesh's extent


def _rotations(rng, n):
    """n proper rotations, orthogonal to float64 rounding"""
    q, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def _frames(rng, n, spread=1.0):
    f = np.tile(np.eye(4), (n, 1, 1))
    f[:, :3, :3] = _rotations(rng, n)
    f[:, :3, 3] = rng.standard_normal((n, 3)) * spread
    return f


def _rig(rng, V=200, P=6, K=4):
    v = rng.standard_normal((V, 3))
    joints = np.stack([rng.permutation(P)[:K] for _ in range(V)]).astype(np.int32)
    w = rng.random((V, K)) + 0.05
    joints[::3, K - 1] = -1                                                  # unused slots
    w[::3, K - 1] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    return v, joints, w


def _extent(v):
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


# ------------------------------------------------------------------------------------------- properties of the referee's LBS
@pytest.mark.parametrize("cs", [1.0, 3.0])
def test_lbs_properties_hold_in_float64(cs):
    rng = np.random.default_rng(7)
    P = 6
    v, joints, w = _rig(rng, P=P)
    ext = _extent(v)
    rest, bl = _frames(rng, P)[None], rng.random((1, P)) + 0.5
    A = SK.records(rest, bl, coordinate_scale=cs)
    # the rest pose returns the vertices
    e = np.abs(SK.pose(v, joints, w, A, A, cs)[0] - v).max() / ext
    print(f"rest pose: {e:.2e}")
    assert e <= TOL
    # one rigid motion G of every part returns G v, whatever the weights
    G = _frames(rng, 1)[0]
    moved = np.einsum("ij,bpjk->bpik", G, rest)
    e = np.abs(SK.pose(v, joints, w, A, SK.records(moved, bl, coordinate_scale=cs), cs)[0] - (v @ G[:3, :3].T + G[:3, 3])).max() / ext
    print(f"common rigid motion: {e:.2e}")
    assert e <= TOL
    # one part moved, weights (1/2, 1/2): the midpoint
    two = np.array([[0, 1, -1, -1]], np.int32).repeat(len(v), 0)
    half = np.array([[0.5, 0.5, 0.0, 0.0]]).repeat(len(v), 0)
    target = rest.copy()
    target[0, 1] = G @ rest[0, 1]
    got = SK.pose(v, two, half, A, SK.records(target, bl, coordinate_scale=cs), cs)[0]
    e = np.abs(got - 0.5 * (v + (v @ G[:3, :3].T + G[:3, 3]))).max() / ext
    print(f"mixed weights: {e:.2e}")
    assert e <= TOL
    # a bone-length ratio rho scales a vertex's offset from its part origin by rho
    rho = 1.7
    bl2 = bl.copy()
    bl2[0, 2] *= rho
    only = np.array([[2, -1, -1, -1]], np.int32).repeat(len(v), 0)
    one = np.array([[1.0, 0.0, 0.0, 0.0]]).repeat(len(v), 0)
    got = SK.pose(v, only, one, A, SK.records(rest, bl2, coordinate_scale=cs), cs)[0]
    origin = rest[0, 2, :3, 3]
    e = np.abs((got - origin) - rho * (v - origin)).max() / ext
    print(f"bone-length scale: {e:.2e}")
    assert e <= TOL
    # several frames at once are the frames one by one
    both = SK.pose(v, joints, w, A, np.concatenate([A, SK.records(moved, bl2, coordinate_scale=cs)]), cs)
    assert np.array_equal(both[0], SK.pose(v, joints, w, A, A, cs)[0]) and both.shape == (2, len(v), 3)


# --------------------------------------------------------------------------------------------- the referee's weight rules
def _coincident(n=6):
    """n coincident axis-aligned parts at the origin (canonical scale 0.5) over identical part-probability planes"""
    pose = torch.eye(4).repeat(1, n, 1, 1)
    scale = torch.full((1, n), 0.5)
    cpose = torch.eye(4).repeat(n, 1, 1)
    g = torch.Generator().manual_seed(2)
    tri = torch.zeros(1, 96 + 3 * n, 8, 8)
    tri[0, 96:] = torch.randn(3, 8, 8, generator=g).repeat(n, 1, 1)
    return pose, scale, cpose, tri


def test_equal_weights_keep_the_lowest_parts():
    g = torch.Generator().manual_seed(3)
    pts = (torch.rand(1, 3, 50, generator=g) * 1.8 - 0.9).contiguous()
    r4 = SK.weights(pts, *_coincident(), K=4)
    assert (r4["n_valid"] == 6).all() and (r4["joints"] == np.arange(4)).all()
    assert (r4["weights"] == 0.25).all() and r4["ambiguous"].all()
    assert np.allclose(r4["kept_mass"], 4 / 6, rtol=0, atol=1e-15)            # 6 w is not exact in float64: one rounding
    r8 = SK.weights(pts, *_coincident(), K=8)
    assert (r8["joints"] == [0, 1, 2, 3, 4, 5, -1, -1]).all() and (r8["kept_mass"] == 1).all() and not r8["ambiguous"].any()
    assert np.allclose(r8["weights"][:, :6], 1 / 6, rtol=0, atol=1e-15) and (r8["weights"][:, 6:] == 0).all()
    d = SK.dense(r4["joints"], r4["weights"], 6)
    assert np.array_equal(d, np.tile([0.25] * 4 + [0.0] * 2, (50, 1)))


def test_an_unowned_vertex_takes_the_nearest_part():
    """two parts one unit apart in x (test_seg_cpu's scene): (5, 0.2, 0) lies outside both cubes, max |local| is 5 for
    part 0 and 4 for part 1; (-3, 0, 0) is nearer to part 0; (0.5, 3, 0) is equally far from both (|local y| = 3): the
    lowest index"""
    pose = torch.eye(4).repeat(1, 2, 1, 1)
    pose[0, 1, 0, 3] = 1.0
    scale = torch.tensor([[0.5, 1.0]])
    cpose = torch.eye(4).repeat(2, 1, 1)
    tri = torch.zeros(1, 96 + 6, 4, 4)
    tri[0, 96 + 3:] = math.log(3.0)
    pts = torch.tensor([[5.0, 0.2, 0.0], [-3.0, 0.0, 0.0], [0.5, 3.0, 0.0], [0.5, 0.0, 0.0]]).t()[None].contiguous()
    r = SK.weights(pts, pose, scale, cpose, tri, K=4)
    assert r["unowned"].tolist() == [True, True, True, False]
    assert r["joints"][:3].tolist() == [[1, -1, -1, -1], [0, -1, -1, -1], [0, -1, -1, -1]]
    assert r["weights"][:3].tolist() == [[1, 0, 0, 0]] * 3 and r["kept_mass"].tolist() == [0, 0, 0, 1]
    # the owned one: both parts, the larger weight first, normalised
    w0, w1 = 0.125, 0.75 ** 3
    assert r["joints"][3].tolist() == [1, 0, -1, -1]
    assert np.allclose(r["weights"][3], [w1 / (w0 + w1), w0 / (w0 + w1), 0, 0], rtol=0, atol=1e-7)


@pytest.mark.parametrize("ol", ["center_fixed", "center+head"])
def test_referee_ambiguity_stays_within_the_cap(ol):
    """the cap and the cut-off count of tests/test_gpu_skin.py hold for the referee itself on that file's points"""
    sc = Scene(16, 1, ol, 20)
    pts = SK.scene_points(sc)
    for K in (4, 8):
        r = SK.weights(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], K)
        many, amb = int((r["n_valid"] > K).sum()), int(r["ambiguous"].sum())
        owned = ~r["unowned"]
        print(f"{ol} K={K}: {amb} ambiguous of {many} with more than K valid parts, {int(r['unowned'].sum())} unowned, "
              f"kept sum >= {r['kept_sum'][owned].min():.4f}, mean kept_mass there {r['kept_mass'][r['n_valid'] > K].mean():.3f}")
        assert many > 1000 and amb <= SK.MAX_AMBIGUOUS * many and int(r["unowned"].sum()) == 34
        assert r["kept_sum"][owned].min() >= 0.126
        assert np.allclose(r["weights"].sum(axis=1), 1.0, rtol=0, atol=1e-12)


# --------------------------------------------------------------------------------------------------------------- export_glb
def _parse_glb(path):
    raw = open(path, "rb").read()
    magic, version, length = struct.unpack_from("<4sII", raw, 0)
    assert magic == b"glTF" and version == 2 and length == len(raw) and length % 4 == 0
    n_json, kind = struct.unpack_from("<I4s", raw, 12)
    assert kind == b"JSON" and n_json % 4 == 0
    doc = json.loads(raw[20:20 + n_json].decode("utf-8"))
    n_bin, kind = struct.unpack_from("<I4s", raw, 20 + n_json)
    assert kind == b"BIN\0" and n_bin % 4 == 0 and 20 + n_json + 8 + n_bin == len(raw)
    assert doc["buffers"] == [{"byteLength": n_bin}]
    return doc, raw[28 + n_json:]

_COMPONENT = {5126: ("<f4", 4), 5121: ("u1", 1), 5125: ("<u4", 4)}
_WIDTH = {"SCALAR": 1, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def _accessor(doc, blob, index):
    acc = doc["accessors"][index]
    view = doc["bufferViews"][acc["bufferView"]]
    dtype, size = _COMPONENT[acc["componentType"]]
    width = _WIDTH[acc["type"]]
    assert view["byteOffset"] % 4 == 0 and view["byteLength"] == acc["count"] * width * size
    assert view["byteOffset"] + view["byteLength"] <= len(blob)
    return np.frombuffer(blob, dtype, acc["count"] * width, view["byteOffset"]).reshape(acc["count"], width)


def _quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("K", [4, 8])
def test_glb_round_trip_reproduces_the_skinning(tmp_path, K):
    rng = np.random.default_rng(11 + K)
    P, V = 23, 150
    v, joints, w = _rig(rng, V=V, P=P, K=K)
    v32, w32 = v.astype(np.float32), w.astype(np.float32)
    tris = rng.integers(0, V, (40, 3))
    rest, bl = _frames(rng, P, 0.5).astype(np.float32), (rng.random((1, P, 1)) + 0.5).astype(np.float32)
    colors = rng.random((V, 3)).astype(np.float32)
    rig = RiggedMesh(torch.from_numpy(v32), torch.from_numpy(tris), torch.from_numpy(joints), torch.from_numpy(w32),
                     torch.ones(V), torch.from_numpy(rest)[None], torch.from_numpy(bl), colors=torch.from_numpy(colors))
    path = str(tmp_path / "rig.glb")
    export_glb(rig, path)
    doc, blob = _parse_glb(path)
    prim = doc["meshes"][0]["primitives"][0]
    att = prim["attributes"]
    assert sorted(att) == sorted(["POSITION", "COLOR_0"] + [f"{n}_{s}" for n in ("JOINTS", "WEIGHTS") for s in range(K // 4)])
    pos = _accessor(doc, blob, att["POSITION"])
    assert np.array_equal(pos, v32) and np.array_equal(_accessor(doc, blob, att["COLOR_0"]), colors)
    pa = doc["accessors"][att["POSITION"]]
    assert pa["count"] == V and pa["min"] == v32.min(axis=0).tolist() and pa["max"] == v32.max(axis=0).tolist()
    idx = _accessor(doc, blob, prim["indices"])
    assert doc["accessors"][prim["indices"]]["count"] == 120 and np.array_equal(idx.reshape(-1, 3), tris)
    gj = np.concatenate([_accessor(doc, blob, att[f"JOINTS_{s}"]) for s in range(K // 4)], axis=1)
    gw = np.concatenate([_accessor(doc, blob, att[f"WEIGHTS_{s}"]) for s in range(K // 4)], axis=1)
    assert gj.dtype == np.uint8 and gj.shape == (V, K) and gw.shape == (V, K)
    assert np.array_equal(gj, np.where(joints >= 0, joints, 0)) and np.array_equal(gw, np.where(joints >= 0, w32, 0))
    skin = doc["skins"][0]
    assert skin["joints"] == list(range(P)) and doc["accessors"][skin["inverseBindMatrices"]]["count"] == P
    ibm = _accessor(doc, blob, skin["inverseBindMatrices"]).reshape(P, 4, 4).transpose(0, 2, 1).astype(np.float64)   # column-major
    mesh_node = [n for n in doc["nodes"] if "mesh" in n]
    assert len(mesh_node) == 1 and mesh_node[0]["skin"] == 0 and "animations" not in doc
    for k in range(P):                                                      # the bind pose is the rest pose
        node = doc["nodes"][skin["joints"][k]]
        assert np.abs(_quat_matrix(node["rotation"]) - rest[k, :3, :3]).max() < 1e-6
        assert np.abs(np.array(node["translation"]) - rest[k, :3, 3]).max() == 0
        assert node["extras"]["bone_length"] == float(bl[0, k, 0])
    # a viewer sets node k to (t_k, R_k, scale rho_k) of a second pose: vertex = sum_j w_j (G_j IBM_j) v
    target, bl2 = _frames(rng, P, 0.5).astype(np.float32), (rng.random((1, P, 1)) + 0.5).astype(np.float32)
    rho = (bl2 / bl).astype(np.float64).reshape(P)
    G = np.tile(np.eye(4), (P, 1, 1))
    G[:, :3, :3] = target[:, :3, :3].astype(np.float64) * rho[:, None, None]
    G[:, :3, 3] = target[:, :3, 3]
    M = G @ ibm
    vh = np.concatenate([pos.astype(np.float64), np.ones((V, 1))], axis=1)
    viewer = np.einsum("vk,vkij,vj->vi", gw.astype(np.float64), M[gj], vh)[:, :3]
    want = SK.pose(v32, joints, w32, SK.records(rest[None], bl), SK.records(target[None], bl2))[0]
    e = np.abs(viewer - want).max() / _extent(want)
    print(f"K={K}: glTF skinning against the referee's LBS: {e:.2e} of the mesh's extent")
    assert e <= 1e-5
    with pytest.raises(ValueError):
        export_glb(RiggedMesh(rig.vertices, rig.triangles, rig.joints[:, :3], rig.weights[:, :3], rig.kept_mass, rig.rest_pose,
                              rig.rest_bone_length), path)


# ------------------------------------------------------------------------------------------------------ binding and host checks
def test_the_row_and_the_binding_cover_the_header():
    import re
    from enarf_gan_amd import _skin_lib
    assert build.SIDE_LIBRARIES["skin"] == (["enarf_skin.hip"], "enarf_skin.h") and list(build.SIDE_LIBRARIES)[-1] == "skin"
    header = open(build.lib_deps("skin")[-2]).read()
    declared = set(re.findall(r"\b(enarf_skin_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_skin_lib.SIGNATURES) and all(n.startswith("enarf_skin_") for n in declared)
    assert f"#define ENARF_SKIN_ABI_VERSION {_skin_lib.ABI_VERSION}\n" in header
    assert f"#define ENARF_SKIN_FRAMES_PER_GROUP  {_skin_lib.FRAMES_PER_GROUP} " in header


def test_host_side_rejections():
    P = 23
    v, parts, cpose, tri = torch.zeros(10, 3), torch.zeros(1, P, 16), torch.zeros(P, 4, 4), torch.zeros(1, 96 + 3 * P, 8, 8)
    with pytest.raises(ValueError, match="4 or 8"):
        ops.skin_weights(v, parts, cpose, tri, max_influences=5)
    with pytest.raises(ValueError, match="at most 32"):
        ops.skin_weights(v, torch.zeros(1, 33, 16), torch.zeros(33, 4, 4), torch.zeros(1, 96 + 99, 8, 8))
    with pytest.raises(ValueError):
        ops.skin_weights(torch.zeros(3, 10), parts, cpose, tri)
    with pytest.raises(ValueError, match="one identity"):
        ops.skin_weights(v, torch.zeros(2, P, 16), cpose, tri)
    with pytest.raises(ValueError):
        ops.skin_weights(v, parts, torch.zeros(24, 4, 4), tri)
    with pytest.raises(ValueError):
        ops.skin_weights(v, parts, cpose, torch.zeros(1, 96 + 3 * 24, 8, 8))
    with pytest.raises(ValueError, match="H, W >= 2"):
        ops.skin_weights(v, parts, cpose, torch.zeros(1, 96 + 3 * P, 1, 8))
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.skin_weights(v, parts, cpose, tri)
    joints, w, tgt = torch.zeros(10, 4, dtype=torch.int32), torch.zeros(10, 4), torch.zeros(5, P, 16)
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.skin_pose(v, joints, w, parts, tgt)
    for bad in (dict(joints=torch.zeros(10, 5, dtype=torch.int32)), dict(weights=torch.zeros(10, 8)), dict(joints=joints[:9]),
                dict(parts=torch.zeros(5, 24, 16)), dict(parts_rest=torch.zeros(2, P, 16)), dict(vertices=torch.zeros(10, 4)),
                dict(coordinate_scale=0.0)):
        args = {**dict(vertices=v, joints=joints, weights=w, parts_rest=parts, parts=tgt, coordinate_scale=1.0), **bad}
        cs = args.pop("coordinate_scale")
        with pytest.raises(ValueError):
            ops.skin_pose(*args.values(), coordinate_scale=cs)
