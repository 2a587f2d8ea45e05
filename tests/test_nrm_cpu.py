"""CPU checks of the field normals (libenarf_nrm.so): every argument check of the binding raises before
any device is touched, the float64 ray referee (tests/nrm_reference.py) obeys its own rules on a hand-written case and
tells three planted bugs from the contract on the very inputs the GPU test uses, and the mesh writers carry normals. The
kernels themselves are held to the referees in tests/test_gpu_nrm.py."""
import json
import struct

import numpy as np
import pytest
import torch

import geom_reference as GR
import nrm_reference as NR
from enarf_gan_amd import _nrm_lib, ops
from enarf_gan_amd._loader import EnarfHipError

P, H, W = 23, 8, 8


def _gradient_inputs(B=2, N=5):
    return dict(points=torch.zeros(B, 3, N), parts=torch.zeros(B, P, 16), canonical_pose=torch.zeros(P, 4, 4),
                tri_nchw=torch.zeros(B, 96 + 3 * P, H, W), feat_cl=torch.zeros(B, 3, H, W, 32),
                mlp_pack=torch.zeros(B, _nrm_lib.PACK_BYTES, dtype=torch.uint8))


@pytest.mark.parametrize("name,bad,exc", [
    ("points", torch.zeros(2, 4, 5), ValueError),
    ("points", torch.zeros(3, 5), ValueError),
    ("parts", torch.zeros(2, P, 15), ValueError),
    ("parts", torch.zeros(1, P, 16), ValueError),
    ("parts", torch.zeros(2, 33, 16), ValueError),
    ("canonical_pose", torch.zeros(P + 1, 4, 4), ValueError),
    ("tri_nchw", torch.zeros(2, 96 + 3 * P + 1, H, W), ValueError),
    ("tri_nchw", torch.zeros(3, 96 + 3 * P, H, W), ValueError),
    ("tri_nchw", torch.zeros(2, 96 + 3 * P, 1, W), ValueError),
    ("feat_cl", torch.zeros(2, 3, H, W, 16), ValueError),
    ("mlp_pack", torch.zeros(2, 100, dtype=torch.uint8), ValueError),
])
def test_field_gradient_rejects_wrong_shapes_without_a_device(name, bad, exc):
    a = _gradient_inputs()
    a[name] = bad
    with pytest.raises(exc):
        ops.field_gradient(**a)


def test_field_gradient_rejects_host_tensors_and_wrong_dtypes_without_a_device():
    with pytest.raises(EnarfHipError, match="device tensors"):
        ops.field_gradient(**_gradient_inputs())
    with pytest.raises(NotImplementedError):
        _nrm_lib.check_gradient_args((65536, 3, 1), (65536, P, 16), (P, 4, 4), (1, 96 + 3 * P, H, W), (1, 3, H, W, 32),
                                     (65536, _nrm_lib.PACK_BYTES))
    assert _nrm_lib.check_gradient_args((2, 3, 0), (2, P, 16), (P, 4, 4), (1, 96 + 3 * P, H, W), (1, 3, H, W, 32),
                                        (2, _nrm_lib.PACK_BYTES)) == (2, 0, P, H, W)


def _ray_inputs(B=2, n=4, Nf=3):
    return dict(gradient=torch.zeros(B, 3, n * Nf), weights=torch.zeros(B, n, Nf - 1), mask=torch.zeros(B, n))


@pytest.mark.parametrize("change,exc", [
    (dict(gradient=torch.zeros(2, 3, 11)), ValueError),
    (dict(gradient=torch.zeros(2, 12, 3)), ValueError),
    (dict(gradient=torch.zeros(2, 3, 12, dtype=torch.float64)), ValueError),
    (dict(weights=torch.zeros(2, 5, 2)), ValueError),
    (dict(weights=torch.zeros(2, 4, 0), gradient=torch.zeros(2, 3, 4)), NotImplementedError),          # Nf = 1
    (dict(weights=torch.zeros(2, 4, 128), gradient=torch.zeros(2, 3, 4 * 129)), NotImplementedError),  # Nf = 129
    (dict(mask=torch.zeros(8)), ValueError),
    (dict(mask=np.zeros((2, 4), np.float32)), ValueError),
    (dict(fallback=torch.zeros(2, 4, 3)), ValueError),                                                  # without its flags
    (dict(flags=torch.zeros(2, 4, dtype=torch.uint8)), ValueError),                                     # without normals
    (dict(fallback=torch.zeros(2, 4, 3), flags=torch.zeros(2, 4, dtype=torch.int32)), ValueError),
    (dict(fallback=torch.zeros(2, 4, 2), flags=torch.zeros(2, 4, dtype=torch.uint8)), ValueError),
    (dict(fallback=torch.zeros(2, 4, 3), flags=torch.zeros(2, 5, dtype=torch.uint8)), ValueError),
    (dict(points=torch.zeros(2, 5, 3)), ValueError),
    (dict(shade="depth"), ValueError),
    (dict(shade="lit"), ValueError),                                                                     # without points
    (dict(shade="normal", background=(1, 2)), ValueError),
    (dict(min_gradient="much"), ValueError),
    (dict(mask_threshold=None), ValueError),
])
def test_ray_normals_rejects_what_it_does_not_take_without_a_device(change, exc):
    with pytest.raises(exc):
        ops.ray_normals(**{**_ray_inputs(), **change})


def test_ray_normals_rejects_host_tensors_and_large_batches_without_a_device():
    with pytest.raises(EnarfHipError, match="device tensors"):
        ops.ray_normals(**_ray_inputs())
    with pytest.raises(NotImplementedError, match="65535"):
        ops.ray_normals(torch.zeros(65536, 3, 2), torch.zeros(65536, 1, 1), torch.zeros(65536, 1))
    g, w, m = (torch.zeros(2, 3, 12), torch.zeros(2, 1, 4, 2), torch.zeros(2, 2, 2))
    assert _nrm_lib.check_ray_args(g, w, m, None, None, None, None) == (2, 4, 3)       # the march's (B, 1, n, Nf - 1); (B, H, W)


def test_the_ray_referee_follows_its_rules_on_a_hand_written_ray():
    """two samples count (Nf = 3): G = 0.5 (0, 0, -2) + 0.25 (0, 4, 0) = (0, 1, -1), the third sample is not read"""
    g = np.zeros((1, 3, 1, 3), np.float32)
    g[0, :, 0, 0], g[0, :, 0, 1], g[0, :, 0, 2] = (0, 0, -2), (0, 4, 0), (100, 100, 100)
    w = np.float32([[[0.5, 0.25]]])
    fb, fl = np.float32([[[0, 0, -1]]]), np.uint8([[3]])
    out = NR.ray_normals(g.reshape(1, 3, 3), w, np.float32([[1.0]]), fb, fl, shade="normal")
    r = 1 / np.sqrt(2)
    assert np.allclose(out["normals"][0, 0], [0, -r, r], rtol=0, atol=1e-15) and out["magnitude"][0, 0] == np.sqrt(2.0)
    assert out["flags"][0, 0] == 7 and out["image"][0, 0].tolist() == [127, int(255 * (0.5 + 0.5 * r)), int(255 * (0.5 - 0.5 * r))]
    below = NR.ray_normals(g.reshape(1, 3, 3), w, np.float32([[0.4]]), fb, fl, shade="normal")       # the fallback
    assert below["normals"][0, 0].tolist() == [0, 0, -1] and below["flags"][0, 0] == 3 and below["image"][0, 0].tolist() == [127, 127, 255]
    none = NR.ray_normals(g.reshape(1, 3, 3), w, np.float32([[0.4]]), fb, np.uint8([[5]]), shade="normal", background=(1, 0.5, 0))
    assert not none["normals"].any() and none["flags"][0, 0] == 1 and none["image"][0, 0].tolist() == [255, 127, 0]
    high = NR.ray_normals(g.reshape(1, 3, 3), w, np.float32([[1.0]]), min_gradient=1.5)               # m = 1.41 <= 1.5
    assert not high["normals"].any() and high["flags"][0, 0] == 0
    g[0, :, 0, 0], g[0, :, 0, 1] = (0, 0, 2), (0, 0, 0)                                                 # G = (0, 0, 1), N = (0, 0, -1)
    lit = NR.ray_normals(g.reshape(1, 3, 3), w, np.float32([[1.0]]), points=np.float32([[[0, 0, 2]]]), shade="lit")
    assert lit["image"][0, 0].tolist() == [255] * 3                                                     # facing the eye: 0.5 + 0.3 + 0.2
    away = NR.ray_normals(g.reshape(1, 3, 3), w, np.float32([[1.0]]), points=np.float32([[[0, 0, -2]]]), shade="lit")
    assert away["image"][0, 0].tolist() == [127] * 3                                                    # facing away: ambient only


@pytest.mark.parametrize("n,Nf", NR.RAY_CASES)
@pytest.mark.parametrize("wrong", NR.WRONG)
def test_the_ray_referee_tells_planted_bugs_from_the_contract(n, Nf, wrong):
    """on the GPU test's inputs each wrong variant moves at least one ray's normal by more than one fp32 step: a kernel
    with that bug could not pass tests/test_gpu_nrm.py"""
    c = NR.ray_case(n, Nf)
    kw = dict(fallback=c["fallback"], flags=c["flags"])
    right = NR.ray_normals(c["gradient"], c["weights"], c["mask"], **kw)
    bad = NR.ray_normals(c["gradient"], c["weights"], c["mask"], wrong=wrong, **kw)
    steps = GR.ulps_from(bad["normals"].astype(np.float32), right["normals"]).max(axis=-1)
    print(f"{wrong} at n = {n}, Nf = {Nf}: {int((steps > 1).sum())} of {steps.size} rays more than one step away")
    assert (steps > 1).any()
    kinds = c["kind"]
    assert all((kinds == k).any() for k in range(5)) or n == 1
    assert ((c["flags"] & 2) > 0).any() and ((c["flags"] & 2) == 0).any() or n == 1


def _parse_glb(path):
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack("<4sII", raw[:12])
    assert magic == b"glTF" and version == 2 and total == len(raw)
    n_json, kind = struct.unpack("<I4s", raw[12:20])
    assert kind == b"JSON"
    doc = json.loads(raw[20:20 + n_json])
    n_bin, kind = struct.unpack("<I4s", raw[20 + n_json:28 + n_json])
    assert kind == b"BIN\0"
    return doc, raw[28 + n_json:28 + n_json + n_bin]


def test_the_mesh_writers_carry_normals_and_keep_their_bytes_without(tmp_path):
    from enarf_gan_amd.libraries.NARF.mesh_rendering import RiggedMesh, export_glb, export_obj, export_ply
    rng = np.random.default_rng(3)
    v = rng.standard_normal((5, 3)).astype(np.float32)
    f = np.int64([[0, 1, 2], [2, 3, 4]])
    nrm = rng.standard_normal((5, 3)).astype(np.float32)
    for writer, name in ((export_obj, "m.obj"), (export_ply, "m.ply")):
        a, b, c = (str(tmp_path / (k + name)) for k in "abc")
        writer(v, f, a)
        writer(v, f, b, normals=None)
        writer(v, f, c, normals=nrm)
        assert open(a, "rb").read() == open(b, "rb").read() != open(c, "rb").read()
        with pytest.raises(ValueError):
            writer(v, f, c, normals=nrm[:4])
    text = open(str(tmp_path / "cm.obj")).read().splitlines()
    assert [ln for ln in text if ln.startswith("vn ")][4] == "vn %r %r %r" % tuple(float(x) for x in nrm[4])
    assert text[-1] == "f 3//3 4//4 5//5"
    ply = open(str(tmp_path / "cm.ply"), "rb").read()
    head, body = ply.split(b"end_header\n")
    assert b"property float nx" in head
    assert np.frombuffer(body[:5 * 24], "<f4").reshape(5, 6)[:, 3:].tobytes() == nrm.tobytes()
    fields = {fl.name for fl in __import__("dataclasses").fields(RiggedMesh)}
    frames = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    kw = dict(vertices=v, triangles=f, joints=np.int32([[0, 1, -1, -1]] * 5), weights=np.float32([[0.5, 0.5, 0, 0]] * 5),
              rest_pose=frames, rest_bone_length=np.ones((2, 1), np.float32))
    rig = RiggedMesh(**{k: kw.get(k) for k in fields})
    a, b, c = (str(tmp_path / (k + ".glb")) for k in "abc")
    export_glb(rig, a)
    export_glb(rig, b, normals=None)
    export_glb(rig, c, normals=nrm)
    assert open(a, "rb").read() == open(b, "rb").read()
    doc, binary = _parse_glb(c)
    acc = doc["accessors"][doc["meshes"][0]["primitives"][0]["attributes"]["NORMAL"]]
    assert acc["count"] == 5 and acc["type"] == "VEC3" and acc["componentType"] == 5126
    view = doc["bufferViews"][acc["bufferView"]]
    assert binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]] == nrm.tobytes()
    assert "NORMAL" not in _parse_glb(a)[0]["meshes"][0]["primitives"][0]["attributes"]
    with pytest.raises(ValueError):
        export_glb(rig, c, normals=nrm[:4])
