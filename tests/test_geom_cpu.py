"""CPU checks of the geometry buffers and the depth error (libenarf_geom.so): the float64 referee
(tests/geom_reference.py) against analytic scenes and hand-written buffers that plant one rule each, its depth error
against torch's MSELoss, the point-cloud writer, and every ValueError of the binding. The kernels themselves are held to
the same referee in tests/test_gpu_geom.py."""
import numpy as np
import pytest
import torch

import geom_cases as GC
import geom_reference as GR
from enarf_gan_amd import ops
from enarf_gan_amd._loader import EnarfHipError


def _run(s, **kw):
    return GR.buffers(s["disparity"][None], s["mask"][None], s["inv_intrinsics"], **kw)


def _angles(out, s):
    """(angles in degrees of the pixels with a normal, how many pixels have one)"""
    has = (out["flags"][0] & 2) > 0
    return GR.angle_deg(out["normals"][0][has], s["normal"][has]), int(has.sum())


def test_tilted_plane_normals():
    s = GC.scene("plane", 37, 53)
    out = _run(s)
    assert (out["flags"] == 3).all()
    ang, n = _angles(out, s)
    print(f"tilted plane: largest angle {ang.max():.5f} deg over {n} pixels")
    assert n == 37 * 53 and ang.max() <= 0.01
    assert (GR._dot(out["normals"], out["points"]) < 0).all()
    assert np.allclose(out["points"][0] @ GC.PLANE_NORMAL, GC.PLANE_NORMAL[2] * 3, rtol=0, atol=1e-5)   # on the plane itself


@pytest.mark.parametrize("H,W", [(64, 64), (37, 53)])
def test_sphere_normals(H, W):
    s = GC.scene("sphere", H, W)
    out = _run(s)
    assert np.array_equal(out["flags"][0] & 1, s["surface"].astype(np.uint8))
    ang, n = _angles(out, s)
    print(f"sphere {H} x {W}: median {np.median(ang):.3f} deg, {100 * (ang > 10).mean():.2f} % above 10 deg, {n} normals")
    assert n > 0.2 * H * W and np.median(ang) <= 0.5 and (ang > 10).mean() <= 0.02
    assert (GR._dot(out["normals"], out["points"])[0][(out["flags"][0] & 2) > 0] < 0).all()
    on = s["surface"]
    assert np.allclose(np.linalg.norm(out["points"][0][on] - GC.SPHERE_CENTRE, axis=-1), GC.SPHERE_RADIUS, rtol=0, atol=1e-5)
    assert (out["normals"][0][~on] == 0).all() and (out["depth"][0][~on] == 0).all() and (out["image"][0][~on] == 255).all()


def test_the_edge_rule_keeps_normals_from_bridging_a_silhouette():
    s = GC.scene("sphere_on_plane", 64, 64)
    with_edge, n_with = _angles(_run(s, edge=0.05), s)
    without, n_without = _angles(_run(s, edge=-1), s)
    print(f"sphere on plane: edge 0.05 {100 * (with_edge > 10).mean():.2f} % above 10 deg ({n_with} normals); "
          f"no edge {100 * (without > 10).mean():.2f} %, largest {without.max():.0f} deg")
    assert n_with >= 4000 and n_without == 64 * 64
    assert (with_edge > 10).mean() <= 0.01
    assert (without > 10).mean() >= 0.03


def _cross_normal(p, pix, how):
    """the normal of pixel `pix` from the points p (H, W, 3) and the neighbours HAND_DIFFERENCES names"""
    r, c = pix
    dx = p[r, c + 1 if "h" in how[0] else c] - p[r, c - 1 if "l" in how[0] else c]
    dy = p[r + 1 if "h" in how[1] else r, c] - p[r - 1 if "l" in how[1] else r, c]
    n = np.cross(dy, dx)
    n /= np.linalg.norm(n)
    return -n if n @ p[r, c] > 0 else n


def test_hand_written_buffers_rule_by_rule():
    q, m, K = GC.hand_buffer(5)
    out = GR.buffers(q[None], m[None], K)
    flags, p = out["flags"][0], out["points"][0]
    for pix in GC.HAND_INVALID:                                   # q = 0, q < 0, NaN, inf, a mask below the threshold
        assert flags[pix] == 0 and out["depth"][0][pix] == 0 and (out["normals"][0][pix] == 0).all(), pix
        assert (out["image"][0][pix] == 255).all()
    assert (flags & 1).sum() == 25 - len(GC.HAND_INVALID)
    assert flags[1, 1] == 1                                       # a mask exactly at the threshold is valid
    assert out["depth"][0][1, 1] == 0.5 / np.float64(q[1, 1])      # normalise: m / q
    for pix, how in GC.HAND_DIFFERENCES.items():
        if "" in how:
            assert flags[pix] == 1, pix                           # valid, a difference missing: no normal
        else:
            assert flags[pix] == 3, pix
            assert GR.angle_deg(out["normals"][0][pix], _cross_normal(p, pix, how)) < 1e-4, pix
    # without the edge rule the pixel at half the depth is a neighbour like any other
    loose = GR.buffers(q[None], m[None], K, edge=-1)
    assert loose["flags"][0][1, 1] == 3 and loose["flags"][0][0, 1] == 3 and loose["flags"][0][2, 1] == 3
    assert GR.angle_deg(loose["normals"][0][0, 1], _cross_normal(p, (0, 1), ("lh", "h"))) < 1e-4
    # normalise off: the disparity is the surface's own inverse depth
    plain = GR.buffers(q[None], m[None], K, normalise=False, depth_scale=2.0)
    assert plain["depth"][0][1, 1] == 2.0 / np.float64(q[1, 1]) and plain["depth"][0][2, 2] == 2.0 / np.float64(q[2, 2])
    assert plain["flags"][0][1, 1] == 3 and np.array_equal(plain["flags"] & 1, out["flags"] & 1)
    # a threshold above every mask leaves nothing
    assert (GR.buffers(q[None], m[None], K, mask_threshold=1.5)["flags"] == 0).all()


def test_the_edge_test_at_equality():
    q, m, K, edge = GC.edge_equality()
    out = GR.buffers(q[None], m[None], K, edge=edge)
    p = out["points"][0]
    assert out["depth"][0][1, 0] == 0.75 and out["depth"][0][1, 2] < 0.75
    assert out["flags"][0][1, 1] == 3
    assert GR.angle_deg(out["normals"][0][1, 1], _cross_normal(p, (1, 1), ("l", "lh"))) < 1e-4      # left usable, right not
    assert GR.angle_deg(out["normals"][0][1, 1], _cross_normal(p, (1, 1), ("lh", "lh"))) > 1
    assert out["flags"][0][1, 0] == 1 and out["flags"][0][1, 2] == 1                                # their own limits are tighter


def test_every_shade_mode():
    s = GC.scene("sphere", 37, 53)
    bg = (0.25, 0.5, 0.75)
    normal, lit = _run(s, shade="normal", background=bg), _run(s, shade="lit", background=bg)
    depth = _run(s, shade="depth", near=1.5, far=4.0, background=bg)
    has, valid = (normal["flags"][0] & 2) > 0, (normal["flags"][0] & 1) > 0
    N, z = normal["normals"][0], normal["depth"][0]
    for out in (normal, lit):
        assert (out["image"][0][~has] == [63, 127, 191]).all()
    assert (depth["image"][0][~valid] == [63, 127, 191]).all()
    want = np.floor(255 * np.clip(0.5 + 0.5 * N * [1, -1, -1], 0, 1)).astype(np.uint8)
    assert np.array_equal(normal["image"][0][has], want[has])
    centre = (18, 26)                                               # the sphere's centre faces the camera: blue-violet
    assert has[centre] and abs(int(normal["image"][0][centre][2]) - 255) <= 2 and abs(int(normal["image"][0][centre][0]) - 127) <= 20
    grey = lit["image"][0]
    assert (grey[..., 0] == grey[..., 1])[has].all() and (grey[..., 1] == grey[..., 2])[has].all()
    assert grey[has][:, 0].max() >= 230 and 127 <= grey[has][:, 0].min() < 200  # 0.5 + 0.3 + 0.2 head on, 0.5 + 0.3 c at the rim
    g = (1 / z[valid] - 1 / 4.0) / (1 / 1.5 - 1 / 4.0)
    assert np.array_equal(depth["image"][0][valid][:, 0], np.floor(255 * np.clip(g, 0, 1)).astype(np.uint8))
    assert depth["image"][0][centre][0] >= int(depth["image"][0][valid].max()) - 2 > 100   # nearest = brightest


def test_depth_error_referee_against_mse_loss():
    results, gens, targets = [], [], []
    for seed, shape in ((0, (3, 37, 53)), (1, (1, 1, 1)), (2, (2, 16, 16))):
        q, g, m = GC.error_batch(shape, seed)
        results.append(GR.depth_error(q, g, m))
        gens.append(torch.from_numpy(q).double().reshape(-1))
        targets.append(torch.from_numpy(g).double().reshape(-1))
        fg = g > 0
        assert results[-1]["n_fg"] == fg.sum() and results[-1]["inter"] == ((m >= 0.5) & fg).sum()
        assert results[-1]["union"] == ((m >= 0.5) | fg).sum()
        assert GR.depth_error(q, g)["inter"] == ((q > 0) & fg).sum()          # without a mask q > 0 is the silhouette
    total = GR.merge(results)
    want = torch.nn.MSELoss()(torch.cat(gens), torch.cat(targets)).item()
    assert total["n"] == 3 * 37 * 53 + 1 + 512 and abs(total["inv_depth_mse"] - want) <= 1e-14 * want
    q, g, m = GC.error_batch((4, 4), 3)
    q[0, 0] = np.nan
    assert np.isnan(GR.depth_error(q, g, m)["sse_all"])                       # non-finite values propagate, as in MSELoss
    assert torch.isnan(torch.nn.MSELoss()(torch.from_numpy(q), torch.from_numpy(g)))


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    count = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    kinds = {"float": "<f4", "uchar": "u1"}
    fields = [(ln.split()[2], kinds[ln.split()[1]]) for ln in lines if ln.startswith("property")]
    assert not any(ln.startswith("element face") for ln in lines)
    vert = np.frombuffer(body, dtype=fields)
    assert len(vert) == count
    return vert


def test_point_cloud_round_trip(tmp_path):
    from enarf_gan_amd.libraries.NARF.mesh_rendering import export_point_cloud
    s = GC.scene("sphere", 37, 53)
    out = _run(s, shade="lit")
    points, normals = out["points"].astype(np.float32), out["normals"].astype(np.float32)
    keep = (out["flags"] & 1) > 0
    path = str(tmp_path / "cloud.ply")
    export_point_cloud(torch.from_numpy(points), torch.from_numpy(out["flags"]), path, colors=torch.from_numpy(out["image"]),
                       normals=normals)
    vert = _read_ply(path)
    assert len(vert) == keep.sum() and vert.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), points[keep])
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), normals[keep])
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), out["image"][keep])
    export_point_cloud(points[0], out["flags"][0], path, colors=np.full(points[0].shape, 0.5))      # floats in [0, 1]
    vert = _read_ply(path)
    assert vert.dtype.names == ("x", "y", "z", "red", "green", "blue") and (vert["green"] == 127).all()
    export_point_cloud(points, np.zeros_like(out["flags"]), path)                                   # nothing valid: a header
    assert len(_read_ply(path)) == 0
    for bad in (dict(flags=out["flags"][0]), dict(normals=normals[0]), dict(colors=out["image"][..., :2])):
        with pytest.raises(ValueError):
            export_point_cloud(**{**dict(points=points, flags=out["flags"], path=path), **bad})


def test_host_side_rejections():
    """every ValueError of the binding is raised from shapes, dtypes and values alone, before any device is asked for; what
    passes them on CPU tensors meets 'no CPU fallback'"""
    q, m, K = torch.ones(2, 4, 5), torch.ones(2, 4, 5), torch.eye(3)
    bad = [dict(disparity=q.double()), dict(mask=m.half()), dict(inv_intrinsics=K.double()), dict(disparity=q.numpy()),
           dict(disparity=torch.ones(4, 5), mask=torch.ones(4, 5)), dict(mask=torch.ones(2, 5, 4)), dict(inv_intrinsics=torch.ones(3, 3, 3)),
           dict(inv_intrinsics=torch.ones(2, 3, 4)), dict(inv_intrinsics=torch.ones(9)), dict(size=(5, 4)), dict(size=5),
           dict(disparity=torch.ones(2, 20), mask=torch.ones(2, 20)), dict(origin=3), dict(origin=(1, 2, 3)), dict(step="wide"),
           dict(shade="phong"), dict(shade="depth"), dict(shade="depth", near=1.0), dict(shade="depth", near=2.0, far=2.0),
           dict(shade="depth", near=-1.0, far=2.0), dict(want=()), dict(want=("depth", "albedo")), dict(background=(1, 2)),
           dict(background="white"), dict(edge=None), dict(depth_scale="one"), dict(mask_threshold=None),
           dict(out={"points": torch.zeros(2, 4, 5, 3)}, want=("depth",)), dict(out={"depth": torch.zeros(2, 5, 4)}),
           dict(out={"image": torch.zeros(2, 4, 5, 3)}), dict(out={"depth": torch.zeros(2, 4, 10)[:, :, ::2]})]
    for b in bad:
        with pytest.raises(ValueError):
            ops.geometry_buffers(**{**dict(disparity=q, mask=m, inv_intrinsics=K), **b})
    with pytest.raises(ValueError, match=r"outside \[1, 4096\]"):
        ops.geometry_buffers(torch.ones(1, 1, 1).expand(1, 4097, 2), torch.ones(1, 1, 1).expand(1, 4097, 2), K)
    with pytest.raises(ValueError, match=r"outside \[1, 4096\]"):
        ops.geometry_buffers(torch.ones(1, 0, 4), torch.ones(1, 0, 4), K)
    with pytest.raises(ValueError, match=r"2\^31"):
        ops.geometry_buffers(torch.ones(1, 1, 1).expand(128, 4096, 4096), torch.ones(1, 1, 1).expand(128, 4096, 4096), K)
    with pytest.raises(ValueError, match=r"2\^31"):
        ops.geometry_buffers(torch.ones(0, 4, 5), torch.ones(0, 4, 5), K)
    for ok in (dict(), dict(size=(4, 5)), dict(disparity=torch.ones(2, 20), mask=torch.ones(2, 20), size=(4, 5)),
               dict(inv_intrinsics=torch.ones(2, 3, 3)), dict(shade="depth", near=1, far=2), dict(shade="depth", want=("depth",))):
        with pytest.raises(EnarfHipError, match="no CPU fallback"):
            ops.geometry_buffers(**{**dict(disparity=q, mask=m, inv_intrinsics=K), **ok})
    assert ops.GeometryBuffers._fields == ("depth", "points", "normals", "flags", "image")
    err = ops.DepthError()
    for args in ((q.double(), q), (q, q.half()), (q, q, m.double()), (q, torch.ones(2, 5, 4)), (q, q, torch.ones(2, 4)),
                 (q.numpy(), q), (torch.ones(0, 4), torch.ones(0, 4))):
        with pytest.raises(ValueError):
            err.update(*args)
    with pytest.raises(ValueError):
        ops.DepthError(mask_threshold="half")
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        err.update(q, q, m)
    empty = err.result()                                             # nothing added, no device asked for
    assert empty["n"] == 0 and np.isnan(empty["inv_depth_mse"]) and np.isnan(empty["iou"])
    from enarf_gan_amd import _geom_lib
    lib = _geom_lib.load()
    for n in (0, 1, 2048, 2049, 37 * 53 * 3, 2 ** 21, 2 ** 21 + 1, 2 ** 31 - 1, 2 ** 31, -5):
        assert lib.enarf_geom_err_records(n) == _geom_lib.err_records(n), n


def test_the_c_abi_refuses_sizes_and_null_pointers_before_any_launch():
    """ENARF_ERR_ARG from the host checks alone: no device is needed to be refused"""
    import ctypes as C
    from enarf_gan_amd import _geom_lib
    lib = _geom_lib.load()

    def args(**kw):
        a = _geom_lib.BuffersArgs()
        a.B, a.H, a.W, a.KB, a.normalise, a.shade = 1, 4, 4, 1, 1, 0
        a.step, a.depth_scale, a.mask_threshold, a.edge = 1.0, 1.0, 0.5, 0.05
        a.disparity = a.mask = a.inv_intrinsics = a.depth = 64      # never dereferenced: every case below is refused
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw in (dict(H=0), dict(W=4097), dict(B=0), dict(B=2 ** 31 - 1, H=2), dict(B=128, H=4096, W=4096), dict(KB=2),
               dict(shade=3), dict(shade=-1), dict(disparity=None), dict(mask=None), dict(inv_intrinsics=None), dict(depth=None),
               dict(shade=2, image=64), dict(shade=2, image=64, near_depth=1.0, far_depth=1.0)):
        assert lib.enarf_geom_buffers(C.byref(args(**kw)), None) == -1, kw
        assert b"enarf_geom_buffers" in lib.enarf_geom_last_error()
    assert lib.enarf_geom_buffers(None, None) == -1
    for a in ((None, None, 64, 10, 0.5, 64, 1, 64, None), (64, None, None, 10, 0.5, 64, 1, 64, None),
              (64, None, 64, 0, 0.5, 64, 1, 64, None), (64, None, 64, 2 ** 31, 0.5, 64, 1024, 64, None),
              (64, None, 64, 10, 0.5, None, 1, 64, None), (64, None, 64, 10, 0.5, 64, 1, None, None),
              (64, None, 64, 4097, 0.5, 64, 2, 64, None)):
        assert lib.enarf_geom_err_update(*a) == -1, a


def test_eval_depth_tool_reads_its_ground_truth_and_builds_the_reference_batches(tmp_path):
    """tools/eval_depth.py without a device: --disparity-npy is taken as it is and checked against the cache's size; packed
    entries go through formats.unpack_image, whose ImportError (blosc is not a dependency) becomes the tool's message; the
    batches carry the reference loader's keys, cut at the end"""
    import pickle

    import libraries as L
    tool = L.tool("eval_depth")
    maps = np.random.default_rng(0).random((5, 8, 8)).astype(np.float32)
    np.save(tmp_path / "d.npy", maps)
    assert np.array_equal(tool.read_disparity(None, str(tmp_path / "d.npy"), 5), maps)
    with pytest.raises(SystemExit, match=r"expected \(4, S, S\)"):
        tool.read_disparity(None, str(tmp_path / "d.npy"), 4)
    with open(tmp_path / "cache.pickle", "wb") as f:
        pickle.dump({"disparity": [b"not a blosc frame"] * 5, "camera_intrinsic": np.zeros((5, 3, 3))}, f)
    try:
        import blosc  # noqa: F401
    except ImportError:
        with pytest.raises(SystemExit, match="--disparity-npy"):
            tool.read_disparity(str(tmp_path / "cache.pickle"), None, 5)
    with open(tmp_path / "poses.pickle", "wb") as f:
        pickle.dump({"camera_intrinsic": np.zeros((5, 3, 3))}, f)
    with pytest.raises(SystemExit, match="not a depth cache"):
        tool.read_disparity(str(tmp_path / "poses.pickle"), None, 5)
    poses, K, bone = np.zeros((5, 24, 4, 4)), np.ones((5, 3, 3)), np.ones((5, 23, 1))
    got = list(tool.batches(poses, K, bone, maps, np.array([4, 0, 2]), 2))
    assert [len(b["img"]) for b in got] == [2, 1] and set(got[0]) == {"pose_3d", "pose_3d_world", "bone_length", "intrinsics", "img"}
    assert torch.equal(got[0]["img"], torch.from_numpy(maps[[4, 0]])) and got[1]["pose_3d"].dtype == torch.float32
