"""GPU tests of the mesh rasteriser (libenarf_raster.so): agreement with the float64 numpy restatement of the contract
(tests/raster_reference.py) on hand-placed triangles and on marching-cubes meshes, determinism, the empty mesh, and the
model-level render_extracted_mesh."""
import numpy as np
import pytest
import torch

import mc_reference as M
import raster_reference as RR
from _helpers import Scene

pytestmark = pytest.mark.gpu

# (R, img_size, fx, fy, cx, cy): fx != fy, an off-centre principal point, img_size != R
CAMERAS = {64: (64, 96, 110.0, 90.0, 52.0, 41.0), 257: (257, 128, 150.0, 130.0, 70.0, 58.0),
           512: (512, 160, 190.0, 170.0, 83.0, 75.0)}


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def _raster(verts, tris, K, img_size, R):
    from enarf_gan_amd.libraries.NARF.mesh_rendering import rasterize_mesh
    out = rasterize_mesh(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).cuda(),
                         torch.from_numpy(np.ascontiguousarray(tris, np.int64)).reshape(-1, 3).cuda(),
                         torch.from_numpy(K).reshape(1, 3, 3).cuda(), img_size, R)
    torch.cuda.synchronize()
    return out


def _numpy(out):
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


def _check(got, ref, what):
    amb = ref["ambiguous"]
    ok = ~amb
    assert amb.mean() < 0.05, f"{what}: {amb.mean():.3f} of the pixels are ambiguous"
    R = ok.shape[0]
    assert got["image"].shape == (R, R, 3) and got["image"].dtype == np.uint8, what
    assert np.array_equal(got["pix_to_face"][ok], ref["pix_to_face"][ok]), \
        f"{what}: pix_to_face differs on {(got['pix_to_face'] != ref['pix_to_face'])[ok].sum()} unambiguous pixels"
    cov = ok & (ref["pix_to_face"] >= 0)
    bg = ok & (ref["pix_to_face"] < 0)
    assert cov.sum() > 0, what
    assert np.allclose(got["zbuf"][cov], ref["zbuf"][cov], rtol=1e-5, atol=0), what
    assert np.allclose(got["bary"][cov], ref["bary"][cov], rtol=1e-5, atol=1e-5), what
    assert np.abs(got["normals"][cov] - ref["normals"][cov]).max() <= 1e-4, what
    assert (got["zbuf"][bg] == -1).all() and (got["bary"][bg] == -1).all() and (got["normals"][bg] == 0).all(), what
    d = np.abs(got["image"].astype(np.int16) - ref["image"].astype(np.int16))[ok]
    assert d.max() <= 1, f"{what}: image differs by {d.max()} levels"
    assert (d == 0).all(-1).mean() >= 0.999, what
    assert (got["image"][..., 0] == got["image"][..., 1]).all() and (got["image"][..., 0] == got["image"][..., 2]).all()


def _check_deterministic(a, b, verts, tris, K, img_size, R, what):
    """two calls bit-identical; zbuf is exactly the fp32 depth the key was built from (1 / sum(b_i / z_i) rounded)"""
    for k in a._fields:
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs between two calls"
    p2f = a.pix_to_face.cpu().numpy()
    zb = a.zbuf.cpu().numpy()
    ref = RR.rasterize(verts, tris, K, img_size, R)
    sel = (p2f >= 0) & (p2f == ref["pix_to_face"]) & ~ref["ambiguous"]
    # fp64 all the way to the rounding: within one fp32 rounding of the float64 restatement
    assert (np.abs(zb[sel].astype(np.float64) - ref["zbuf"][sel]) <= np.spacing(zb[sel]).astype(np.float64)).all(), what


def _hand_mesh():
    rng = np.random.default_rng(11)
    verts, tris = [], []

    def add(pts):
        b = len(verts)
        verts.extend(np.asarray(pts, np.float64).tolist())
        tris.append([b, b + 1, b + 2])
        return b

    for _ in range(40):                                                 # overlapping, interpenetrating
        c = rng.uniform([-0.8, -0.8, 2.0], [0.8, 0.8, 5.0])
        add(c + rng.normal(0, 0.3, (3, 3)) * [1, 1, 0.4])
    tris.append(list(tris[3]))                                          # the same triangle twice: an exact tie
    add([verts[i] for i in tris[5]])                                    # a copy with vertices of its own
    add([[-3.0, 0.0, 2.0], [0.3, 0.2, 2.5], [-3.0, 1.0, 3.0]])         # partly off-screen
    add([[0.0, 0.0, 2.0], [0.5, 0.0, -1.0], [0.0, 0.5, 2.0]])          # a vertex behind the camera
    add([[0.1, 0.1, 1.5], [0.1, 0.1, 1.5], [0.3, 0.2, 1.5]])           # zero area (two equal vertices)
    b = add([[0.2, -0.1, 1.8], [0.5, -0.3, 1.9], [0.4, 0.1, 1.7]])
    tris.append([b, b, b + 1])                                          # zero area (a repeated index)
    tris.append([0, 1, len(verts) + 7])                                 # an index outside [0, V): not drawn
    add([[-30.0, -30.0, 7.0], [30.0, -30.0, 7.0], [0.0, 40.0, 7.5]])   # larger than the screen, behind the rest
    return np.array(verts, np.float32), np.array(tris, np.int64)


@pytest.mark.parametrize("R", sorted(CAMERAS))
def test_hand_placed_triangles_match_reference(R):
    _, img, fx, fy, cx, cy = CAMERAS[R]
    K = _K(fx, fy, cx, cy)
    verts, tris = _hand_mesh()
    a = _raster(verts, tris, K, img, R)
    b = _raster(verts, tris, K, img, R)
    got = _numpy(a)
    ref = RR.rasterize(verts, tris, K, img, R)
    _check(got, ref, f"hand-placed R={R}")
    p2f = got["pix_to_face"]
    assert len(tris) == 49 and (p2f == 48).mean() > 0.1              # the screen-filling triangle shows round the rest
    assert not np.isin(p2f, [40, 41]).any()                          # exact ties with 3 and 5: the smaller id wins
    assert not np.isin(p2f, [43, 44, 46, 47]).any()                  # not drawn
    _check_deterministic(a, b, verts, tris, K, img, R, f"hand-placed R={R}")


def test_screen_filling_triangles_match_reference():
    """triangles far larger than the screen only, wound both ways, two of them crossing in depth"""
    R, img, fx, fy, cx, cy = CAMERAS[257]
    K = _K(fx, fy, cx, cy)
    verts = np.array([[-40, -40, 3], [40, -40, 5], [0, 50, 4], [-40, 45, 4.5], [0, -50, 3.5], [45, 45, 4.2]], np.float32)
    tris = np.array([[0, 1, 2], [3, 5, 4]])
    a = _raster(verts, tris, K, img, R)
    got = _numpy(a)
    ref = RR.rasterize(verts, tris, K, img, R)
    _check(got, ref, "screen-filling")
    assert set(np.unique(got["pix_to_face"])) == {0, 1}
    _check_deterministic(a, _raster(verts, tris, K, img, R), verts, tris, K, img, R, "screen-filling")


def _mc_mesh(kind):
    from enarf_gan_amd.libraries.NARF.mesh_rendering import marching_cubes
    if kind == "sphere":
        n = 65
        x = np.arange(n, dtype=np.float64) - (n - 1) / 2
        g = np.meshgrid(x, x, x, indexing="ij")
        vol, scale, centre = 30.3 - np.sqrt(sum(a * a for a in g)), 0.8 / 30.3, [0.05, -0.03, 3.0]
        rot = np.eye(3)
    else:
        xs, zs = np.arange(68, dtype=np.float64) - 33.5, np.arange(24, dtype=np.float64) - 11.5
        x, y, z = np.meshgrid(xs, xs, zs, indexing="ij")
        vol, scale, centre = 9.0 - np.sqrt((np.sqrt(x * x + y * y) - 22.0) ** 2 + z * z), 1.0 / 31.0, [-0.1, 0.05, 3.2]
        a = 0.9
        rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    shape = np.array(vol.shape)
    v, t = marching_cubes(torch.from_numpy(vol.astype(np.float32)).cuda(), 0.0)
    v = ((v.cpu().numpy() - (shape - 1) / 2) * scale) @ rot.T + centre
    return v.astype(np.float32), t.cpu().numpy()


@pytest.mark.parametrize("kind,R", [("sphere", 64), ("sphere", 257), ("torus", 512)])
def test_marching_cubes_meshes_match_reference(kind, R):
    _, img, fx, fy, cx, cy = CAMERAS[R]
    K = _K(fx, fy, cx, cy)
    verts, tris = _mc_mesh(kind)
    assert 10_000 <= len(tris) <= 50_000, len(tris)
    a = _raster(verts, tris, K, img, R)
    got = _numpy(a)
    ref = RR.rasterize(verts, tris, K, img, R)
    _check(got, ref, f"{kind} R={R}")
    cov = got["pix_to_face"] >= 0
    assert cov.mean() > 0.1 and (got["image"][cov][:, 0] > 127).mean() > 0.95    # wound outward: lit
    _check_deterministic(a, _raster(verts, tris, K, img, R), verts, tris, K, img, R, f"{kind} R={R}")


def test_empty_mesh_is_all_background():
    R, img, fx, fy, cx, cy = CAMERAS[64]
    K = _K(fx, fy, cx, cy)
    for verts, tris in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)),
                        (np.ones((5, 3), np.float32), np.zeros((0, 3), np.int64))):
        got = _numpy(_raster(verts, tris, K, img, R))
        assert (got["image"] == 255).all() and (got["pix_to_face"] == -1).all() and (got["zbuf"] == -1).all()
        assert (got["bary"] == -1).all() and (got["normals"] == 0).all()


def test_render_extracted_mesh_matches_rasterize_mesh():
    """TriNARFGenerator.render_extracted_mesh == rasterize_mesh(*extract_mesh(...), K, size) on the synthetic scene of
    test_gpu_mesh's generator case, at a coarse voxel"""
    from enarf_gan_amd.libraries.NARF.mesh_rendering import rasterize_mesh
    from enarf_gan_amd.models.generator import TriNARFGenerator
    from test_host_cpu import Cfg, _nerf_cfg
    sc = Scene(32, 1, "center_fixed", 256)
    s = sc.raw
    gen = TriNARFGenerator(Cfg(z_dim=256, background_ratio=0.7, crop_background=True, pretrained_background=False,
                               nerf_params=_nerf_cfg(constant_triplane=False)), 32, 24, s["parents"], 23, black_background=True)
    gen.register_canonical_pose(s["canonical_pose"])
    gen.nerf.load_state_dict({f"mlp.{k}": v for k, v in s["mlp"].items()}, strict=False)
    gen = gen.cuda().eval()
    tri_plane = s["tri_plane"][:1].cuda()
    gen.nerf.tri_plane_gen = lambda z_, enc, truncation_psi=1: tri_plane
    z = torch.cat([torch.randn(1, 512, generator=torch.Generator().manual_seed(0)), s["z_rend"][:1]], dim=1).cuda()
    one = lambda t: t[:1].cuda()
    voxel = 0.05
    vol = gen.density_volume(one(s["pose_to_camera"]), z, one(s["bone_length"]), voxel_size=voxel)
    th = float(vol.max()) * 0.4
    K = one(s["intrinsics"])
    img, (gv, gt) = gen.render_extracted_mesh(one(s["pose_to_camera"]), K, z, one(s["bone_length"]), voxel_size=voxel,
                                              mesh_th=th)
    ev, et = gen.extract_mesh(one(s["pose_to_camera"]), z, one(s["bone_length"]), voxel_size=voxel, mesh_th=th)
    assert torch.equal(gv, ev) and torch.equal(gt, et) and len(et) > 0
    assert isinstance(img, np.ndarray) and img.shape == (512, 512, 3) and img.dtype == np.uint8
    want = rasterize_mesh(ev, et, K, gen.size).image.cpu().numpy()
    assert np.array_equal(img, want)
    cov = rasterize_mesh(ev, et, K, gen.size).pix_to_face.cpu().numpy() >= 0
    assert cov.sum() > 1000
    assert (img[cov][:, 0] > 127).mean() >= 0.95      # marching cubes winds outward: the visible surface faces the light
    assert (img[~cov] == 255).all()
