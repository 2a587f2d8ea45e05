"""GPU tests of marching cubes (libenarf_mesh.so): exact agreement with the numpy restatement of the contract
(tests/mc_reference.py), surface checks, a 667^3 volume counted with torch, and the model-level extract_mesh."""
import numpy as np
import pytest
import torch

import mc_reference as M
from _helpers import Scene
from oracle import enarf_oracle as O

pytestmark = pytest.mark.gpu


def _mc(vol, iso):
    from enarf_gan_amd.libraries.NARF.mesh_rendering import marching_cubes
    v, t = marching_cubes(torch.as_tensor(vol).cuda(), iso)
    torch.cuda.synchronize()
    return v.cpu().numpy(), t.cpu().numpy()


def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2 for n in shape], indexing="ij")


def _closed(v):
    v = v.copy()
    v[0] = v[-1] = -1e3
    v[:, 0] = v[:, -1] = -1e3
    v[:, :, 0] = v[:, :, -1] = -1e3
    return v


def _volumes():
    rng = np.random.default_rng(7)
    x, y, z = _grid((33, 33, 33))
    sphere = (12.3 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
    x, y, z = _grid((48, 40, 36))
    torus = (5.5 - np.sqrt((np.sqrt(x * x + y * y) - 11.0) ** 2 + z * z)).astype(np.float32)
    x, y, z = _grid((65, 65, 65))
    gauss = sum(np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / 60.0) for c in rng.uniform(-18, 18, (6, 3)))
    gauss = gauss.astype(np.float32)
    noise = rng.standard_normal((17, 19, 23)).astype(np.float32)
    ties = rng.choice(np.array([0.5, 1.5, -0.5, np.nan], dtype=np.float32), size=(9, 10, 11), p=[0.4, 0.25, 0.25, 0.1])
    x, y, z = _grid((4, 4, 1500))
    longrow = (np.sin(z / 7.0) + 0.3 * x - 0.2 * y).astype(np.float32)
    return [
        ("sphere 33^3", sphere, 0.0),
        ("torus 48x40x36", torus, 0.0),
        ("gaussians 65^3", gauss, 0.35),
        ("white noise 17x19x23", noise, 0.1),
        ("values equal to iso and NaN", ties, 0.5),
        ("all inside", np.ones((5, 6, 7), np.float32), 0.0),
        ("all outside", -np.ones((5, 6, 7), np.float32), 0.0),
        ("2x2x2", np.array([1, -1, -1, 2, 0.5, -3, 4, -1], np.float32).reshape(2, 2, 2), 0.0),
        ("long rows 4x4x1500", longrow, 0.05),
    ]


def _assert_vertices_within_2ulp(got, ref, what):
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    tol = 2 * np.spacing(np.maximum(np.abs(ref), np.abs(got)).astype(np.float32))
    err = np.abs(got - ref)
    assert (err[~nan] <= tol[~nan]).all(), f"{what}: max vertex error {err[~nan].max()}"


def test_marching_cubes_matches_reference():
    for name, vol, iso in _volumes():
        rv, rt = M.marching_cubes(vol, iso)
        gv, gt = _mc(vol, iso)
        assert gv.dtype == np.float32 and gt.dtype == np.int64 and gv.shape[1:] == (3,) and gt.shape[1:] == (3,), name
        assert np.array_equal(gt, rt), f"{name}: triangles differ ({len(gt)} vs {len(rt)})"
        _assert_vertices_within_2ulp(gv, rv, name)
        if name.startswith("all"):
            assert gv.shape == (0, 3) and gt.shape == (0, 3)
        else:
            assert len(rt) > 0, name


def test_closed_surfaces_are_watertight_and_deterministic():
    rng = np.random.default_rng(3)
    vols = [_closed(rng.standard_normal((21, 18, 25)).astype(np.float32)), _volumes()[0][1], _volumes()[1][1]]
    for vol in vols:
        a = torch.from_numpy(vol).cuda()
        from enarf_gan_amd.libraries.NARF.mesh_rendering import marching_cubes
        v1, t1 = marching_cubes(a, 0.0)
        v2, t2 = marching_cubes(a, 0.0)
        assert torch.equal(v1, v2) and torch.equal(t1, t2)
        V, T = v1.cpu().numpy(), t1.cpu().numpy()
        assert len(T) > 0 and M.watertight_and_oriented(T) and M.signed_volume(V, T) > 0
    V, T = _mc(vols[1], 0.0)
    assert M.euler_characteristic(V, T) == 2
    V, T = _mc(vols[2], 0.0)
    assert M.euler_characteristic(V, T) == 0


def test_667_cube_counts_match_torch():
    from enarf_gan_amd.libraries.NARF.mesh_rendering import marching_cubes
    n = 667
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    vol = 200.0 - torch.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2)
    vol += torch.randn(n, n, n, device="cuda", generator=g) * 0.8
    verts, tris = marching_cubes(vol, 0.0)
    ins = vol > 0
    V = int((ins[1:] != ins[:-1]).sum()) + int((ins[:, 1:] != ins[:, :-1]).sum()) + int((ins[:, :, 1:] != ins[:, :, :-1]).sum())
    ntri, _ = M.load_table()
    case = torch.zeros(n - 1, n - 1, n - 1, dtype=torch.uint8, device="cuda")
    for b in range(8):
        dx, dy, dz = b & 1, (b >> 1) & 1, (b >> 2) & 1
        case |= ins[dx:n - 1 + dx, dy:n - 1 + dy, dz:n - 1 + dz].to(torch.uint8) << b
    T = int(torch.from_numpy(ntri).cuda()[case.long()].sum())
    del case, ins
    assert verts.shape == (V, 3) and tris.shape == (T, 3) and V > 10 ** 6
    assert int(tris.min()) >= 0 and int(tris.max()) < V
    assert bool(torch.isfinite(verts).all())
    assert float(verts.min()) >= 0 and float(verts.max()) <= n - 1


def _model(sc):
    from test_gpu_api import _model as make
    return make(sc)


def test_extract_mesh_matches_density_volume_and_the_oracle_grid():
    """TriNARFGenerator.extract_mesh == marching_cubes(density_volume(...)) with the reference's transform; and on the
    scene of test_density_volume_matches_oracle_grid_sweep, TriPlaneNARF's mesh matches mc_reference on the oracle's
    density grid."""
    from enarf_gan_amd.libraries.NARF.mesh_rendering import density_volume, extract_mesh, marching_cubes
    from enarf_gan_amd.models.generator import TriNARFGenerator
    from test_host_cpu import Cfg, _nerf_cfg
    sc = Scene(32, 1, "center_fixed", 20)
    s = sc.raw
    m = _model(sc)
    voxel = 0.125
    center = torch.tensor([0.02, -0.03, 1.0]).reshape(1, 3, 1)
    center[0, :, 0] += sc.pose_parts[0, :, :3, 3].mean(0) - torch.tensor([0.0, 0.0, 1.0])
    mi = {"z": None, "z_rend": s["z_rend"].cuda(), "bone_length": sc.bl_parts.cuda(), "truncation_psi": 1}
    pose = sc.pose_parts.cuda()
    cube = int(1 / voxel)
    bins = torch.arange(-cube, cube + 1) / cube
    p = (torch.stack(torch.meshgrid(bins, bins, bins, indexing="ij")).reshape(1, 3, -1) + center) * 3.0
    den, _, _ = O.query(p, sc.pose_scaled, sc.scale, sc.cpose, s["tri_plane"], sc.weights())
    ref = den.reshape(2 * cube + 1, 2 * cube + 1, 2 * cube + 1).numpy().astype(np.float32)
    # a threshold no density comes within 1e-3 of, with a surface to find
    cands = [th for th in np.linspace(0.05, 0.95, 19) * float(ref.max())
             if np.abs(ref - th).min() > 1e-3 and (ref > th).sum() > 20]
    assert cands
    th = float(cands[len(cands) // 2])
    verts, tris = extract_mesh(m, pose, center, voxel, th, mi)
    rv, rt = M.marching_cubes(ref, th)
    assert np.array_equal(tris.cpu().numpy(), rt) and len(rt) > 0
    rv_t = (torch.from_numpy(rv) - cube) * voxel + center[:, :, 0]
    err = float((verts.cpu() - rv_t).abs().max())
    assert err < 0.05 * voxel, f"vertex error {err} (scene units)"
    # the same mesh through the generator, one sample (z = [tri-plane 512 | renderer 256], as the GAN forward test)
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
    vol = gen.density_volume(one(s["pose_to_camera"]), z, one(s["bone_length"]), voxel_size=voxel)
    th = float(vol.max()) * 0.4
    gv, gt = gen.extract_mesh(one(s["pose_to_camera"]), z, one(s["bone_length"]), voxel_size=voxel, mesh_th=th)
    ev, et = marching_cubes(vol, th)
    c = one(s["pose_to_camera"])[:, 0, :3, 3:]
    assert len(et) > 0 and torch.equal(gt, et)
    assert torch.equal(gv, (ev - cube) * voxel + c[:, :, 0])
    with pytest.raises(AssertionError):          # one sample at a time, as create_mesh
        gen.extract_mesh(s["pose_to_camera"].cuda(), z.expand(2, -1), s["bone_length"].cuda(), voxel_size=voxel)
