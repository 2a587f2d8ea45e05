"""CPU checks of the mesh rasteriser (libenarf_raster.so, include/enarf_raster.h): the numpy restatement of the contract
(tests/raster_reference.py) on hand-computed cases, the library's exported ABI and kernel inventory, and the host
layer's refusals without a device."""
import math
import os

import numpy as np
import pytest
import torch

import libraries as L
import mc_reference as M
import raster_reference as RR

ROOT = L.ROOT

# ------------------------------------------------------------------------------------------------- the reference
def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def test_one_triangle_covers_the_exact_pixel_set_top_left():
    # K's image is 32 px, output 16 px (s = 2); vertices at z = 1 project to (4.4, 4.4), (20.4, 4.4), (4.4, 20.4) of K's
    # image = (2.2, 2.2), (10.2, 2.2), (2.2, 10.2) output pixels: centres (c + 1/2, r + 1/2) with c, r >= 2, c + r <= 11
    verts = np.array([[4.4, 4.4, 1.0], [20.4, 4.4, 1.0], [4.4, 20.4, 1.0]], np.float32)
    for tri in ([0, 1, 2], [0, 2, 1]):                    # either winding
        out = RR.rasterize(verts, np.array([tri]), _K(1, 1, 0, 0), 32, 16)
        want = {(r, c) for r in range(16) for c in range(16) if r >= 2 and c >= 2 and r + c <= 11}
        got = {tuple(x) for x in np.argwhere(out["pix_to_face"] == 0)}
        assert got == want
        assert max(r for r, _ in got) < 8 + 4 and all(r < 8 or c < 8 for r, c in got)
        assert not out["ambiguous"].any()
        assert (out["pix_to_face"][out["pix_to_face"] != 0] == -1).all()
        cov = out["pix_to_face"] == 0
        assert np.allclose(out["zbuf"][cov], 1.0) and (out["zbuf"][~cov] == -1).all()
        assert np.allclose(out["bary"][cov].sum(-1), 1.0) and (out["bary"][~cov] == -1).all()
        assert (out["image"][~cov] == 255).all() and (out["normals"][~cov] == 0).all()
    # the top-left corner of K's image lands in rows and columns < R / 2 (no flip left in the output)
    corner = RR.rasterize(np.array([[1, 1, 1], [9, 1, 1], [1, 9, 1]], np.float32), np.array([[0, 1, 2]]),
                          _K(1, 1, 0, 0), 32, 32)
    rc = np.argwhere(corner["pix_to_face"] == 0)
    assert len(rc) and rc.max() < 16


def test_shading_facing_the_camera_is_255_and_facing_away_127():
    # R odd, the optical axis through the centre of pixel (7, 7); the triangle in the plane z = 2 faces the camera:
    # (v1 - v0) x (v2 - v0) = (0, 0, -16) for this winding
    verts = np.array([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]], np.float32)
    front = np.array([[0, 2, 1]])
    K = _K(10, 10, 7.5, 7.5)
    out = RR.rasterize(verts, front, K, 15, 15)
    assert out["pix_to_face"][7, 7] >= 0 and not out["ambiguous"][7, 7]
    assert np.allclose(out["normals"][7, 7], [0, 0, -1])
    assert (out["image"][7, 7] == 255).all()
    cov = out["pix_to_face"] >= 0
    assert (out["image"][cov] > 127).all()
    back = RR.rasterize(verts, front[:, ::-1], K, 15, 15)   # the same plane wound inward: N . L <= 0 everywhere
    cov = back["pix_to_face"] >= 0
    assert cov.sum() > 50 and (back["image"][cov] == 127).all()
    assert math.floor(0.5 * 255) == 127


def test_nearer_triangle_wins_and_ties_go_to_the_smaller_id():
    far = [[-3, -3, 4], [3, -3, 4], [-3, 3, 4]]
    near = [[-3, -3, 2], [3, -3, 2], [-3, 3, 2]]
    verts = np.array(far + near + near, np.float32)
    tris = np.array([[0, 1, 2], [5, 4, 3], [6, 7, 8], [3, 4, 5]])
    out = RR.rasterize(verts, tris, _K(8, 8, 8, 8), 16, 16)
    p = out["pix_to_face"]
    cov = (p >= 0) & ~out["ambiguous"]
    assert cov.sum() > 20
    assert set(np.unique(p[cov])) == {1}                    # 1, 2 and 3 tie exactly in front of 0: the smallest id
    assert np.allclose(out["zbuf"][cov], 2.0)


def test_reference_sphere_silhouette_is_the_analytic_disc():
    n, rad = 65, 30.3
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    g = np.meshgrid(x, x, x, indexing="ij")
    vol = (rad - np.sqrt(sum(a * a for a in g))).astype(np.float32)
    V, T = M.marching_cubes(vol, 0.0)
    rho, D, f, R = 0.5, 3.0, 300.0, 128
    verts = ((V - (n - 1) / 2) * (rho / rad) + np.array([0, 0, D])).astype(np.float32)
    out = RR.rasterize(verts, T, _K(f, f, R / 2, R / 2), R, R)
    disc = math.pi * (f * rho / math.sqrt(D * D - rho * rho)) ** 2
    covered = int((out["pix_to_face"] >= 0).sum())
    assert abs(covered / disc - 1) < 0.02, (covered, disc)
    # marching cubes winds outward: the visible surface faces the light
    cov = out["pix_to_face"] >= 0
    assert (out["image"][cov][:, 0] > 127).mean() > 0.95


# ------------------------------------------------------------------------------------------------- the library
def test_header_symbols_exported_and_bound():
    """what is specific to this library; tests/test_libraries_cpu.py holds the checks every library gets"""
    from enarf_gan_amd import _raster_lib
    assert L.declared("raster") == ["enarf_raster_abi_version", "enarf_raster_last_error", "enarf_raster_mesh",
                                    "enarf_raster_workspace_bytes"]
    assert _raster_lib.ABI_VERSION == 1


def test_sources_read_no_environment_and_hold_no_assembly():
    src = open(os.path.join(ROOT, "enarf-gan_amd", "csrc", "enarf_raster.hip")).read()
    assert "getenv" not in src and "asm" not in src


def test_argument_checks_need_no_device():
    from enarf_gan_amd import _raster_lib
    L.library("raster")
    lib = _raster_lib.load()
    ws = lib.enarf_raster_workspace_bytes
    assert ws(-1, 0, 512) == 0 and ws(0, -1, 512) == 0
    assert ws(1 << 31, 0, 512) == 0 and ws(0, 1 << 31, 512) == 0
    assert ws(10, 10, 0) == 0 and ws(10, 10, 4097) == 0
    assert ws(0, 0, 1) > 0 and ws(10, 10, 4096) >= 8 * 4096 * 4096
    # O(V + T + R^2)
    assert ws(8_418_232, 16_828_096, 512) <= 24 * 8_418_232 + 16 * 16_828_096 + (8 + 3 * 40) * 512 * 512 + 4096
    mesh = lib.enarf_raster_mesh
    args = lambda V=3, T=1, K=1, img=32, R=16, w=1, im=1: (1 if V else None, V, 1 if T else None, T, K, img, R, w, im,
                                                          None, None, None, None, None)
    assert mesh(*args(V=-1)) == -1
    assert b"[0, 2^31)" in lib.enarf_raster_last_error()
    assert mesh(*args(T=1 << 31)) == -1
    assert mesh(*args(R=0)) == -1 and b"render size 0" in lib.enarf_raster_last_error()
    assert mesh(*args(R=4097)) == -1
    assert mesh(*args(img=0)) == -1 and b"img_size" in lib.enarf_raster_last_error()
    assert mesh(*args(K=None)) == -1 and b"null" in lib.enarf_raster_last_error()
    assert mesh(*args(w=None)) == -1
    assert mesh(*args(im=None)) == -1
    assert mesh(None, 3, 1, 1, 1, 32, 16, 1, 1, None, None, None, None, None) == -1     # vertices null with V > 0
    assert mesh(1, 3, None, 1, 1, 32, 16, 1, 1, None, None, None, None, None) == -1     # triangles null with T > 0


def test_host_layer_has_no_cpu_fallback():
    from enarf_gan_amd._lib import EnarfHipError
    from enarf_gan_amd.libraries.NARF.mesh_rendering import rasterize_mesh
    verts = torch.zeros(3, 3)
    tris = torch.tensor([[0, 1, 2]])
    with pytest.raises(EnarfHipError):
        rasterize_mesh(verts, tris, torch.eye(3), 32, 16)
    with pytest.raises(EnarfHipError):
        rasterize_mesh(verts.numpy(), tris, torch.eye(3), 32)
