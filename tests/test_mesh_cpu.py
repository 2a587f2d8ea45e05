"""CPU checks of marching cubes (libenarf_mesh.so, include/enarf_mesh.h): the generated case table and its rule, the
numpy restatement of the contract (tests/mc_reference.py) on closed fields, the library's exported ABI and kernel
inventory, and the host layer's refusals without a device."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import libraries as L
import mc_reference as M

ROOT = L.ROOT

# ------------------------------------------------------------------------------------------------- the table
def test_generator_reproduces_the_committed_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_table.py"), "--stdout"],
                       capture_output=True, text=True, check=True)
    assert r.stdout == open(M.TABLE_H).read(), "csrc/enarf_mc_table.h is not what tools/gen_mc_table.py generates"


def _edge_corners(e):
    (dx, dy, dz), a = M.edge_offsets()[e]
    c0 = dx + 2 * dy + 4 * dz
    return c0, c0 + (1 << a)


def test_every_case_uses_its_crossing_edges_in_closed_loops():
    ntri, tri = M.load_table()
    assert ntri.max() <= 5 and ntri[0] == 0 and ntri[255] == 0
    for case in range(256):
        ins = [(case >> c) & 1 for c in range(8)]
        crossing = {e for e in range(12) if ins[_edge_corners(e)[0]] != ins[_edge_corners(e)[1]]}
        t = tri[case, :3 * ntri[case]].reshape(-1, 3)
        assert (tri[case, 3 * ntri[case]:] == -1).all()
        assert set(t.reshape(-1).tolist()) == crossing, case
        # closed: every directed edge of the case's triangles is matched by its reverse or lies on a cube face
        # (a boundary segment, drawn once); the boundary segments form closed loops through every crossing edge
        d = [(int(a), int(b)) for x in t for a, b in ((x[0], x[1]), (x[1], x[2]), (x[2], x[0]))]
        boundary = [s for s in d if (s[1], s[0]) not in d]
        assert len(boundary) == len(crossing), case
        outs = sorted(a for a, _ in boundary)
        ins_ = sorted(b for _, b in boundary)
        assert outs == ins_ == sorted(crossing), case


def _faces():
    """6 faces: (corner ids, edge ids) with the corners fixed on one side of one axis"""
    out = []
    for a in range(3):
        for s in (0, 1):
            corners = [c for c in range(8) if (c >> a) & 1 == s]
            edges = [e for e in range(12) if set(_edge_corners(e)) <= set(corners)]
            out.append((corners, edges))
    return out


def _face_segments(ntri, tri, case, edges):
    """undirected boundary segments of the case's triangles that join two edges of one face"""
    t = tri[case, :3 * ntri[case]].reshape(-1, 3)
    d = [(int(a), int(b)) for x in t for a, b in ((x[0], x[1]), (x[1], x[2]), (x[2], x[0]))]
    return sorted(tuple(sorted(s)) for s in d if (s[1], s[0]) not in d and s[0] in edges and s[1] in edges)


def test_table_is_face_consistent():
    ntri, tri = M.load_table()
    for corners, edges in _faces():
        others = [c for c in range(8) if c not in corners]
        for bits in range(16):
            base = sum(((bits >> q) & 1) << c for q, c in enumerate(corners))
            segs = {tuple(_face_segments(ntri, tri, base | sum(((o >> q) & 1) << c for q, c in enumerate(others)), edges))
                    for o in range(16)}
            assert len(segs) == 1, (corners, bits, segs)


# ------------------------------------------------------------------------------------------------- the reference
def _closed(v):
    v = v.copy()
    v[0] = v[-1] = -1e3
    v[:, 0] = v[:, -1] = -1e3
    v[:, :, 0] = v[:, :, -1] = -1e3
    return v


def _grid(n):
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    return np.meshgrid(x, x, x, indexing="ij")


@pytest.mark.parametrize("seed", range(4))
def test_reference_on_random_closed_fields_is_watertight_and_oriented(seed):
    rng = np.random.default_rng(seed)
    noise = _closed(rng.standard_normal((11, 13, 12)).astype(np.float32))          # full of ambiguous faces
    smooth = _closed(sum(np.exp(-sum((g - c) ** 2 for g, c in zip(_grid(20), rng.uniform(-6, 6, 3))) / 12)
                         for _ in range(5)).astype(np.float32))
    for vol, iso in ((noise, 0.0), (noise, 0.7), (smooth, 0.3)):
        V, T = M.marching_cubes(vol, iso)
        assert len(T) > 0
        assert M.watertight_and_oriented(T)
        assert M.signed_volume(V, T) > 0


def test_reference_topology_and_volume():
    x, y, z = _grid(65)
    r = 25.0
    V, T = M.marching_cubes((r - np.sqrt(x * x + y * y + z * z)).astype(np.float32), 0.0)
    assert M.euler_characteristic(V, T) == 2
    assert abs(M.signed_volume(V, T) / (4 / 3 * math.pi * r ** 3) - 1) < 0.02
    tor = 6.0 - np.sqrt((np.sqrt(x * x + y * y) - 16.0) ** 2 + z * z)
    V, T = M.marching_cubes(tor.astype(np.float32), 0.0)
    assert M.euler_characteristic(V, T) == 0 and M.watertight_and_oriented(T) and M.signed_volume(V, T) > 0


# ------------------------------------------------------------------------------------------------- the library
def test_header_symbols_exported_and_bound():
    """what is specific to this library; tests/test_libraries_cpu.py holds the checks every library gets"""
    from enarf_gan_amd import _mesh_lib
    assert len(L.declared("mesh")) == 5
    assert _mesh_lib.ABI_VERSION == 1


def test_argument_checks_need_no_device():
    from enarf_gan_amd import _mesh_lib
    L.library("mesh")
    lib = _mesh_lib.load()
    assert lib.enarf_mesh_workspace_bytes(1, 5, 5) == 0
    assert lib.enarf_mesh_workspace_bytes(2048, 1024, 1024) == 0           # 2^31 points
    assert lib.enarf_mesh_workspace_bytes(667, 667, 667) < 16 * 667 * 667 + 4096   # O(X * Y)
    assert lib.enarf_mesh_count(None, 1, 5, 5, 0.0, None, None, None) == -1
    assert b">= 2" in lib.enarf_mesh_last_error()
    assert lib.enarf_mesh_count(None, 2048, 1024, 1024, 0.0, None, None, None) == -2
    assert lib.enarf_mesh_count(None, 4, 4, 4, 0.0, None, None, None) == -1          # null pointers
    assert lib.enarf_mesh_emit(None, 4, 1, 4, 0.0, None, None, None, None) == -1


def test_host_layer_has_no_cpu_fallback():
    from enarf_gan_amd._lib import EnarfHipError
    from enarf_gan_amd.libraries.NARF.mesh_rendering import extract_mesh, marching_cubes
    with pytest.raises(EnarfHipError):
        marching_cubes(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(EnarfHipError):
        extract_mesh(None, torch.zeros(1, 24, 4, 4), torch.zeros(1, 3, 1), 0.125, 15, {})


def test_export_obj_round_trips(tmp_path):
    from enarf_gan_amd.libraries.NARF.mesh_rendering import export_obj
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0 / 3.0]])
    tris = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int64)
    path = tmp_path / "tet.obj"
    export_obj(verts, tris, str(path))
    v, f = [], []
    for line in open(path):
        kind, *rest = line.split()
        (v if kind == "v" else f).append([float(x) for x in rest] if kind == "v" else [int(x) for x in rest])
    assert torch.equal(torch.tensor(v, dtype=torch.float32), verts)
    assert torch.equal(torch.tensor(f) - 1, tris)
    assert min(min(x) for x in f) == 1
