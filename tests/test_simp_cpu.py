"""CPU checks of the mesh simplification (libenarf_simp.so's host side and the referee of the GPU tests): no GPU. The
float64 referee (tests/simp_reference.py) against values worked out by hand on the hand meshes of tests/simp_cases.py and
against the properties the method is used for on the 33^3 sphere; every host check of _simp_lib.check_simplify_args; the
signatures that gained `simplify_cell`."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import libraries as L
import mc_reference as M
import paint_cases as PC
import simp_cases as SC
import simp_reference as SR
from enarf_gan_amd import _simp_lib as S


# ------------------------------------------------------------------------------------------------- the referee, by hand
@pytest.mark.parametrize("name", list(SC.HAND))
def test_the_referee_on_a_hand_mesh_gives_the_values_worked_out_by_hand(name):
    want = SC.HAND[name]
    for placement in ("quadric", "mean"):
        got = SC.referee(name, placement)
        assert got.vertex_cluster.dtype == np.int32 and got.vertex_cluster.tolist() == want["vertex_cluster"]
        assert got.cluster_size.dtype == np.int32 and got.cluster_size.tolist() == want["cluster_size"]
        assert got.triangles.dtype == np.int64 and got.triangles.shape[1:] == (3,)
        assert np.array_equal(got.triangles, want["out_triangles"])
        assert got.vertices.dtype == np.float32 and got.vertices.shape == (len(want["cluster_size"]), 3)
    # the hand values are exact up to the rounding of the fp32 inputs (0.1, 0.9, ... are not fp32 numbers)
    if "out_vertices" in want:
        np.testing.assert_allclose(SC.referee(name, "quadric").vertices, want["out_vertices"], rtol=0, atol=2e-6)
    mean = want.get("mean", want.get("out_vertices"))
    if mean is not None:
        np.testing.assert_allclose(SC.referee(name, "mean").vertices, mean, rtol=0, atol=2e-6)


def test_the_clamp_acts_on_the_wedge_and_nowhere_else_among_the_hand_meshes():
    want = SC.HAND["wedge"]
    got = SC.referee("wedge", "quadric")
    np.testing.assert_allclose(got.info["unclamped"], want["unclamped"], rtol=0, atol=2e-5)
    assert got.info["clamped"].tolist() == want["clamped"]
    assert got.info["unclamped"][0, 1] > 1.0 and got.vertices[0, 1] == np.float32(1.0)       # back on the cell's face y = 1
    assert np.nanmax(got.info["cond"]) <= 1 + 1 / 1e-3 + 1e-6
    for name in SC.HAND:
        if name != "wedge":
            assert not SC.referee(name, "quadric").info["clamped"].any(), name
    for name in ("unreferenced", "zero_area", "bad_indices"):                                 # clusters with trace(A) == 0
        assert (SC.referee(name, "quadric").info["trace"] == 0).any(), name
    assert (SC.referee("zero_area", "quadric").info["trace"] == 0).all()


def test_a_vertex_on_a_cell_face_belongs_to_the_upper_cell():
    v, _, h, o = SC.mesh("on_a_face")
    assert SR.cells_of(v, h, o)[:, 0].tolist() == [2, 1, 0]
    v, _, h, o = SC.mesh("on_a_face_h1")
    assert SR.cells_of(v, h, o)[:, 0].tolist() == [2, 1, 0, 0] and float(v[1, 0]) < 2.0


# ------------------------------------------------------------------------------------------------- the referee, on the sphere
@pytest.mark.parametrize("m", SC.SPHERE_CELLS)
def test_the_simplified_sphere_is_a_sphere(m):
    """watertight and oriented, Euler characteristic 2, every normal outward, and the quadric placement's volume deficit
    less than half the mean placement's (the mean pulls every vertex inside the surface it averages)"""
    v, t = PC.sphere()
    assert (len(v), len(t)) == (3846, 7688)
    centre, sphere = np.array([0.05, -0.03, 3.0]), 4.0 / 3.0 * np.pi * SC.SPHERE_RADIUS ** 3
    deficit = {}
    for placement in ("quadric", "mean"):
        got = SC.referee(m, placement)
        assert (len(got.vertices), len(got.triangles), int(got.cluster_size.max())) == SC.SPHERE_TABLE[m]
        assert int(got.cluster_size.sum()) == len(v) and int(got.cluster_size.min()) >= 1
        assert M.watertight_and_oriented(got.triangles)
        assert M.euler_characteristic(got.vertices, got.triangles) == 2
        p = got.vertices.astype(np.float64)[got.triangles]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert ((n * (p.mean(1) - centre)).sum(-1) > 0).all()
        assert (got.triangles[:, 0] < got.triangles[:, 1]).all() and (got.triangles[:, 0] < got.triangles[:, 2]).all()
        deficit[placement] = abs(1 - M.signed_volume(got.vertices, got.triangles) / sphere)
    cond = SC.referee(m, "quadric").info["cond"]
    print(f"cell {m} voxels: deficit quadric {deficit['quadric']:.4f}, mean {deficit['mean']:.4f}, ratio "
          f"{deficit['quadric'] / deficit['mean']:.3f}, max cond {np.nanmax(cond):.0f}")
    assert deficit["quadric"] < 0.5 * deficit["mean"]
    assert np.nanmax(cond) <= 1 + 1 / 1e-3 + 1e-6 and not np.isnan(cond).any()


def test_the_referee_with_an_origin_below_the_minimum_shifts_the_cells():
    v, t = PC.sphere()
    h = SC.sphere_cell(3)
    o = v.min(0) - np.float32(0.4 * h)
    a, b = SR.simplify(v, t, h), SR.simplify(v, t, h, origin=o)
    assert len(a.vertices) != len(b.vertices) or not np.array_equal(a.vertex_cluster, b.vertex_cluster)
    assert np.array_equal(SR.cells_of(v, h, o), np.floor((v.astype(np.float64) - o.astype(np.float64)) / h))
    assert M.watertight_and_oriented(b.triangles)


# ------------------------------------------------------------------------------------------------- the host checks
def _mesh():
    v, t, h, o = SC.mesh("three_cells")
    return torch.from_numpy(v.copy()), torch.from_numpy(t.copy()), h, o


def test_check_accepts_the_hand_meshes_without_a_device():
    for name in SC.HAND:
        v, t, h, o = SC.mesh(name)
        V, T, cell, origin = S.check_simplify_args(torch.from_numpy(v.copy()), torch.from_numpy(t.copy()), h, o)
        assert (V, T, cell, origin) == (len(v), len(t), float(np.float32(h)), tuple(float(x) for x in o))
    v, t, h, _ = _mesh()
    assert S.check_simplify_args(v, t, h)[3] == (0.5, 0.5, 0.5)                    # the default origin: the minimum
    assert S.check_simplify_args(v, t, 0.1)[2] == float(np.float32(0.1))           # the cell is taken as fp32
    assert S.check_simplify_args(v[:0], t[:0], h) == (0, 0, 1.0, None)             # an empty mesh needs no bounds


def test_check_rejects_shapes_and_dtypes():
    v, t, h, o = _mesh()
    for bad in (v.numpy(), v.double(), v.reshape(-1), v[:, :2], v[None]):
        with pytest.raises(ValueError):
            S.check_simplify_args(bad, t, h, o)
    for bad in (t.numpy(), t.int(), t.float(), t.reshape(-1), t[:, :2]):
        with pytest.raises(ValueError):
            S.check_simplify_args(v, bad, h, o)


def test_check_rejects_sizes_at_2_to_the_31():
    v, t, h, o = _mesh()
    big_v = torch.empty(2 ** 31, 3, dtype=torch.float32, device="meta")
    big_t = torch.empty((2 ** 31 + 2) // 3, 3, dtype=torch.int64, device="meta")
    ok_t = torch.empty((2 ** 31 - 1) // 3, 3, dtype=torch.int64, device="meta")
    bounds = ((0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="2\\^31"):
        S.check_simplify_args(big_v, t, h, o, bounds=bounds)
    with pytest.raises(ValueError, match="2\\^31"):
        S.check_simplify_args(v, big_t, h, o)
    assert S.check_simplify_args(torch.empty(2 ** 31 - 1, 3, dtype=torch.float32, device="meta"), ok_t, h, o, bounds=bounds)[:2] == \
        (2 ** 31 - 1, (2 ** 31 - 1) // 3)


def test_check_rejects_cells_origins_vertices_extents_and_placements():
    v, t, h, o = _mesh()
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, "wide", None):        # 1e-50 is 0 as fp32, 1e39 is inf
        with pytest.raises(ValueError):
            S.check_simplify_args(v, t, bad, o)
    for bad in ((0, 0), (0, 0, float("nan")), (0, 0, float("inf")), "abc", (0, 0, 0, 0)):
        with pytest.raises(ValueError):
            S.check_simplify_args(v, t, h, bad)
    for k in range(3):                                                                     # an origin above the minimum
        above = [0.5, 0.5, 0.5]
        above[k] = float(np.nextafter(np.float32(0.5), np.float32(1)))
        with pytest.raises(ValueError, match="above"):
            S.check_simplify_args(v, t, h, above)
    assert S.check_simplify_args(v, t, h, (0.5, 0.5, 0.5))[3] == (0.5, 0.5, 0.5)
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = v.clone()
        w[1, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            S.check_simplify_args(w, t, h)
    # an extent of 2^21 cells or more: the vertices span 1 on x from 0.5, so h = 2^-21 puts the last in cell 2^21 exactly
    with pytest.raises(NotImplementedError, match="2\\^21"):
        S.check_simplify_args(v, t, 2.0 ** -21)
    assert S.check_simplify_args(v, t, float(np.nextafter(np.float32(2.0 ** -21), np.float32(1))))[0] == 3
    for bad in ("median", "QUADRIC", None, 1):
        with pytest.raises(ValueError, match="placement"):
            S.check_simplify_args(v, t, h, o, placement=bad)
    for bad in (0.0, -1e-3, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="reg"):
            S.check_simplify_args(v, t, h, o, reg=bad)
    for placement in S.PLACEMENTS:
        assert S.check_simplify_args(v, t, h, o, placement=placement)[:2] == (3, 1)


def test_simplify_mesh_refuses_host_tensors_and_takes_exactly_one_of_cell_and_target():
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF import mesh_rendering as MR
    v, t, h, o = _mesh()
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.simplify_mesh(v, t, h)
    with pytest.raises(ValueError, match="exactly one"):
        MR.simplify_mesh(v, t)
    with pytest.raises(ValueError, match="exactly one"):
        MR.simplify_mesh(v, t, cell=h, target_triangles=10)
    assert S.SimplifiedMesh._fields == ("vertices", "triangles", "vertex_cluster", "cluster_size")


def test_the_argument_records_have_the_layout_of_the_header():
    """include/enarf_simp.h: 8-byte fields first or paired 4-byte fields, so no padding on either side"""
    assert (C.sizeof(S.KeysArgs), C.sizeof(S.CornersArgs), C.sizeof(S.PlaceArgs)) == (40, 56, 112)
    assert (S.KeysArgs.vertices.offset, S.CornersArgs.triangles.offset, S.PlaceArgs.reg.offset, S.PlaceArgs.vertices.offset) == \
        (24, 24, 40, 48)
    header = open(os.path.join(L.ROOT, "include", "enarf_simp.h")).read()
    assert f"#define ENARF_SIMP_AXIS_BITS   {S.AXIS_BITS}" in header and "0x7FFFFFFF" in header and S.NO_CLUSTER == 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------- the signatures
# every parameter and default the entry points had before `simplify_cell`, in order; simplify_cell = None comes last
_BEFORE = {
    "mesh_rendering.extract_mesh": [("model",), ("pose_to_camera",), ("center",), ("voxel_size", 0.003), ("mesh_th", 15),
                                    ("model_input", {}), ("return_part_labels", False), ("return_colors", False)],
    "mesh_rendering.extract_rigged_mesh": [("model",), ("pose_to_camera",), ("center",), ("voxel_size", 0.003), ("mesh_th", 15),
                                           ("model_input", {}), ("max_influences", 4), ("return_colors", False),
                                           ("return_part_labels", False), ("texture_size", None), ("texture_color", "field")],
    "TriPlaneNARF.extract_mesh": [("self",), ("pose_to_camera",), ("z",), ("z_rend",), ("bone_length",), ("voxel_size", 0.003),
                                  ("mesh_th", 15), ("truncation_psi", 0.4), ("return_part_labels", False), ("return_colors", False)],
    "TriPlaneNARF.extract_rigged_mesh": [("self",), ("pose_to_camera",), ("z",), ("z_rend",), ("bone_length",),
                                         ("voxel_size", 0.003), ("mesh_th", 15), ("truncation_psi", 0.4), ("max_influences", 4),
                                         ("return_colors", False), ("return_part_labels", False), ("texture_size", None),
                                         ("texture_color", "field")],
    "TriPlaneNARF.render_textured_mesh": [("self",), ("pose_to_camera",), ("intrinsics",), ("z",), ("z_rend",), ("bone_length",),
                                          ("voxel_size", 0.01), ("mesh_th", 15), ("truncation_psi", 0.4), ("img_size", 128),
                                          ("texture_size", 1024), ("color", "field"), ("lit", True)],
    "TriNARFGenerator.extract_mesh": [("self",), ("pose_to_camera",), ("z",), ("bone_length",), ("voxel_size", 0.003),
                                      ("mesh_th", 15), ("truncation_psi", 0.4), ("return_part_labels", False),
                                      ("return_colors", False)],
    "TriNARFGenerator.extract_rigged_mesh": [("self",), ("pose_to_camera",), ("z",), ("bone_length",), ("voxel_size", 0.003),
                                             ("mesh_th", 15), ("truncation_psi", 0.4), ("max_influences", 4),
                                             ("return_colors", False), ("return_part_labels", False), ("texture_size", None),
                                             ("texture_color", "field")],
    "TriNARFGenerator.render_textured_mesh": [("self",), ("pose_to_camera",), ("intrinsics",), ("z",), ("bone_length",),
                                              ("voxel_size", 0.01), ("mesh_th", 15), ("truncation_psi", 0.4),
                                              ("texture_size", 1024), ("color", "field"), ("lit", True)],
}


@pytest.mark.parametrize("name", list(_BEFORE))
def test_simplify_cell_is_added_last_and_leaves_the_other_defaults_as_they_are(name):
    from enarf_gan_amd.libraries.NARF import mesh_rendering
    from enarf_gan_amd.models.generator import TriNARFGenerator
    from enarf_gan_amd.models.narf import TriPlaneNARF
    owner, attr = name.split(".")
    fn = getattr({"mesh_rendering": mesh_rendering, "TriPlaneNARF": TriPlaneNARF, "TriNARFGenerator": TriNARFGenerator}[owner], attr)
    fn = inspect.unwrap(fn)
    params = list(inspect.signature(fn).parameters.values())
    got = [(p.name,) if p.default is inspect.Parameter.empty else (p.name, p.default) for p in params]
    assert got == _BEFORE[name] + [("simplify_cell", None)]
