"""GPU tests of the mesh simplification (libenarf_simp.so): simp_key_kernel, simp_corner_kernel and both instantiations of
simp_place_kernel, through ops.simplify_mesh, against the float64 numpy restatement of the contract (tests/simp_reference.py)
on the hand meshes of tests/simp_cases.py (one per edge case of the contract) and on the 33^3 sphere at cells of 2, 3, 4 and 6
voxels (short segments up to vertex segments of 72 and incidence segments of several wavefronts, no multiple of 64);
determinism, the empty mesh, a custom origin, the search for a triangle count, and the model-level entry points.

vertex_cluster, cluster_size and the triangles are integers and must be equal. A coordinate is the referee's rounded to
fp32, or one fp32 step from it: the kernel folds 64 partial sums where the referee adds one after the other, a difference of
about 1e-16 relative in A, b and the mean, about 1e-13 after a solve of condition number <= 1001, which can move the
rounding to fp32 only where the exact value lies that near a tie."""
import json
import struct

import numpy as np
import pytest
import torch

import paint_cases as PC
import simp_cases as SC
import simp_reference as SR
from test_gpu_paint import _dev, _model

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _simplify(v, t, h, **kw):
    from enarf_gan_amd import ops
    out = ops.simplify_mesh(_dev(v), _dev(t), h, **kw)
    torch.cuda.synchronize()
    assert out._fields == ("vertices", "triangles", "vertex_cluster", "cluster_size")
    assert (out.vertices.dtype, out.triangles.dtype, out.vertex_cluster.dtype, out.cluster_size.dtype) == \
        (torch.float32, torch.int64, torch.int32, torch.int32)
    assert all(x.is_cuda and x.is_contiguous() for x in out)
    return out


def _compare(got, ref, what):
    C = len(ref.cluster_size)
    assert got.vertices.shape == (C, 3) and got.triangles.shape == ref.triangles.shape, what
    assert np.array_equal(_np(got.vertex_cluster), ref.vertex_cluster), what
    assert np.array_equal(_np(got.cluster_size), ref.cluster_size), what
    assert np.array_equal(_np(got.triangles), ref.triangles), what
    gv = _np(got.vertices)
    print(f"{what}: {C} clusters, {len(ref.triangles)} triangles, {(gv != ref.vertices).sum()} of {gv.size} coordinates one step off")
    assert SR.one_step_of(gv, ref.vertices), what


# ------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("case", SC.ALL)
def test_every_case_matches_the_referee(case, placement):
    if case in SC.HAND:
        v, t, h, o = SC.mesh(case)
    else:
        (v, t), h, o = PC.sphere(), SC.sphere_cell(case), None
    ref = SC.referee(case, placement)
    if case == "wedge" and placement == "quadric":
        assert ref.info["clamped"].tolist() == [True, False]                   # the clamp acts
    if case in SC.SPHERE_TABLE:
        assert (len(ref.vertices), len(ref.triangles), int(ref.cluster_size.max())) == SC.SPHERE_TABLE[case]
    _compare(_simplify(v, t, h, origin=o, placement=placement), ref, f"{case} {placement}")


def test_two_calls_are_bit_identical_and_an_empty_mesh_is_empty():
    v, t = PC.sphere()
    for placement in ("quadric", "mean"):
        a, b = (_simplify(v, t, SC.sphere_cell(6), placement=placement) for _ in range(2))
        for x, y in zip(a, b):
            assert x.shape == y.shape and _np(x).tobytes() == _np(y).tobytes()
        for V, T in ((0, 0), (0, 2)):                                          # no vertex: the triangles name none
            e = _simplify(np.zeros((V, 3), np.float32), np.zeros((T, 3), np.int64), 0.1, placement=placement)
            assert (e.vertices.shape, e.triangles.shape, e.vertex_cluster.shape, e.cluster_size.shape) == ((0, 3), (0, 3), (0,), (0,))
        # vertices and no triangle: every cluster at its mean, nothing to connect
        cloud = _simplify(v, np.zeros((0, 3), np.int64), SC.sphere_cell(6), placement=placement)
        _compare(cloud, SR.simplify(v, np.zeros((0, 3), np.int64), SC.sphere_cell(6), placement=placement), f"cloud {placement}")
        assert cloud.triangles.shape == (0, 3)
        assert _np(cloud.vertices).tobytes() == _np(_simplify(v, t, SC.sphere_cell(6), placement="mean").vertices).tobytes()


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_an_origin_below_the_minimum_shifts_the_cells_as_the_referee_says(placement):
    v, t = PC.sphere()
    h = SC.sphere_cell(3)
    o = v.min(0) - np.float32(0.4 * h)
    ref = SR.simplify(v, t, h, origin=o, placement=placement)
    assert not np.array_equal(ref.vertex_cluster, SC.referee(3, placement).vertex_cluster)
    _compare(_simplify(v, t, h, origin=tuple(float(x) for x in o), placement=placement), ref, f"origin {placement}")
    _compare(_simplify(v, t, h, origin=torch.from_numpy(o), placement=placement), ref, f"origin tensor {placement}")
    with pytest.raises(ValueError, match="above"):
        _simplify(v, t, h, origin=tuple(float(x) for x in v.min(0) + np.float32(1e-3)))
    bad = v.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        _simplify(bad, t, h)


def test_a_target_triangle_count_is_met_and_one_step_finer_exceeds_it():
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF import mesh_rendering as MR
    v, t = PC.sphere()
    dv, dt = _dev(v), _dev(t)
    target = 500
    best, steps = MR.simplify_steps(dv, dt, target)
    got = MR.simplify_mesh(dv, dt, target_triangles=target)
    assert len(steps) <= 12 and steps[0][1] == 0                               # run 1: the diagonal, one cluster
    assert np.isclose(steps[0][0], 1.0001 * np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)), rtol=1e-6)
    within = [(h, n) for h, n in steps if n <= target]
    over = [(h, n) for h, n in steps if n > target]
    cell = min(h for h, _ in within)
    print(f"target {target}: {len(steps)} runs, cell {cell:.5f} with {got.triangles.shape[0]} triangles; next finer "
          f"{max(h for h, _ in over):.5f} with {[n for h, n in over if h == max(x for x, _ in over)][0]}")
    assert 0 < got.triangles.shape[0] <= target
    want = ops.simplify_mesh(dv, dt, cell)
    for x, y, z in zip(got, want, best):
        assert torch.equal(x, y) and torch.equal(x, z)
    # one bisection step finer exceeds the target: the nearest finer cell that was tried, and every finer one
    assert over and max(h for h, _ in over) < cell and all(h < cell for h, _ in over)
    assert MR.simplify_mesh(dv, dt, cell=cell).triangles.shape[0] == got.triangles.shape[0]
    assert MR.simplify_mesh(dv, dt, target_triangles=0).triangles.shape[0] == 0
    assert torch.equal(MR.simplify_mesh(dv, dt, target_triangles=len(t), max_runs=12).triangles,
                       MR.simplify_steps(dv, dt, len(t))[0].triangles)
    with pytest.raises(ValueError, match="exactly one"):
        MR.simplify_mesh(dv, dt)


# ------------------------------------------------------------------------------------------------- the model's entry points
def _pieces():
    gen, s, z, pose, bl, K, mesh = _model()
    z_nerf, z_render, _ = gen._latent_parts(z)
    _, pose_parts, model_input = gen.nerf._mesh_inputs(pose, z_nerf, z_render, bl, 0.4)
    return gen, pose_parts, model_input, 2 * mesh["voxel_size"]


def test_extract_mesh_with_simplify_cell_is_simplify_mesh_of_extract_mesh():
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import point_part_labels, vertex_colors
    gen, s, z, pose, bl, K, mesh = _model()
    _, pose_parts, model_input, h = _pieces()
    fv, ft = gen.extract_mesh(pose, z, bl, **mesh)
    nv, nt = gen.extract_mesh(pose, z, bl, **mesh, simplify_cell=None)
    assert torch.equal(nv, fv) and torch.equal(nt, ft)
    want = ops.simplify_mesh(fv, ft, h)
    sv, st, labels, colors = gen.extract_mesh(pose, z, bl, **mesh, simplify_cell=h, return_part_labels=True, return_colors=True)
    print(f"model mesh: {len(fv)} vertices, {len(ft)} triangles -> {len(sv)}, {len(st)} at a cell of {h}")
    assert torch.equal(sv, want.vertices) and torch.equal(st, want.triangles)
    assert 0 < len(st) < len(ft) // 2 and len(sv) == want.cluster_size.shape[0] and int(want.cluster_size.sum()) == len(fv)
    assert int(st.min()) >= 0 and int(st.max()) < len(sv)
    # the referee on the very mesh the kernels read
    _compare(want, SR.simplify(_np(fv), _np(ft), h), "model mesh")
    # labels and colours are those of the new vertices, from the calls that exist
    assert torch.equal(labels, point_part_labels(gen.nerf, pose_parts, sv, model_input, points_last=True)[0][0])
    assert torch.equal(colors, vertex_colors(gen.nerf, pose_parts, sv, model_input))
    assert labels.shape == (len(sv),) and colors.shape == (len(sv), 3) and float(colors.std()) > 0.01
    pv, pt = gen.extract_mesh(pose, z, bl, **mesh, simplify_cell=h)
    assert torch.equal(pv, sv) and torch.equal(pt, st)


def _cells_needed(T):
    n = 1
    while 2 * n * n < T:
        n += 1
    return n


def _glb_document(path):
    raw = open(path, "rb").read()
    magic, version, length = struct.unpack_from("<4sII", raw, 0)
    assert magic == b"glTF" and version == 2 and length == len(raw)
    n_json, kind = struct.unpack_from("<I4s", raw, 12)
    assert kind == b"JSON"
    return json.loads(raw[20:20 + n_json].decode("utf-8"))


def test_a_simplified_rig_is_made_of_its_own_pieces_and_round_trips_through_glb(tmp_path):
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import _mask_tri_plane, export_glb
    from enarf_gan_amd.libraries.NeRF.rendering import _parts_from_part_poses
    gen, s, z, pose, bl, K, mesh = _model()
    _, pose_parts, model_input, h = _pieces()
    fv, ft = gen.extract_mesh(pose, z, bl, **mesh)
    sv, st = gen.extract_mesh(pose, z, bl, **mesh, simplify_cell=h)
    # an atlas the layout refuses for the fine mesh and accepts for the simplified one
    A = 6 * _cells_needed(len(ft)) - 1
    assert A >= 6 * _cells_needed(len(st))
    with pytest.raises(NotImplementedError):
        ops.bake_layout(len(ft), A)
    with pytest.raises(NotImplementedError):
        gen.extract_rigged_mesh(pose, z, bl, **mesh, texture_size=A)
    rig = gen.extract_rigged_mesh(pose, z, bl, **mesh, simplify_cell=h, texture_size=A, return_colors=True)
    assert torch.equal(rig.vertices, sv) and torch.equal(rig.triangles, st)
    nerf = gen.nerf
    flags = nerf.kernel_flags()
    parts = _parts_from_part_poses(nerf, pose_parts, model_input["bone_length"])
    joints, weights, kept = ops.skin_weights(sv, parts, nerf.canonical_pose, _mask_tri_plane(nerf, model_input), max_influences=4,
                                             clamp_mask=flags["clamp_mask"], uniform_part_weight=flags["uniform_part_weight"],
                                             coordinate_scale=float(nerf.coordinate_scale))
    assert torch.equal(rig.joints, joints) and torch.equal(rig.weights, weights) and torch.equal(rig.kept_mass, kept)
    assert rig.joints.shape == (len(sv), 4)
    atlas = gen.bake_texture(pose, z, bl, sv, st, size=A)
    assert (rig.texture.num_triangles, rig.texture.size) == (len(st), A) and rig.texture.cell == ops.bake_layout(len(st), A).cell
    assert torch.equal(rig.texture.texture, atlas.texture) and int((atlas.texture[..., 3] == 255).sum()) > 1000
    assert rig.colors.shape == (len(sv), 3)
    # the smaller rig goes through skin_mesh and export_glb as it is
    from enarf_gan_amd.libraries.NARF.mesh_rendering import skin_mesh
    posed = skin_mesh(nerf, rig, rig.rest_pose, rig.rest_bone_length)
    assert posed.shape == (1, len(sv), 3) and float((posed[0] - sv).abs().max()) < 1e-6      # the rest pose gives the mesh back
    path = str(tmp_path / "small.glb")
    export_glb(rig, path)
    doc = _glb_document(path)
    prim = doc["meshes"][0]["primitives"][0]
    att = prim["attributes"]
    assert doc["accessors"][prim["indices"]]["count"] == 3 * len(st)
    for name in ("POSITION", "TEXCOORD_0", "JOINTS_0", "WEIGHTS_0"):           # de-indexed for the atlas: a vertex a corner
        assert doc["accessors"][att[name]]["count"] == 3 * len(st), name
    plain = gen.extract_rigged_mesh(pose, z, bl, **mesh, simplify_cell=h)
    export_glb(plain, path)
    doc = _glb_document(path)
    prim = doc["meshes"][0]["primitives"][0]
    assert doc["accessors"][prim["attributes"]["POSITION"]]["count"] == len(sv)
    assert doc["accessors"][prim["indices"]]["count"] == 3 * len(st)
