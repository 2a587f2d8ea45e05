"""CPU checks of the part segmentation (libenarf_seg.so's host side, the palette, the referee of the GPU tests): no GPU.
The library checks of the `seg` row (header against exports and SIGNATURES, ABI version, kernel inventory against
tests/seg_kernel_coverage.py, tracked headers, disjoint kernels) are tests/test_side_libraries_cpu.py's."""
import math

import numpy as np
import pytest
import torch

import seg_reference as R
from _helpers import Scene
from enarf_gan_amd import ops
from enarf_gan_amd._loader import EnarfHipError
from enarf_gan_amd.libraries.NeRF.rendering import render, semantic_palette


# ------------------------------------------------------------------------------------------------------------- palette
def test_palette_literals_and_distinct_entries():
    p23, p24 = semantic_palette(23), semantic_palette(24)
    assert p23.shape == (23, 3) and p24.shape == (24, 3) and p23.dtype == torch.float32
    assert p23[[0, 1, 2, 22]].tolist() == [[1, 0, 0], [-1, -1, 0], [1, -1, 1], [-1, -1, -1]]
    assert p24[23].tolist() == [1, 0, 1]
    for p in (p23, p24):
        assert len({tuple(r) for r in p.tolist()}) == len(p)
        assert set(p.unique().tolist()) <= {-1.0, 0.0, 1.0}
    # the reference's own statement of the table (rendering.py:300-302), for every part count the kernels take
    for n in range(1, 33):
        i = torch.arange(n)
        ref = torch.stack([i // 9, (i // 3) % 3, i % 3], dim=1) - 1
        ref[::2] = ref.flip(dims=(0,))[1 - n % 2::2]
        assert torch.equal(semantic_palette(n), ref.float()), n


# ------------------------------------------------------------------------------------------------------------- referee
def _two_parts(tie):
    """Two axis-aligned parts one unit apart in x: part 0 at the origin with canonical scale 0.5, part 1 at x = 1 with
    canonical scale 1 (so its canonical cube IS its local cube). Constant part-probability planes: part 0 samples 0
    (weight 0.5^3), part 1 samples ln 3 (weight 0.75^3), or 0 as well for the tie."""
    pose = torch.eye(4).repeat(1, 2, 1, 1)
    pose[0, 1, 0, 3] = 1.0
    scale = torch.tensor([[0.5, 1.0]])
    cpose = torch.eye(4).repeat(2, 1, 1)
    tri = torch.zeros(1, 96 + 6, 4, 4)
    if not tie:
        tri[0, 96 + 3:] = math.log(3.0)
    return pose, scale, cpose, tri


def test_referee_on_a_hand_worked_case():
    pts = torch.tensor([[-0.5, 0.0, 0.0],     # inside part 0 only (part 1: local x = -1.5)
                        [0.5, 0.0, 0.0],      # inside both (part 1: local x = -0.5)
                        [5.0, 5.0, 5.0],      # inside neither
                        [-1.0, 0.0, 0.0],     # on a face of part 0's local cube: |local| <= 1 is inclusive, canonical -0.5
                        [2.0, 0.0, 0.0],      # on a face of part 1's canonical cube: |canonical| < 1 is strict
                        [1.5, 0.0, 0.0]]).t()[None].contiguous()
    r = R.labels(pts, *_two_parts(tie=False))
    assert r["label"].tolist() == [[0, 1, -1, 0, -1, 1]]
    assert R.bits(r["valid"]).tolist() == [[1, 3, 0, 1, 0, 2]]
    w0, w1 = 0.125, 0.75 ** 3                 # ln 3 is stored in fp32: the sample is off by 3e-8, the weight by less
    assert np.allclose(r["top"], [[w0, w1, 0, w0, 0, w1]], rtol=0, atol=1e-7)
    assert np.allclose(r["second"], [[-1, w0, -1, -1, -1, -1]], rtol=0, atol=1e-7)
    assert r["ambiguous"].tolist() == [[False] * 6]
    # an exact tie: the lowest part wins, and the sample is ambiguous
    t = R.labels(pts, *_two_parts(tie=True))
    assert t["label"].tolist() == [[0, 0, -1, 0, -1, 1]]
    assert t["top"][0, 1] == 0.125 and t["second"][0, 1] == 0.125 and t["ambiguous"].tolist() == [[False, True] + [False] * 4]
    # uniform weights: the lowest valid part everywhere, 1 / P
    u = R.labels(pts, *_two_parts(tie=False), uniform_part_weight=True)
    assert u["label"].tolist() == [[0, 0, -1, 0, -1, 1]] and u["top"][0, 1] == 0.5 and u["second"][0, 1] == 0.5


def test_referee_composite_on_a_hand_worked_case():
    pal = semantic_palette(3)
    labels = torch.tensor([[[0, 1, 1, 2],        # masses 0.5, 0.25 + 0.125: part 0; the last label carries no weight
                            [2, -1, 2, 0],       # masses: part 2 = 0.5 + 0.125
                            [-1, -1, -1, 1],     # nothing labelled among the first Nf - 1
                            [1, 0, 0, 0],        # masses 0.25 + 0.125 vs 0.375... a tie: the lowest part
                            [1, 1, 1, 1]]])      # labelled but weightless
    w = torch.tensor([[[0.5, 0.25, 0.125], [0.5, 0.25, 0.125], [0.5, 0.25, 0.125], [0.375, 0.25, 0.125], [0.0, 0.0, 0.0]]])
    c = R.composite(labels, w, pal)
    assert c["part_map"].tolist() == [[0, 2, -1, 0, -1]]
    assert c["part_mass"].tolist() == [[0.5, 0.625, 0.0, 0.375, 0.0]]
    assert c["labelled"].tolist() == [[True, True, False, True, False]]
    assert c["ambiguous"].tolist() == [[False, False, False, True, False]]
    want0 = 0.5 * pal[0].double() + 0.375 * pal[1].double()
    assert np.array_equal(c["color"][0, :, 0], want0.numpy()) and np.array_equal(c["color"][0, :, 2], np.zeros(3))
    # an ambiguous sample lends its weight to the ray's slack
    amb = torch.zeros(1, 5, 4, dtype=torch.bool)
    amb[0, 0, 2] = True                          # 0.125 of ray 0 may move: 0.5 against 0.375 is then within reach
    assert R.composite(labels, w, pal, amb)["ambiguous"].tolist() == [[True, False, False, True, False]]


# ------------------------------------------------------------------------------------------------ host-side rejections
def _frames(P, B=1, H=8):
    return torch.zeros(B, P, 16), torch.zeros(P, 4, 4), torch.zeros(B, 96 + 3 * P, H, H)


def test_host_side_rejections():
    parts, cpose, tri = _frames(23)
    pts = torch.zeros(1, 3, 10)
    with pytest.raises(ValueError, match="at most 32"):
        ops.part_labels(pts, *_frames(33))
    with pytest.raises(ValueError):
        ops.part_labels(torch.zeros(1, 10, 3), parts, cpose, tri)                # (B, M, 3) without points_last
    with pytest.raises(ValueError):
        ops.part_labels(torch.zeros(10, 4), parts, cpose, tri, points_last=True)
    with pytest.raises(ValueError):
        ops.part_labels(pts, parts, torch.zeros(24, 4, 4), tri)
    with pytest.raises(ValueError):
        ops.part_labels(pts, parts, cpose, torch.zeros(1, 96 + 3 * 24, 8, 8))   # planes of another part count
    with pytest.raises(ValueError):
        ops.part_labels(pts, parts, cpose, torch.zeros(3, 96 + 69, 8, 8))       # tri-plane batch neither 1 nor B
    with pytest.raises(ValueError):
        ops.part_labels(torch.zeros(2, 3, 10), parts, cpose, tri)                # frames of another batch
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.part_labels(pts, parts, cpose, tri)
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.part_labels(torch.zeros(10, 3), parts, cpose, tri, points_last=True)
    n, Nf = 5, 8
    ray = dict(image_coord=torch.zeros(1, 1, 3, n), inv_intrinsics=torch.eye(3), depth_min=torch.zeros(1, n),
               depth_max=torch.ones(1, n), bins=torch.zeros(1, n, Nf))
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.part_labels_on_rays(**ray, parts=parts, canonical_pose=cpose, tri_nchw=tri)
    for bad in (dict(depth_min=torch.zeros(1, n + 1)), dict(bins=torch.zeros(1, n + 1, Nf)), dict(inv_intrinsics=torch.eye(4)),
                dict(image_coord=torch.zeros(1, 2, n))):
        with pytest.raises(ValueError):
            ops.part_labels_on_rays(**{**ray, **bad}, parts=parts, canonical_pose=cpose, tri_nchw=tri)
    with pytest.raises(ValueError, match="at most 32"):
        ops.part_labels_on_rays(**ray, parts=_frames(33)[0], canonical_pose=_frames(33)[1], tri_nchw=_frames(33)[2])
    labels, pal = torch.zeros(1, n, Nf, dtype=torch.int32), semantic_palette(23)
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.semantic_composite(labels, torch.zeros(1, 1, n, Nf - 1), pal)
    with pytest.raises(ValueError, match="closes the last interval"):
        ops.semantic_composite(labels, torch.zeros(1, 1, n, Nf), pal)           # Nf mismatch between labels and weights
    with pytest.raises(ValueError):
        ops.semantic_composite(torch.zeros(1, n, 129, dtype=torch.int32), torch.zeros(1, 1, n, 128), pal)
    with pytest.raises(ValueError):
        ops.semantic_composite(torch.zeros(1, n, 1, dtype=torch.int32), torch.zeros(1, 1, n, 0), pal)
    with pytest.raises(ValueError):
        ops.semantic_composite(labels, torch.zeros(1, 1, n, Nf - 1), semantic_palette(33))
    with pytest.raises(ValueError):
        ops.semantic_composite(labels, torch.zeros(1, 1, n, Nf - 1), torch.zeros(23, 4))


def test_semantic_map_with_gradients_raises_not_implemented():
    from enarf_gan_amd.models.narf import TriPlaneNARF
    from test_host_cpu import _nerf_cfg
    sc = Scene(16, 1, "center_fixed", 20)
    m = TriPlaneNARF(_nerf_cfg(Nc=8, Nf=8), 20, 24, parent=sc.raw["parents"], num_bone_param=23)
    m.register_canonical_pose(sc.raw["canonical_pose"])
    mi = {"z": None, "z_rend": sc.raw["z_rend"], "bone_length": sc.bl_parts, "truncation_psi": 1}
    assert m.tri_plane.requires_grad
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="semantic_map"):
        render(m, sc.raw["image_coord"], sc.pose_parts, sc.raw["inv_intrinsics"], Nc=8, Nf=8, semantic_map=True, model_input=mi)


# ------------------------------------------------------------------------------ the referee alone, on the GPU tests' scenes
@pytest.mark.parametrize("batch,ol", [(1, "center_fixed"), (2, "center_fixed"), (1, "center+head")])
def test_referee_ambiguity_stays_within_the_caps(batch, ol):
    """The caps of tests/test_gpu_seg.py hold for the referee itself on the scenes that file uses (the importance samples
    are the oracle's own draw here): few samples have two part weights within AMBIGUITY, few rays two such masses."""
    sc = Scene(16, batch, ol, 20)
    torch.manual_seed(3)
    _, _, _, taps = sc.oracle_render(sc.raw["image_coord"], 48, 64, None)
    n, Nf = 256, 64
    pts = R.ray_points(sc.raw["image_coord"], sc.raw["inv_intrinsics"], taps["depth_min"], taps["depth_max"], taps["bins"])
    r = R.labels(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"])
    assert torch.equal(r["valid"].reshape(batch, sc.P, n, Nf), taps["fine_valid"])
    multi = int((r["n_valid"] > 1).sum())
    amb = int(r["ambiguous"].sum())
    print(f"B={batch} {ol}: {amb} ambiguous of {multi} samples with two or more valid parts")
    assert multi > 1000 and amb <= R.MAX_AMBIGUOUS_SAMPLES * multi
    w = taps["fine_weights"] * (taps["ray_validity"] if batch == 1 else torch.ones_like(taps["ray_validity"]))[..., None]
    c = R.composite(r["label"].reshape(batch, n, Nf), w, semantic_palette(sc.P), r["ambiguous"].reshape(batch, n, Nf))
    rays, amb_rays = int(c["labelled"].sum()), int(c["ambiguous"].sum())
    print(f"B={batch} {ol}: {amb_rays} ambiguous of {rays} labelled rays")
    assert rays > 50 and amb_rays <= R.MAX_AMBIGUOUS_RAYS * rays
    assert len(np.unique(c["part_map"][c["labelled"]])) >= 5
