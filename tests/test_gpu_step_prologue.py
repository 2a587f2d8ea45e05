"""The serial stretch between the end of one march and the first texel load of the next (DESIGN.md 3.1 "start-up", 3.2):

* the prepare role of the pre-march launch is sliced: layers 0 and 1 of an image's MLP pack are written by 4 and 8 blocks of
  512 weights each instead of one block per layer (prepare_role_block, csrc/enarf_render.hip). A slice redoes the layer's
  style product and demodulates its own rows, so the pack and the part frames must come out bit for bit as enarf_prepare
  (one block per layer) writes them: for one and three images, 23 and 24 parts, a short and a long style vector;
* the tri-plane re-layout role of the same launch against the stand-alone enarf_triplane_pack, at the plane sizes at which
  its blocks take another path: below, at and one past the 64-texel row segment, odd segment counts, rows whose segments
  alternate between the 16-byte and the 4-byte path (W = 68), a tensor 4 bytes off 16-byte alignment, one and three
  tri-planes, with and without mask channels behind the 96 feature channels, and a few thousand segments;
* render_kernel (march="ray") stages the first image's MLP pack, biases and part frames with every load in flight at once
  (stage_common_batched, csrc/enarf_march.h); loads past the end of a section are clamped and their stores skipped. That
  changes no value: every case asks for the same bits as march="task" (which stages with the plain loop) and as a second
  run, in all outputs, the drawn bins and the work counters, and for a silent watchdog. The cases are launches with fewer
  rays than workgroups and ragged ray counts, a batch whose live rays all sit in the last frame, a frame 0 that misses every
  cube in a batch that drops nothing (the missed-ray pass runs in the LDS section the staging then fills), a frame nobody
  hits (every workgroup leaves at its first pop), two sample counts and the f32 and f16x3 packs (different section sizes).
"""
import pytest
import torch

from _helpers import DeviceScene, Scene

pytestmark = pytest.mark.gpu
OUTPUTS = ("color", "mask", "disparity", "fine_weights", "fine_depth")
GUARD = 1024          # floats of canary on either side of the channel-last planes


@pytest.fixture(scope="module")
def ops():
    from enarf_gan_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


_SCENES = {}


def _scene(B):
    if B not in _SCENES:
        _SCENES[B] = Scene(32, B, "center_fixed", 20)
    return _SCENES[B]


def _status():
    from enarf_gan_amd import _lib
    return _lib.device_status(clear=False)


# ---------------------------------------------------------------------------------------------------- the prepare role
@pytest.mark.parametrize("B,origin,style_dim", [(1, "center_fixed", 20), (3, "center_fixed", 20), (1, "center+head", 20),
                                                (3, "center+head", 256)])
def test_sliced_prepare_role_matches_prepare(ops, B, origin, style_dim):
    """the pre-march launch alone (ENARF_STEP_PRE) against enarf_prepare: part frames and every byte of the MLP packs"""
    sc = Scene(32, B, origin, style_dim)
    s, d = sc.raw, torch.device("cuda:0")
    mlp = {k: v.to(d) for k, v in s["mlp"].items()}
    pose, bl, cbl, z = s["pose_to_camera"].to(d), s["bone_length"].to(d), sc.cbl.to(d), s["z_rend"].to(d)

    def buffers():      # the same canary in both, so that a byte neither entry writes compares equal
        return (torch.full((B, sc.P, 16), 777.0, device=d),
                torch.full((B, ops.mlp_pack_bytes()), 0xA5, dtype=torch.uint8, device=d))

    ref_parts, ref_pack = buffers()
    ops.prepare(pose, bl, cbl, z, mlp, s["parents"], sc.ol, sc.cs, parts_out=ref_parts, pack_out=ref_pack)      # a block per layer
    parts, pack = buffers()
    tri = s["tri_plane"][:1, :, :8, :8].contiguous().to(d)
    st = ops.RenderStep(pose, bl, cbl, z, mlp, s["parents"], sc.ol, sc.cs, s["image_coord"][..., :64].contiguous().to(d),
                        s["inv_intrinsics"].to(d), sc.cpose.to(d), tri, torch.empty(1, 3, 8, 8, 32, device=d), 16, 16,
                        parts_out=parts, pack_out=pack)
    st.run(ops.STEP_PRE)
    torch.cuda.synchronize()
    assert sc.P == (24 if origin == "center+head" else 23)
    assert not bool((ref_parts == 777.0).any()) and int((ref_pack != 0xA5).sum()) > ref_pack.numel() // 2
    assert torch.equal(parts, ref_parts), "part frames"
    assert torch.equal(pack, ref_pack), "MLP pack"
    assert _status() == 0


# ---------------------------------------------------------------------------------------------------- the re-layout role
def _relayout_case(ops, tri_B, extra_ch, H, W, misalign=False):
    """the pre-march launch alone (ENARF_STEP_PRE) on random planes of the given shape; returns (tri, planes written by the
    fused role, the two guards)"""
    sc = _scene(tri_B)
    s, d = sc.raw, torch.device("cuda:0")
    Ct = 96 + (3 * sc.P if extra_ch else 0)
    g = torch.Generator().manual_seed(1000 * H + W + tri_B)
    numel = tri_B * Ct * H * W
    flat = torch.empty(numel + 4, device=d)
    flat[:] = torch.randn(numel + 4, generator=g).to(d)
    off = 1 if misalign else 0
    tri = flat[off:off + numel].view(tri_B, Ct, H, W)
    assert tri.data_ptr() % 16 == (4 if misalign else 0) and tri.is_contiguous()
    n_out = tri_B * 3 * H * W * 32
    buf = torch.full((n_out + 2 * GUARD,), float("nan"), device=d)
    feat = buf[GUARD:GUARD + n_out].view(tri_B, 3, H, W, 32)
    mlp = {k: v.to(d) for k, v in s["mlp"].items()}
    st = ops.RenderStep(s["pose_to_camera"].to(d), s["bone_length"].to(d), sc.cbl.to(d), s["z_rend"].to(d), mlp,
                        s["parents"], sc.ol, sc.cs, s["image_coord"][..., :64].contiguous().to(d), s["inv_intrinsics"].to(d),
                        sc.cpose.to(d), tri, feat, 16, 16)
    assert st.tri.data_ptr() == tri.data_ptr()
    st.run(ops.STEP_PRE)
    torch.cuda.synchronize()
    return tri, feat, (buf[:GUARD], buf[GUARD + n_out:])


def _assert_relayout(ops, tri, feat, guards):
    B, _, H, W = tri.shape
    alone = ops.triplane_pack(tri)
    assert torch.equal(feat, alone), "fused re-layout role differs from enarf_triplane_pack"
    assert torch.equal(feat, tri[:, :96].reshape(B, 3, 32, H, W).permute(0, 1, 3, 4, 2)), "re-layout differs from a permute"
    for gd in guards:
        assert bool(torch.isnan(gd).all()), "the role wrote outside the planes"
    assert _status() == 0


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (5, 3), (64, 64), (7, 65), (65, 7), (4, 130), (130, 4), (5, 68)])
@pytest.mark.parametrize("tri_B", [1, 3])
@pytest.mark.parametrize("extra_ch", [True, False], ids=["ch96+3P", "ch96"])
def test_relayout_role_matches_standalone_pack(ops, H, W, tri_B, extra_ch):
    """plane sizes around the 64-texel segment (both orientations of the odd ones), one and three tri-planes, with and
    without the mask channels behind the 96 feature channels"""
    _assert_relayout(ops, *_relayout_case(ops, tri_B, extra_ch, H, W))


@pytest.mark.parametrize("H,W", [(5, 3), (64, 64), (7, 65), (5, 68)])
def test_relayout_role_unaligned_tensor(ops, H, W):
    """a tri-plane tensor 4 bytes past 16-byte alignment: every segment takes the 4-byte path"""
    _assert_relayout(ops, *_relayout_case(ops, 1, True, H, W, misalign=True))


@pytest.mark.parametrize("H,W,tri_B", [(130, 64, 3),      # 1 170 segments
                                       (129, 68, 1),      # 774 segments, wide and ragged ones alternating
                                       (256, 128, 3)])    # 4 608 segments: more than are resident at once
def test_relayout_role_many_segments(ops, H, W, tri_B):
    """more row segments than a handful: the role's block index to (plane, row, segment) map over several planes"""
    _assert_relayout(ops, *_relayout_case(ops, tri_B, False, H, W))


# ---------------------------------------------------------------------------------------------------- the march's start-up
def _check(ds, coord, Nc, Nf, **kw):
    """march="ray" twice and march="task" once: equal bits everywhere, no watchdog; returns the first run"""
    assert _status() == 0
    a = ds.render(coord, Nc, Nf, None, count=True, return_bins=True, march="ray", **kw)
    again = ds.render(coord, Nc, Nf, None, count=True, return_bins=True, march="ray", **kw)
    task = ds.render(coord, Nc, Nf, None, count=True, return_bins=True, march="task", **kw)
    torch.cuda.synchronize()
    for other, what in ((again, "second run"), (task, "task march")):
        for name in OUTPUTS:
            assert torch.equal(getattr(a, name), getattr(other, name)), (name, what, Nc, Nf, kw)
        assert torch.equal(a.taps["bins"], other.taps["bins"]), ("bins", what, Nc, Nf, kw)
        assert torch.equal(a.counters[:4], other.counters[:4]), (what, a.counters, other.counters)
        assert int(other.counters[7]) == 0, what
    assert int(a.counters[7]) == 0
    assert _status() == 0
    return a


@pytest.fixture(scope="module")
def frame32():
    sc = _scene(1)
    return sc, DeviceScene(sc)


def _missing_columns():
    """columns 0 .. 3 of every row of the 32 x 32 frame miss every part's cube: 128 rays"""
    return torch.tensor([r * 32 + c for r in range(32) for c in range(4)])


def _body_rays(n):
    """n consecutive pixels from the middle of row 12 on: through the body"""
    return torch.arange(32 * 12 + 14, 32 * 12 + 14 + n)


SHAPES = [(16, 16, "f32"), (16, 16, "f16x3"), (48, 64, "f32"), (48, 64, "f16x3")]


@pytest.mark.parametrize("Nc,Nf,mode", SHAPES)
@pytest.mark.parametrize("n", [1, 3, 33, 257])
def test_startup_few_and_ragged_ray_counts(ops, frame32, n, Nc, Nf, mode):
    """one frame, fewer rays than workgroups, counts that are no multiple of 32 or 64: most workgroups find the queues
    drained at their first pop, the others march one ray on a freshly staged image context"""
    sc, ds = frame32
    idx = torch.tensor([16 * 32 + 16]) if n == 1 else _body_rays(n)
    a = _check(ds, sc.raw["image_coord"][..., idx].contiguous(), Nc, Nf, seed=21, mlp_mode=mode)
    assert 0 < int(a.counters[2]) <= n
    assert float(a.mask.max()) > 0.05


@pytest.mark.parametrize("Nc,Nf,mode", [(16, 16, "f32"), (48, 64, "f16x3")])
def test_startup_first_ray_in_the_last_frame(ops, Nc, Nf, mode):
    """B = 2, a tri-plane per frame, every live ray in frame 1: frame 0's bands hold no ray to march, so every workgroup's
    first ray - the one whose image it stages at start-up - comes from frame 1, for half the XCDs out of another band;
    frame 1 marched with frame 0's MLP pack, part frames or planes would not give the task march's bits"""
    sc = _scene(2)
    assert not torch.equal(sc.raw["pose_to_camera"][0], sc.raw["pose_to_camera"][1])
    assert not torch.equal(sc.raw["tri_plane"][0], sc.raw["tri_plane"][1])
    ds = DeviceScene(sc)
    coord = torch.stack([sc.raw["image_coord"][0][..., _missing_columns()],
                         sc.raw["image_coord"][1][..., _body_rays(128)]]).contiguous()
    a = _check(ds, coord, Nc, Nf, seed=22, mlp_mode=mode)
    assert float(a.mask[0].abs().max()) == 0.0 and float(a.mask[1].max()) > 0.05
    assert int(a.counters[2]) == 2 * 128          # a batch drops nothing: missed and marched rays together


@pytest.mark.parametrize("Nc,Nf,mode", [(16, 16, "f32"), (48, 64, "f16x3")])
def test_startup_missed_ray_pass_ahead_of_staging(ops, Nc, Nf, mode):
    """B = 3, every ray of frame 0 misses all cubes, nothing dropped: the missed-ray pass runs on scratch slots in the MLP
    section, and the image context is staged over them afterwards"""
    sc = _scene(3)
    ds = DeviceScene(sc)
    ic = sc.raw["image_coord"]
    coord = torch.stack([ic[0][..., _missing_columns()], ic[1][..., _body_rays(128)], ic[2][..., _body_rays(128)]]).contiguous()
    a = _check(ds, coord, Nc, Nf, seed=23, mlp_mode=mode, drop_invalid_rays=False)
    assert float(a.mask[0].abs().max()) == 0.0
    assert float(a.mask[1].max()) > 0.05 and float(a.mask[2].max()) > 0.05
    assert int(a.counters[2]) == 3 * 128


@pytest.mark.parametrize("Nc,Nf,mode", [(16, 16, "f32"), (48, 64, "f16x3")])
def test_startup_frame_without_a_hit(ops, frame32, Nc, Nf, mode):
    """a single frame whose rays all miss: everything is dropped, every workgroup returns at its first pop"""
    sc, ds = frame32
    a = _check(ds, sc.raw["image_coord"][..., _missing_columns()].contiguous(), Nc, Nf, seed=24, mlp_mode=mode)
    assert int(a.counters[2]) == 0
    assert float(a.mask.abs().max()) == 0.0 and float(a.color.abs().max()) == 0.0
