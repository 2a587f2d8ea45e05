"""render_kernel (march="ray") hands a ray's fine tiles to its compositing wave by a count in LDS instead of a workgroup
barrier: the three other waves go straight on to the next ray's coarse tiles. The change reschedules only,
so every case here asks for the same bits as march="task" - the schedule that shares the stages but none of this code - in
all outputs, the drawn bins and the work counters, for the same bits from a second run of itself, and for a silent hand-off
watchdog (counters[7] and the device's sticky status word).

The cases are the shapes at which the hand-off takes another path: a spare coarse wave that composites (Nc 48), none
(Nc 64: the compositing wave owns a coarse tile), two tiles per wave (72 + 96), waves without a fine tile that must still
count themselves in (Nf 32, 48), a change of image (the restage path keeps its full barrier), workgroups that start on a
drained queue and a last ray whose compositing wave is the only one left, and fine tiles that early termination skips.
"""
import pytest
import torch

from _helpers import DeviceScene, Scene

pytestmark = pytest.mark.gpu
OUTPUTS = ("color", "mask", "disparity", "fine_weights", "fine_depth")


@pytest.fixture(scope="module")
def ops():
    from enarf_gan_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def frame32():
    sc = Scene(32, 1, "center_fixed", 20)
    return sc, DeviceScene(sc)


@pytest.fixture(scope="module")
def frame64():
    """64 x 64 rays, 1 966 of them live: more than twice the workgroups of a launch (3 per CU), so that workgroups march
    several rays in a row and the steady state of the loop runs - a compositing wave beside three waves that are already in
    the next ray's coarse tiles, a count that grows past 4"""
    sc = Scene(64, 1, "center_fixed", 20)
    return sc, DeviceScene(sc)


def _several_rays_per_workgroup(out):
    wgs = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    return int(out.counters[2]) > 2 * wgs


def _status():
    from enarf_gan_amd import _lib
    return _lib.device_status(clear=False)


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
    print("counters", Nc, Nf, kw, a.counters.tolist())
    return a


def test_spare_wave_composites_flagship_shape(ops, frame64):
    """Nc 48 + Nf 64 on a whole 64 x 64 frame: the wave without a coarse tile in the next ray waits for the count, and every
    workgroup marches several rays, so the count runs up over many rays"""
    sc, ds = frame64
    a = _check(ds, sc.raw["image_coord"], 48, 64, seed=5, mlp_mode="f16x3")
    assert _several_rays_per_workgroup(a) and float(a.mask.max()) > 0.05


@pytest.mark.parametrize("Nc,Nf,kw", [(64, 64, dict()),                   # no spare wave: S4 on a wave that owns a coarse tile
                                      (72, 96, dict()),                   # two tiles per wave, no spare (auto would pick the task march)
                                      (48, 32, dict()), (48, 48, dict()),    # two waves / one wave without a fine tile
                                      (48, 64, dict(early_stop_eps=1e-3))])  # skipped fine tiles: a wave is done at once
def test_handoff_shapes(ops, frame64, Nc, Nf, kw):
    """the whole 64 x 64 frame, like the flagship case: each shape's own steady state (wave 0 compositing while waves 1 - 3
    are in the next coarse tiles, two tiles per wave, waves without a fine tile counting ray after ray, skipped fine tiles
    with a next ray pending) needs workgroups that march several rays"""
    sc, ds = frame64
    a = _check(ds, sc.raw["image_coord"], Nc, Nf, seed=7, mlp_mode="f16x3", **kw)
    assert _several_rays_per_workgroup(a), (a.counters.tolist(), "too few live rays for several per workgroup")
    assert float(a.mask.max()) > 0.05
    if kw:
        assert int(a.counters[4]) > 0, "early termination skipped no fine tile"


def test_change_of_image_keeps_its_barrier(ops):
    """two frames, one tri-plane, different poses: workgroups that run out of rays of the first image restage the second
    image's MLP pack and part frames behind a full barrier, while the compositing of their last ray is handed off by count"""
    sc = Scene(64, 2, "center_fixed", 20)
    assert not torch.equal(sc.raw["pose_to_camera"][0], sc.raw["pose_to_camera"][1])
    sc.raw["tri_plane"] = sc.raw["tri_plane"][:1].contiguous()
    ds = DeviceScene(sc)
    a = _check(ds, sc.raw["image_coord"], 48, 64, seed=3, mlp_mode="f16x3")
    assert _several_rays_per_workgroup(a)
    assert float(a.mask[0].max()) > 0.05 and float(a.mask[1].max()) > 0.05
    assert not torch.equal(a.mask[0], a.mask[1])


def test_short_queues(ops, frame32):
    """fewer live rays than workgroups (most workgroups march one ray: its S4 takes the exit path, on wave 0 alone; the rest
    find every queue drained), and exactly one live ray among rays that miss the body"""
    sc, ds = frame32
    coord = sc.raw["image_coord"]
    wgs = min(3 * torch.cuda.get_device_properties(0).multi_processor_count, coord.shape[-1])
    a = _check(ds, coord, 48, 64, seed=11, mlp_mode="f16x3")
    assert 0 < int(a.counters[2]) < wgs, (int(a.counters[2]), wgs)
    # columns 0 .. 3 of every row miss every part's cube; the centre pixel does not
    idx = torch.tensor([r * 32 + c for r in range(32) for c in range(4)] + [16 * 32 + 16])
    one = _check(ds, coord[..., idx].contiguous(), 48, 64, seed=11, mlp_mode="f16x3")
    assert int(one.counters[2]) == 1
    assert float(one.mask[0, :-1].abs().max()) == 0.0
