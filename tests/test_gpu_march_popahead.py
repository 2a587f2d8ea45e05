"""render_kernel (march="ray"): the pop of the next queue entry and the sorted uniforms + S2 no longer belong to the wave
without a coarse tile (which composites the previous ray first and so came to the coarse barrier last behind short coarse
tiles): a count in LDS hands the pop to the wave that finishes its coarse tile FIRST and the draw and S2 to the second
(popping and drawing ahead of the compositing wave's wait, the form first proposed, measured slower). The
change reschedules only, so every case asks what tests/test_gpu_march_handoff.py asks: the same bits as march="task" - the
schedule that shares the stages but none of this loop - in all outputs, the drawn bins and the work counters, the same bits
from a second run of itself, a silent hand-off watchdog (counters[7]) and a clean device status.

The frame is 32 x 32. A launch has min(3 per CU, rays) workgroups, which is more than the frame's live rays: on the frame
itself nearly every workgroup marches ONE ray - the turn count's first use, a pop that finds the queues drained, the last-ray
exit. The steady state - the count running up by 4 per ray, records popped by one wave and read by all, S2 moving from wave
to wave, the compositing wave arriving late - needs workgroups that march several rays, so every shape also runs on the same
frame's rays four times over in one launch (`_tiled`; 4 096 rays, more than twice the workgroups live). The shapes are those
at which the loop takes another path: a wave without a coarse tile (Nc 48), none (Nc 64: wave 0 composites, then runs its
coarse tile), waves without a fine tile (Nf 32), two tiles per wave (72 + 96), a change of image - two restage barriers
between the compositing and the turn count - with the missed-ray pass in front (B = 3), per-frame tri-planes (B = 2), fine
tiles that early termination skips, and bins from the caller (no draw at all).
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


def _wgs(n_rays):
    return min(3 * torch.cuda.get_device_properties(0).multi_processor_count, n_rays)


def _tiled(coord, times=4):
    """the same rays `times` over, along the ray axis: ray ids differ, so every copy draws its own uniforms"""
    return torch.cat([coord] * times, dim=-1).contiguous()


def _several_rays_per_workgroup(out, n_rays):
    return int(out.counters[2]) > 2 * _wgs(n_rays)


def _status():
    from enarf_gan_amd import _lib
    return _lib.device_status(clear=False)


def _check(ds, coord, Nc, Nf, bins=None, **kw):
    """march="ray" twice and march="task" once: equal bits everywhere, no watchdog; returns the first run"""
    assert _status() == 0
    a = ds.render(coord, Nc, Nf, bins, count=True, return_bins=True, march="ray", **kw)
    again = ds.render(coord, Nc, Nf, bins, count=True, return_bins=True, march="ray", **kw)
    task = ds.render(coord, Nc, Nf, bins, count=True, return_bins=True, march="task", **kw)
    torch.cuda.synchronize()
    for other, what in ((again, "second run"), (task, "task march")):
        for name in OUTPUTS:
            assert torch.equal(getattr(a, name), getattr(other, name)), (name, what, Nc, Nf, kw)
        assert torch.equal(a.taps["bins"], other.taps["bins"]), ("bins", what, Nc, Nf, kw)
        assert torch.equal(a.counters[:4], other.counters[:4]), (what, a.counters, other.counters)
        assert int(other.counters[7]) == 0, what
    assert int(a.counters[7]) == 0
    assert _status() == 0
    print("counters", Nc, Nf, tuple(coord.shape), kw, a.counters.tolist())
    return a


SHAPES = [(48, 64, dict()),                       # a wave without a coarse tile: it composites, others pop and run S2
          (64, 64, dict()),                       # no such wave: wave 0 composites ahead of its coarse tile
          (48, 32, dict()),                       # two waves without a fine tile
          (72, 96, dict()),                       # SPL = 2: two tiles per wave and pass
          (48, 64, dict(early_stop_eps=1e-3))]    # skip flags, read by S4 and the fine tiles


@pytest.mark.parametrize("Nc,Nf,kw", SHAPES)
def test_frame_of_single_ray_workgroups(ops, frame32, Nc, Nf, kw):
    """the 32 x 32 frame as it is: fewer live rays than workgroups, so a workgroup's first ray is (nearly always) its last"""
    sc, ds = frame32
    coord = sc.raw["image_coord"]
    a = _check(ds, coord, Nc, Nf, seed=31, mlp_mode="f16x3", **kw)
    assert 0 < int(a.counters[2]) < _wgs(coord.shape[-1])
    assert float(a.mask.max()) > 0.05
    if kw:
        assert int(a.counters[4]) > 0, "early termination skipped no fine tile"


def test_eight_rays_eight_workgroups(ops, frame32):
    """the frame cropped to 8 rays through the body: a grid of 8 workgroups with a ray each (or two and none): the last-ray
    path: a pop on drained queues, compositing on wave 0 alone"""
    sc, ds = frame32
    idx = torch.arange(32 * 12 + 14, 32 * 12 + 14 + 8)
    a = _check(ds, sc.raw["image_coord"][..., idx].contiguous(), 48, 64, seed=32, mlp_mode="f16x3")
    assert 0 < int(a.counters[2]) <= 8 and float(a.mask.max()) > 0.05


@pytest.mark.parametrize("Nc,Nf,kw", SHAPES)
def test_steady_state_of_each_shape(ops, frame32, Nc, Nf, kw):
    """the frame's rays four times over: workgroups march several rays in a row, so the turn count runs up ray after ray and
    the pop and S2 move from wave to wave"""
    sc, ds = frame32
    coord = _tiled(sc.raw["image_coord"])
    a = _check(ds, coord, Nc, Nf, seed=33, mlp_mode="f16x3", **kw)
    assert _several_rays_per_workgroup(a, coord.shape[-1]), a.counters.tolist()
    assert float(a.mask.max()) > 0.05
    if kw:
        assert int(a.counters[4]) > 0, "early termination skipped no fine tile"


@pytest.mark.parametrize("times", [1, 4])
def test_bins_from_the_caller_no_draw(ops, frame32, times):
    """bins supplied: nothing is drawn, the second wave only runs S2; the bins are those an earlier launch drew"""
    sc, ds = frame32
    coord = _tiled(sc.raw["image_coord"], times)
    drawn = ds.render(coord, 48, 64, None, return_bins=True, march="task", seed=34, mlp_mode="f16x3").taps["bins"]
    a = _check(ds, coord, 48, 64, bins=drawn, seed=35, mlp_mode="f16x3")
    assert torch.equal(a.taps["bins"], drawn)
    assert _several_rays_per_workgroup(a, coord.shape[-1]) == (times == 4)
    assert float(a.mask.max()) > 0.05


@pytest.mark.parametrize("times", [1, 4])
def test_change_of_image_ahead_of_the_turn_count(ops, times):
    """B = 3 frames, one tri-plane, three poses, nothing dropped: columns 0 .. 3 of every row of frame 0 miss every part's cube, so
    the missed-ray pass runs first; the lists are in image order and hold more live rays than there are workgroups, so workgroups
    go from one image to the next: the two restage barriers come ahead of the coarse tiles and of the turn count"""
    sc = Scene(32, 3, "center_fixed", 20)
    assert not torch.equal(sc.raw["pose_to_camera"][0], sc.raw["pose_to_camera"][1])
    sc.raw["tri_plane"] = sc.raw["tri_plane"][:1].contiguous()
    ds = DeviceScene(sc)
    coord = _tiled(sc.raw["image_coord"], times)
    n = coord.shape[-1]
    a = _check(ds, coord, 48, 64, seed=36, mlp_mode="f16x3", drop_invalid_rays=False)
    assert int(a.counters[2]) == 3 * n                    # missed and marched rays together
    missing = torch.tensor([t * 1024 + r * 32 + c for t in range(times) for r in range(32) for c in range(4)])
    assert float(a.mask[0, missing].abs().max()) == 0.0    # frame 0's pose leaves those columns empty
    hit = int((a.mask > 0).sum())                          # a lower bound of the marched rays
    assert hit > (2 if times == 4 else 1) * _wgs(3 * n), (hit, "too few live rays for workgroups to change image")
    for f in range(3):
        assert float(a.mask[f].max()) > 0.05
    assert not torch.equal(a.mask[0], a.mask[1]) and not torch.equal(a.mask[1], a.mask[2])


def test_per_frame_triplanes(ops):
    """B = 2, a tri-plane per frame: the restaged image context brings other planes along with the pack and the part frames"""
    sc = Scene(32, 2, "center_fixed", 20)
    assert not torch.equal(sc.raw["tri_plane"][0], sc.raw["tri_plane"][1])
    ds = DeviceScene(sc)
    coord = _tiled(sc.raw["image_coord"])
    a = _check(ds, coord, 48, 64, seed=37, mlp_mode="f16x3")
    assert int(a.counters[2]) == 2 * coord.shape[-1]      # a batch drops nothing: missed and marched rays together
    hit = int((a.mask > 0).sum())                          # a lower bound of the marched rays
    assert hit > 2 * _wgs(2 * coord.shape[-1]), (hit, "too few live rays for several per workgroup")
    assert float(a.mask[0].max()) > 0.05 and float(a.mask[1].max()) > 0.05
    assert not torch.equal(a.mask[0], a.mask[1])
