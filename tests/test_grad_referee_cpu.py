"""What the per-element gradient bound of tests/grad_referee.py accepts and rejects, on the CPU with the oracle alone: the
fp32 computations outside the bound's yardstick pass against the float64 referee; the fp32 oracle's gradients with their small entries dropped, or with
1 % of the texels off by 1 %, fail (the first passes the max-normalised 1e-3 bound the older backward tests use)."""
import numpy as np
import pytest
import torch

import grad_referee as R
from _helpers import Scene, rel_err


@pytest.fixture(scope="module")
def band():
    """72 rays through the body of a 32^2 frame, Nc 48, Nf 32, sorted random bins, random upstream gradients."""
    sc = Scene(32, 1, "center_fixed", 20)
    n_rays, Nc, Nf = 72, 48, 32
    start = 32 * 32 // 2 - n_rays // 2
    coord = sc.raw["image_coord"][..., start:start + n_rays].contiguous()
    bins = torch.rand(1, n_rays, Nf, generator=torch.Generator().manual_seed(3)).sort(-1).values
    g = torch.Generator().manual_seed(5)
    gc, gm, gd = torch.randn(1, 3, n_rays, generator=g), torch.randn(1, n_rays, generator=g), torch.randn(1, n_rays, generator=g)
    return dict(R.referee(sc, coord, Nc, Nf, bins, gc, gm, gd), args=(sc, coord, Nc, Nf, bins, gc, gm, gd))


def test_referee_decisions_agree(band):
    assert bool(band["keep"].all())                     # no ray of this band needs excluding
    assert float(band["out32"][1].max()) > 0.5
    assert len(band["draws"]) == R.DRAWS


def test_fp32_computations_outside_the_yardstick_pass(band):
    """Independent fp32 arithmetic - the same graph on inputs moved by up to one ulp with other seeds than the yardstick's
    draws - stays within the bound on every entry of every tensor."""
    sc, coord, Nc, Nf, bins, gc, gm, gd = band["args"]
    for j in (50, 51, 52, 53):
        o, l, _ = R.render_forward(R.perturbed_scene(sc, j), coord, Nc, Nf, R.perturb(bins, 1000 + j).sort(-1).values,
                                   torch.float32)
        worst = R.check_grads(R.render_grads(o, l, gc, gm, gd, band["keep"]), band, f"held-out fp32 draw {j}")
        assert len(worst) == 15


@pytest.mark.parametrize("k", ["feat", "mask"])
def test_bound_rejects_small_entries_set_to_zero(band, k):
    r64, r32 = band["g64"][k].numpy(), band["g32"][k].numpy()
    z = r32.copy()
    z[np.abs(z) < 1e-3 * np.abs(z).max()] = 0
    assert rel_err(z, r64).max() <= 1.01e-3                      # the old bound lets this through
    rt = R.bound_ratios(k, z, r64, r32, draws=[d[k].numpy() for d in band["draws"]])
    assert rt.max() > 100 and (rt > 1).sum() > 1000, (rt.max(), (rt > 1).sum())


@pytest.mark.parametrize("k", ["feat", "mask"])
def test_bound_rejects_one_percent_of_texels_off_by_one_percent(band, k):
    r64, r32 = band["g64"][k].numpy(), band["g32"][k].numpy()
    Bt, C, H, W = r32.shape
    sel = np.random.default_rng(0).random((Bt, 1, H, W)) < 0.01
    s = np.where(sel, r32 * np.float32(0.99), r32)
    rt = R.bound_ratios(k, s, r64, r32, draws=[d[k].numpy() for d in band["draws"]])
    assert rt.max() > 10 and (rt > 1).sum() >= 10, (rt.max(), (rt > 1).sum())


def test_bound_groups_and_edges():
    """A feature-plane texel's 32 channels form one group; an entry the referee holds at zero must be zero up to the floor;
    a tensor the referee holds at zero everywhere must be zero exactly."""
    r64 = np.zeros((1, 96, 2, 3))
    r64[0, 5, 1, 2] = 1.0
    r32 = r64.copy()
    ours = r64.copy()
    ours[0, 6, 1, 2] = 5e-5                                     # same texel as the 1.0: within RTOL of the group
    assert R.bound_ratios("feat", ours, r64, r32).max() <= 1
    ours[0, 6, 1, 1] = 5e-5                                     # a texel the referee holds at zero: above FLOOR
    rt = R.bound_ratios("feat", ours, r64, r32)
    assert rt.size == 3 * 6 and rt.max() > 1
    assert R.bound_ratios("mask", np.full(4, 1e-30), np.zeros(4), np.zeros(4)).max() == np.inf
    assert R.bound_ratios("mask", np.zeros(4), np.zeros(4), np.zeros(4)).max() == 0
