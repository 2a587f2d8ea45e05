"""What the per-entry forward bound of tests/fwd_referee.py accepts and rejects, on the CPU with the oracle alone: fp32
renders outside the bound's yardstick pass against the float64 referee on all eight tensors; four corruptions of the fp32
oracle's result, each of which passes the max-normalised 1e-4 bound of the older forward tests (_helpers.assert_close) on
everything those tests compare, fail it. Plus the conditions every case of the GPU matrix (tests/fwd_cases.py) must meet."""
import numpy as np
import pytest
import torch

import fwd_cases as FC
import fwd_referee as FR
import grad_referee as R
from _helpers import rel_err
from oracle import enarf_oracle as O

OLD = {k: 1e-4 for k in FR.NAMES if k != "fine_color"}     # what the older forward tests hold, of each tensor's maximum
OLD["fine_depth"] = 1e-6                                   # (the per-sample colour they compare with nothing)


@pytest.fixture(scope="module")
def band():
    """8 rays of the first row + 40 through the body of a 32^2 frame, Nc 32, Nf 33, sorted random bins (case nf33)"""
    c = FC.build("nf33")
    ref = FR.referee(c["sc"], c["coord"], c["Nc"], c["Nf"], c["bins"], amplitudes=(1, FR.F16X3_ULPS))
    rays = ref["keep"] & ref["live"]
    assert rays.sum() >= 16 and ref["keep"].all()
    return dict(ref, c=c, rays=rays)


@pytest.fixture(scope="module")
def thin_band():
    """the band's rays at render_scale 0.15: the transmittance behind the last interval, 1e-45 .. 1e-8 on the band (its rays
    are opaque), is 1e-7 .. 1e-1 here, so that a sample composited after it weighs something, and on some rays little"""
    c = dict(FC.build("nf33"), render_scale=0.15)
    ref = FR.referee(c["sc"], c["coord"], c["Nc"], c["Nf"], c["bins"], render_scale=c["render_scale"])
    return dict(ref, c=c, rays=ref["keep"] & ref["live"])


def _old_bound_passes(t, band):
    """the older tests' check of every tensor they compare, on the compared rays, against float64"""
    for k, tol in OLD.items():
        e = rel_err(t[k][band["rays"]], band["t64"][k][band["rays"]])
        assert e.max() <= tol, (k, e.max())


def _ratios(t, band, k, ulps=1):
    rt = FR.bound_ratios(k, t[k], band["t64"][k], [band["t32"][k]] + [d[k] for d in band["draws"][ulps]], band["rays"],
                         extra=FR.exp_term(k, band["t64"][k]))
    return rt[band["rays"]]


def _recomposite(band, density=None, color=None, samples=None):
    """the fp32 oracle's compositing again on its own (or corrupted) per-sample results -> tensors(); `samples` = Nf
    composites over all Nf samples, the interval of the last one taken as long as the one before it"""
    p = band["taps32"]
    den = p["fine_density"] if density is None else density
    col = p["fine_color"] if color is None else color
    dep = p["fine_depth"]
    if samples is not None:
        den = torch.cat([den, den[..., -1:]], -1)
        col = torch.cat([col, col[..., -1:]], -1)
        dep = torch.cat([dep, dep[..., -1:] + (dep[..., -1:] - dep[..., -2:-1])], -1)
    rc, rm, rd, w = O.composite(den, col, dep, band["c"]["render_scale"])
    t = FR.tensors(rc, rm, rd, p["coarse_density"], den[..., :p["fine_density"].shape[-1]], col[..., :p["fine_color"].shape[-1]],
                   p["fine_depth"], w[..., :p["fine_weights"].shape[-1]])
    return t


def test_recomposite_reproduces_the_oracle(band):
    t = _recomposite(band)
    for k in FR.NAMES:
        assert np.array_equal(t[k][band["rays"]], band["t32"][k][band["rays"]]), k


def test_held_out_fp32_draws_pass(band):
    """fp32 renders on inputs moved with other seeds than the yardstick's draws - every bin by -1, 0 or +1 ulp at random -
    stay within the bound on every entry of all eight tensors, for both yardsticks"""
    c = band["c"]
    for ulps in (1, FR.F16X3_ULPS):
        for j in (50, 51, 52, 53):
            t, d = FR.draw(c["sc"], c["coord"], c["Nc"], c["Nf"], c["bins"], j, ulps)
            rays = band["rays"] & ~R.disagreeing_rays(d, band["dec32"])
            assert rays.sum() >= 16
            worst = FR.check_forward(t, band, f"held-out fp32 draw {j}, {ulps} ulp", ulps=ulps, rays=rays)
            assert len(worst) == 8
            print(f"held-out draw {j}, {ulps} ulp: {FR.fmt(worst)}")


@pytest.mark.parametrize("below,old", [(1e-4, 1e-4), (1e-3, 1.01e-3)])
def test_bound_rejects_small_fine_weights_set_to_zero(band, below, old):
    """The exported fine weights with every entry below 1e-4 of the maximum set to zero pass the old 1e-4 bound by
    construction; below 1e-3 of the maximum - two thirds of the entries - they come to 1e-3 of the maximum, which the old
    bound still lets through wherever an entry lies below 1e-4. The per-entry bound rejects both."""
    t = {k: v.copy() for k, v in band["t32"].items()}
    w = t["fine_weights"]
    top = np.abs(w[band["rays"]]).max()
    small = (np.abs(w) < below * top) & (w != 0)
    w[small] = 0
    e = rel_err(w[band["rays"]], band["t64"]["fine_weights"][band["rays"]]).max()
    assert e <= old, e
    rt = _ratios(t, band, "fine_weights")
    print(f"fine weights below {below} of the maximum zeroed: {int(small[band['rays']].sum())} entries, old measure {e:.2e}, "
          f"{int((rt > 1).sum())} above the bound, worst {rt.max():.3g}")
    assert (rt > 1).sum() >= 100 and rt.max() > 100, ((rt > 1).sum(), rt.max())


def _one_sample_per_ray(band, score, limit):
    """per compared ray, the fine sample (not the last) with the largest `score` (B,n,Nf-1) not above `limit`; (b, ray, e)"""
    out = []
    for b, r in zip(*np.nonzero(band["rays"])):
        s = np.where((score[b, r] <= limit) & (score[b, r] > 0), score[b, r], -1.0)
        if s.max() > 0:
            out.append((b, r, int(np.argmax(s))))
    return out


def test_bound_rejects_one_density_per_ray_off_by_a_thousandth(band):
    """one fine sample per ray with its density scaled by 0.999, composited again; the sample is one below a twentieth of the
    largest density and with density x interval <= 0.05 (every weight behind it moves by 1e-3 of that), so that the old bound
    passes on every tensor"""
    d32, z32 = band["t32"]["fine_density"], band["t32"]["fine_depth"]
    thin = d32 * (z32[..., 1:] - z32[..., :-1]) <= 0.05
    pick = _one_sample_per_ray(band, np.where(thin, d32, 0.0), 0.05 * d32[band["rays"]].max())
    assert len(pick) >= 16
    den = band["taps32"]["fine_density"].clone()
    for b, r, e in pick:
        den[b, r, e] *= 0.999
    t = _recomposite(band, density=den)
    _old_bound_passes(t, band)
    rt = _ratios(t, band, "fine_density")
    print(f"density x 0.999 on {len(pick)} samples: {int((rt > 1).sum())} above the bound, worst {rt.max():.3g}")
    assert (rt > 1).sum() >= len(pick) - 2 and rt.max() > 10, ((rt > 1).sum(), rt.max())


def test_bound_rejects_one_colour_per_ray_off_by_a_thousandth(band):
    """the colour of one fine sample per ray off by 1e-3 (a sample that weighs at most 0.05, so that the composited pixel
    moves by less than the old bound sees; the per-sample colour itself no older test reads), composited again"""
    w32 = band["t32"]["fine_weights"]
    pick = _one_sample_per_ray(band, w32, 0.05)
    assert len(pick) >= 16
    col = band["taps32"]["fine_color"].clone()
    for b, r, e in pick:
        col[b, :, r, e] += 1e-3
    t = _recomposite(band, color=col)
    _old_bound_passes(t, band)
    rt = _ratios(t, band, "fine_color")
    print(f"colour + 1e-3 on {len(pick)} samples: {int((rt > 1).sum())} above the bound, worst {rt.max():.3g}")
    assert (rt > 1).sum() >= len(pick) and rt.max() > 10, ((rt > 1).sum(), rt.max())


def test_bound_rejects_a_composite_over_all_nf_samples(thin_band):
    """the last fine sample only closes the last interval (rendering.py:307-335); composited as a sample of its own it adds
    its weight to the pixel, the mask and the disparity. On the rays where that weight is at most 5e-5 - the tail of an
    opaque ray - the old bound passes."""
    band = thin_band
    full = _recomposite(band, samples=band["c"]["Nf"])
    extra = full["mask"] - band["t32"]["mask"]
    sel = band["rays"] & (extra > 0) & (extra <= 5e-5)
    assert sel.sum() >= 3, sel.sum()
    t = {k: v.copy() for k, v in band["t32"].items()}
    for k in ("color", "mask", "disparity"):
        t[k][sel] = full[k][sel]
    _old_bound_passes(t, band)
    bad = {k: _ratios(t, band, k) for k in ("color", "mask", "disparity")}
    print("composite over Nf samples: " + ", ".join(f"{k}: {int((v > 1).sum())} above, worst {v.max():.3g}" for k, v in bad.items()))
    print(f"  on {int(sel.sum())} rays, the extra weights {np.sort(extra[sel])}")
    # (the pixel's colour moves by that weight x a colour of ~0.05, which stays inside its bound: it is the mask and the
    # disparity that show the sample)
    assert (bad["mask"] > 1).sum() >= 3 and (bad["disparity"] > 1).sum() >= 3, bad


def test_bound_groups_and_edges():
    """A sample's three colour channels form one group, every other entry is its own; an entry the referee holds at zero
    must be zero up to the floor; a tensor the referee holds at zero everywhere must be zero exactly."""
    r64 = np.zeros((1, 2, 3, 3))
    r64[0, 1, 2, 0] = 1.0
    ours = r64.copy()
    ours[0, 1, 2, 1] = 1e-6                                      # same sample as the 1.0: within RTOL of the group
    rt = FR.bound_ratios("fine_color", ours, r64, [r64])
    assert rt.shape == (1, 2, 3) and rt.max() <= 1
    assert FR.bound_ratios("fine_density", ours, r64, [r64]).max() > 1     # alone, the same entry is above the floor
    ours[0, 0, 0, 1] = 1e-6                                      # a sample the referee holds at zero: above FLOOR
    assert FR.bound_ratios("fine_color", ours, r64, [r64]).max() > 1
    assert FR.bound_ratios("mask", np.full(4, 1e-30), np.zeros(4), [np.zeros(4)]).max() == np.inf
    assert FR.bound_ratios("mask", np.zeros(4), np.zeros(4), [np.zeros(4)]).max() == 0
    rt = FR.bound_ratios("mask", np.array([1.0, 1e-12]), np.array([1.0, 0.0]), [np.array([1.0, 0.0])])
    assert rt[0] == 0 and 0 < rt[1] <= 1                        # zero where it equals the referee; below the floor of 1e-9


def test_yardstick_bins_span_one_ulp():
    """the first four draws move every bin by exactly one ulp: up, down and the two alternations; later ones at random"""
    bins = torch.rand(1, 3, 8, generator=torch.Generator().manual_seed(0)).sort(-1).values + 0.01
    moved = [FR.moved_bins(bins, i) for i in range(6)]
    for m in moved:                                             # x (1 +- 2^-23), rounded: one or two neighbours away at most
        assert float(((m - bins).abs() / bins).max()) <= 2 ** -22
    assert bool((moved[0] > bins).all()) and bool((moved[1] < bins).all())
    assert bool((moved[2][..., 0::2] > bins[..., 0::2]).all()) and bool((moved[2][..., 1::2] < bins[..., 1::2]).all())
    assert bool((moved[3][..., 0::2] < bins[..., 0::2]).all()) and bool((moved[3][..., 1::2] > bins[..., 1::2]).all())
    assert not torch.equal(moved[4], moved[5])


@pytest.mark.parametrize("name", list(FC.CASES))
def test_case_table_conditions(name):
    """every case of the GPU matrix, from its float64 and fp32 renders alone: at least 90 % of its rays are kept, at least 16
    kept rays are valid, at least one ray misses every cube"""
    c = FC.build(name)
    ref = FR.referee(c["sc"], c["coord"], c["Nc"], c["Nf"], c["bins"], render_scale=c["render_scale"], draws=0, **c["modes"])
    rv = ref["dec32"]["ray_valid"]
    assert ref["keep"].mean() >= 0.9 and (ref["keep"] & rv).sum() >= 16 and (~rv).any(), (ref["keep"].mean(), (ref["keep"] & rv).sum())
    if name == "opaque":                     # the weights underflow behind the first samples: fp32 holds zeros where float64 does not
        w64, w32 = ref["t64"]["fine_weights"][ref["keep"] & rv], ref["t32"]["fine_weights"][ref["keep"] & rv]
        assert ((w32 == 0) & (w64 > 0)).sum() >= 100 and (ref["t64"]["mask"][ref["keep"] & rv] > 0.999).all()
