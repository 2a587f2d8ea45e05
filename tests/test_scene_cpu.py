"""CPU checks of the scene compositing (libenarf_scene.so's host side and the referee of the GPU tests): no GPU. The
referee (tests/scene_reference.py) is held to closed forms - the single-avatar compositing of rendering.composite_fine,
front over back for avatars apart in depth, mask = 1 - exp(-sum tau), the instance masses summing to the mask, symmetry
under a permutation of the avatars, the running maximum - and the host-side argument checks of ops.scene_composite and of
the C ABI are made without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import scene_cases as SC
import scene_reference as SR
from enarf_gan_amd import ops
from enarf_gan_amd._loader import EnarfHipError

TINY = 1e-12          # float64 sums of at most 512 terms of one sign pattern: far below this, relative to their magnitude


def _close(got, want, magnitude, what):
    assert np.all(np.abs(np.asarray(got) - np.asarray(want)) <= TINY * (np.asarray(magnitude) + 1e-300)), what


def test_one_avatar_is_composite_fine_on_the_running_maximum():
    from enarf_gan_amd.libraries.NeRF.rendering import composite_fine
    for kind in ("interleaved", "repeated", "inversion", "opaque_start", "zero_density"):
        for Nf in (2, 5, 64):
            d, s, c, _ = SC.planted_ray(kind, 1, Nf, np.random.RandomState(Nf))
            for scale in (1.0, 3.0):
                got = SR.ray(d, s, c, render_scale=scale)
                D = np.maximum.accumulate(d[0].astype(np.float64))
                t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
                col, mask, disp, w = composite_fine(t(s), t(c[0])[None], t(D)[None], scale)
                # every quantity is of order 1 or below; composite_fine's 1 - exp(-x) is good to 1e-16 absolute
                _close(got["color"], col[0].numpy(), 1.0, (kind, Nf, "colour"))
                _close(got["mask"], mask[0].numpy(), 1.0, (kind, Nf, "mask"))
                _close(got["disparity"], disp[0].numpy(), 1.0, (kind, Nf, "disparity"))
                _close(got["weight"][:Nf - 1], w[0].numpy(), 1.0, (kind, Nf, "weights"))
                assert got["weight"][Nf - 1] == 0 and np.array_equal(got["t"], D) and np.array_equal(got["source"], np.arange(Nf))
                _close(got["instance_mass"][0], got["mask"], 1.0, "one avatar carries the whole mask")
                assert got["instance"] == (0 if np.float32(got["mask"]) >= 0.5 else -1) and got["skipped"] == 0


def test_avatars_apart_in_depth_are_front_over_back():
    d, s, c = SC.two_apart()
    both = SR.ray(d, s, c)
    back, front = (SR.composite_fine64(s[k], c[k], d[k]) for k in (0, 1))
    _close(both["color"], front[0] + (1 - front[1]) * back[0], both["abs"]["color"], "colour")
    _close(both["mask"], front[1] + (1 - front[1]) * back[1], 1.0, "mask")
    _close(both["disparity"], front[2] + (1 - front[1]) * back[2], both["disparity"], "disparity")
    _close(both["instance_mass"], [(1 - front[1]) * back[1], front[1]], 1.0, "instance mass")
    Nf = d.shape[1]
    assert np.array_equal(both["source"], np.concatenate([Nf + np.arange(Nf), np.arange(Nf)]))
    assert both["instance"] == (1 if front[1] > (1 - front[1]) * back[1] else 0)
    # the planted disjoint rays of the shared cases: K avatars in a shuffled depth order
    for K, Nf in ((3, 5), (5, 13)):
        d, s, c, _ = SC.planted_ray("disjoint", K, Nf, np.random.RandomState(K))
        got = SR.ray(d, s, c)
        colour, trans, masses = np.zeros(3), 1.0, np.zeros(K)
        for k in np.argsort(d[:, 0]):
            one = SR.composite_fine64(s[k], c[k], d[k])
            colour, masses[k], trans = colour + trans * one[0], trans * one[1], trans * (1 - one[1])
        _close(got["color"], colour, got["abs"]["color"], (K, Nf))
        _close(got["instance_mass"], masses, 1.0, (K, Nf))
        _close(got["mask"], 1 - trans, 1.0, (K, Nf))


def test_mask_is_one_minus_the_transmittance_and_the_instance_masses_sum_to_it():
    for K, Nf, n, F in SC.SHAPES[:5]:
        depth, density, color, valid = SC.case(K, Nf, n, F)
        for f in range(F):
            for r in range(0, n, 3):
                got = SR.ray(depth[f, :, r], density[f, :, r], color[f, :, :, r], valid[f, :, r])
                if "total_tau" in got:
                    _close(got["mask"], -np.expm1(-got["total_tau"]), 1.0, (K, Nf, f, r))
                _close(got["instance_mass"].sum(), got["mask"], 1.0, (K, Nf, f, r))
                assert (got["instance_mass"] >= 0).all() and 0 <= got["mask"] <= 1 + TINY


def test_a_permutation_of_the_avatars_permutes_the_masses_and_keeps_the_ray():
    """bound: one fp32 step at the sum of absolute terms, the GPU tests' bound (the float64 sums differ by far less; ties
    between avatars are broken by the avatar index, which moves breakpoints of equal depth but no value)"""
    for kind in ("interleaved", "tied_lists", "repeated", "one_invalid", "nan_depth"):
        K, Nf = 4, 13
        d, s, c, v = SC.planted_ray(kind, K, Nf, np.random.RandomState(5))
        perm = np.array([2, 0, 3, 1])
        a, b = SR.ray(d, s, c, v), SR.ray(d[perm], s[perm], c[perm], v[perm])
        for k in ("color", "mask", "disparity"):
            assert np.all(np.abs(a[k] - b[k]) <= SR.step32(a["abs"][k])), (kind, k)
        assert np.all(np.abs(a["instance_mass"][perm] - b["instance_mass"]) <= SR.step32(a["abs"]["instance_mass"][perm])), kind
        assert b["skipped"] == sum(((a["skipped"] >> int(k)) & 1) << i for i, k in enumerate(perm))
        assert np.array_equal(a["t"], b["t"])


def test_a_last_ulp_inversion_gives_the_result_of_its_running_maximum():
    d, s, c, v = SC.planted_ray("inversion", 3, 5, np.random.RandomState(9))
    assert (np.diff(d, axis=-1) < 0).any()
    a, b = SR.ray(d, s, c, v), SR.ray(np.maximum.accumulate(d, axis=-1), s, c, v)
    for k in ("t", "source", "weight", "color", "mask", "disparity", "instance_mass"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["weight"] >= 0).all()


def test_what_takes_no_part():
    K, Nf = 3, 5
    for kind, bit in SC.SKIPPED_BIT.items():
        d, s, c, v = SC.planted_ray(kind, K, Nf, np.random.RandomState(2))
        got = SR.ray(d, s, c, v)
        assert got["skipped"] == bit(K) and np.isinf(got["t"][(K - 1) * Nf:]).all() and np.isfinite(got["t"][:(K - 1) * Nf]).all()
        keep = [k for k in range(K) if not (bit(K) >> k) & 1]
        rest = SR.ray(d[keep], s[keep], c[keep])
        assert np.array_equal(got["color"], rest["color"]) and np.array_equal(got["instance_mass"][keep], rest["instance_mass"])
        v2 = v.copy()
        v2[int(np.log2(bit(K)))] = 0                               # the validity byte comes first: no bit then
        assert SR.ray(d, s, c, v2)["skipped"] == 0
    for kind in ("all_invalid", "dropped"):
        d, s, c, v = SC.planted_ray(kind, K, Nf, np.random.RandomState(2))
        got = SR.ray(d, s, c, v)
        assert got["skipped"] == 0 and got["instance"] == -1 and got["mask"] == 0 and not got["color"].any()
        assert (got["source"] == -1).all() and np.isinf(got["t"]).all() and not got["weight"].any()
    d, s, c, v = SC.planted_ray("opaque_start", K, Nf, np.random.RandomState(2))
    got = SR.ray(d, s, c, v)
    assert got["weight"][0] == 1.0 and not got["weight"][1:].any() and got["mask"] == 1.0
    whole = SR.composite(*SC.case(3, 5, 67, 1))
    assert whole["color"].shape == (1, 3, 67) and whole["instance_mass"].shape == (1, 3, 67) and whole["t"].shape == (1, 67, 15)
    one = SR.ray(*(a[0][..., 4, :] if a.ndim > 3 else a[0][:, 4] for a in SC.case(3, 5, 67, 1)))
    assert np.array_equal(whole["color"][0, :, 4], one["color"]) and whole["skipped"][0, 4] == one["skipped"]


def test_host_side_rejections():
    """every error of the binding is raised from shapes, dtypes and values alone, before any library call; what passes
    them on CPU tensors meets 'no CPU fallback'"""
    d, s, c, v = torch.ones(2, 3, 4, 5), torch.ones(2, 3, 4, 5), torch.ones(2, 3, 3, 4, 5), torch.ones(2, 3, 4, dtype=torch.uint8)
    bad = [dict(depth=d.double()), dict(density=s.half()), dict(color=c.double()), dict(depth=d.numpy()), dict(valid=v.float()),
           dict(valid=v.numpy()), dict(density=torch.ones(2, 3, 4, 6)), dict(color=torch.ones(2, 3, 4, 5)),
           dict(color=torch.ones(2, 3, 3, 5, 4)), dict(valid=torch.ones(2, 4, 3, dtype=torch.uint8)), dict(depth=torch.ones(4, 5)),
           dict(depth=torch.ones(1, 2, 3, 4, 5)), dict(want=()), dict(want=("color", "depth")), dict(want=3),
           dict(render_scale="wide"), dict(threshold=None), dict(out={"t": torch.zeros(2, 4, 15)}),
           dict(out={"mask": torch.zeros(2, 5)}), dict(out={"instance": torch.zeros(2, 4)}),
           dict(out={"mask": torch.zeros(2, 8)[:, ::2]})]
    for b in bad:
        with pytest.raises(ValueError):
            ops.scene_composite(**{**dict(depth=d, density=s, color=c, valid=v), **b})
    with pytest.raises(ValueError, match=r"2\^31"):
        big = torch.ones(1, 1, 1, 1)
        ops.scene_composite(big.expand(2 ** 15, 2, 2 ** 16, 2), big.expand(2 ** 15, 2, 2 ** 16, 2), big[None].expand(2 ** 15, 2, 3, 2 ** 16, 2))
    limits = [(9, 4), (0, 4), (2, 1), (2, 129), (8, 65), (5, 128)]
    for K, Nf in limits:
        with pytest.raises(NotImplementedError, match="avatars|samples"):
            ops.scene_composite(torch.ones(1, K, 2, Nf), torch.ones(1, K, 2, Nf), torch.ones(1, K, 3, 2, Nf))
    for name in ("depth", "density", "color"):
        with pytest.raises(NotImplementedError, match="gradient"):
            ops.scene_composite(**{**dict(depth=d, density=s, color=c), name: dict(depth=d, density=s, color=c)[name].clone().requires_grad_()})
    for ok in (dict(), dict(valid=None), dict(depth=d[0], density=s[0], color=c[0], valid=v[0]), dict(want=("t", "source")),
               dict(depth=torch.ones(1, 8, 2, 64), density=torch.ones(1, 8, 2, 64), color=torch.ones(1, 8, 3, 2, 64), valid=None)):
        with pytest.raises(EnarfHipError, match="no CPU fallback"):
            ops.scene_composite(**{**dict(depth=d, density=s, color=c, valid=v), **ok})
    assert ops.SceneComposite._fields == ("color", "mask", "disparity", "instance_mass", "instance", "skipped", "t", "source", "weight")


def test_the_c_abi_refuses_sizes_and_null_pointers_before_any_launch():
    """ENARF_ERR_UNSUPPORTED for the limits, ENARF_ERR_ARG for the rest, from the host checks alone: no device is needed
    to be refused, and F n = 0 returns 0 without a launch"""
    from enarf_gan_amd import _scene_lib
    lib = _scene_lib.load()

    def args(**kw):
        a = _scene_lib.CompositeArgs()
        a.F, a.K, a.n, a.Nf, a.render_scale, a.threshold = 1, 2, 4, 8, 1.0, 0.5
        a.depth = a.density = a.color = a.out_mask = 64              # never dereferenced: every case below ends on the host
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw in (dict(K=0), dict(K=9), dict(Nf=1), dict(Nf=129), dict(K=8, Nf=65), dict(K=5, Nf=128)):
        assert lib.enarf_scene_composite(C.byref(args(**kw)), None) == -2, kw
        assert b"enarf_scene_composite" in lib.enarf_scene_last_error()
    for kw in (dict(F=-1), dict(n=-1), dict(F=2 ** 15, n=2 ** 16), dict(depth=None), dict(density=None), dict(color=None),
               dict(out_mask=None)):
        assert lib.enarf_scene_composite(C.byref(args(**kw)), None) == -1, kw
    assert lib.enarf_scene_composite(None, None) == -1
    for kw in (dict(F=0), dict(n=0), dict(F=0, depth=None)):
        assert lib.enarf_scene_composite(C.byref(args(**kw)), None) == 0, kw
    with pytest.raises(NotImplementedError, match="avatars"):
        _scene_lib.check(lib.enarf_scene_composite(C.byref(args(K=9)), None), "enarf_scene_composite")
    assert (_scene_lib.MAX_AVATARS, _scene_lib.MAX_SAMPLES, _scene_lib.MAX_MERGED) == (8, 128, 512)
