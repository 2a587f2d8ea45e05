"""CPU checks of the scene composite's backward (libenarf_sgrad.so's host side and the referee of the GPU tests): no GPU.
The referee (tests/sgrad_reference.py) is held to float64 torch autograd through a restatement of the forward in its
smooth form (colour = sum_j u_j sum_k s_k c_k with u_j = w_j / sigma_j taking its limit T_j a_j where sigma_j = 0), on the
shared cases of tests/scene_cases.py with every planted ray, and for one avatar to autograd through the march's own
compositing formula; the exact zeros of the contract and the host-side argument checks are made without a device.

The bound of both comparisons is 1e-10 of the entry's magnitude (the referee's sum of absolute terms): both sides are
fp64 and differ only in the order of their sums, a few thousand roundings of 1.1e-16 at most."""
import functools

import numpy as np
import pytest
import torch

import scene_cases as SC
import scene_reference as SR
import sgrad_reference as GR
from enarf_gan_amd import ops

BOUND = 1e-10
CPU_SHAPES = tuple(s for s in SC.SHAPES if s[0] * s[1] <= 65)            # up to (5, 13, 67, 2)


# ------------------------------------------------------------------------------- the forward, smooth form, in torch
def smooth_ray(depth, density, color, valid, render_scale):
    """one ray of the contract of include/enarf_scene.h in its smooth form: depth (K, Nf) numpy (a constant), density
    (K, Nf) and color (K, 3, Nf) float64 torch tensors holding the stored fp32 values, valid (K,) or None -> (colour
    (3,), mask, disparity, instance_mass (K,)), differentiable with respect to density and color"""
    K, Nf = depth.shape
    scale = float(np.float32(render_scale))
    s_np, c_np = density.detach().numpy(), color.detach().numpy()
    part = [k for k in range(K) if SR.takes_part(depth[k], s_np[k], c_np[k], 1 if valid is None else int(valid[k]))[0]]
    zero = density.new_zeros(())
    if not part:
        return density.new_zeros(3), zero, zero, density.new_zeros(K)
    key_d = np.concatenate([np.maximum.accumulate(depth[k].astype(np.float64)) for k in part])
    key_k, key_i = np.repeat(part, Nf), np.tile(np.arange(Nf), len(part))
    order = np.lexsort((key_i, key_k, key_d))
    t, who = torch.from_numpy(key_d[order]), key_k[order]
    M = len(order)
    s_act, sc_act = [density.new_zeros(M)] * K, [density.new_zeros(3, M)] * K
    for k in part:
        active = np.cumsum(who == k) - 1
        has = torch.from_numpy(((active >= 0) & (active <= Nf - 2)).astype(np.float64))
        idx = torch.from_numpy(np.clip(active, 0, Nf - 2))
        s_act[k] = density[k][idx] * has
        sc_act[k] = s_act[k] * color[k][:, idx]
    s_act, sc = torch.stack(s_act), torch.stack(sc_act).sum(0)
    sigma = s_act.sum(0)
    a = torch.cat([(t[1:] - t[:-1]) * scale, t.new_zeros(1)])
    tau = sigma * a
    T = torch.exp(-(torch.cumsum(tau, 0) - tau))
    dense = sigma > 0
    u = torch.where(dense, T * -torch.expm1(-tau) / torch.where(dense, sigma, torch.ones_like(sigma)), T * a)
    live = torch.cat([t.new_ones(M - 1), t.new_zeros(1)])                # the last breakpoint starts no segment
    u = u * live
    return (u * sc).sum(-1), (u * sigma).sum(), (u * sigma / t).sum(), (u * s_act).sum(-1)


def smooth_loss(depth, density, color, valid, render_scale, g_color, g_mask, g_disparity, g_instance_mass):
    """L = g_C . colour + g_M mask + g_D disparity + sum_k g_I[k] instance_mass[k], summed over the rays of a call: depth
    (F, K, n, Nf) numpy, density and color float64 torch tensors in the library's layouts, the upstream gradients numpy
    or None (zeros)"""
    F, K, n, Nf = depth.shape
    up = lambda g, *at: None if g is None else torch.from_numpy(np.asarray(g[at], np.float64))
    total = density.new_zeros(())
    for f in range(F):
        for r in range(n):
            col, mask, disp, mass = smooth_ray(depth[f, :, r], density[f, :, r], color[f, :, :, r],
                                               None if valid is None else valid[f, :, r], render_scale)
            for g, x in ((up(g_color, f, slice(None), r), col), (up(g_mask, f, r), mask), (up(g_disparity, f, r), disp),
                         (up(g_instance_mass, f, slice(None), r), mass)):
                if g is not None:
                    total = total + (g * x).sum()
    return total


def _leaves(density, color):
    make = lambda a: torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)
    return make(density), make(color)


def _held(got, ref, magnitude, what):
    err = np.abs(np.asarray(got) - ref)
    worst = float((err / (magnitude + 1e-300)).max())
    print(f"{what}: worst entry {worst:.2e} of its magnitude")
    assert np.isfinite(ref).all() and np.all(err <= BOUND * magnitude), what


@functools.lru_cache(maxsize=None)
def _referee(K, Nf, n, F, scale):
    inputs = SC.case(K, Nf, n, F)
    return inputs, GR.upstream(F, K, n), GR.composite_bwd(*inputs, scale, *GR.upstream(F, K, n))


# ------------------------------------------------------------------------------------------------------ the referee
@pytest.mark.parametrize("K,Nf,n,F", CPU_SHAPES)
def test_referee_is_autograd_of_the_smooth_forward(K, Nf, n, F):
    scale = 0.37 if F == 2 else 1.0
    (depth, density, color, valid), up, ref = _referee(K, Nf, n, F, scale)
    s, c = _leaves(density, color)
    smooth_loss(depth, s, c, valid, scale, *up).backward()
    _held(s.grad.numpy(), ref["density"], ref["abs"]["density"], f"K {K} Nf {Nf} n {n} F {F}, density")
    _held(c.grad.numpy(), ref["color"], ref["abs"]["color"], f"K {K} Nf {Nf} n {n} F {F}, colour")
    assert np.abs(ref["density"]).max() > 0 and np.abs(ref["color"]).max() > 0


def test_smooth_forward_is_the_forward_referee():
    """the restatement the referee is held to computes what tests/scene_reference.py computes"""
    depth, density, color, valid = SC.case(3, 5, 67, 1)
    ref = SR.composite(depth, density, color, valid, render_scale=2.0)
    s, c = _leaves(density, color)
    with torch.no_grad():
        for r in range(67):
            col, mask, disp, mass = smooth_ray(depth[0, :, r], s[0, :, r], c[0, :, :, r], valid[0, :, r], 2.0)
            for got, k in ((col, "color"), (mass, "instance_mass")):
                assert np.all(np.abs(got.numpy() - ref[k][0, :, r]) <= 1e-12 * (ref["abs"][k][0, :, r] + 1e-300)), (r, k)
            for got, k in ((mask, "mask"), (disp, "disparity")):
                assert abs(float(got) - ref[k][0, r]) <= 1e-12 * ref["abs"][k][0, r], (r, k)


def test_one_avatar_is_autograd_of_the_march_compositing():
    """K = 1 with strictly ascending depths: the referee equals float64 autograd through the formula of
    scene_reference.composite_fine64 (the march's own compositing), restated in torch"""
    for Nf, scale in ((2, 1.0), (5, 0.37), (64, 1.0)):
        rs = np.random.RandomState(Nf)
        d = (2.0 + np.cumsum(rs.uniform(0.01, 0.1, size=(1, Nf)), -1)).astype(np.float32)
        s = np.exp(rs.uniform(-3.0, 3.0, size=(1, Nf))).astype(np.float32)
        s[0, rs.uniform(size=Nf) < 0.2] = 0.0
        c = rs.uniform(-1.0, 1.0, size=(1, 3, Nf)).astype(np.float32)
        gC, gM, gD, gI = (x[0, ..., 0].astype(np.float64) for x in GR.upstream(1, 1, 1, seed=Nf))
        gd, gc, md, mc = GR.ray(d, s, c, None, scale, gC, float(gM), float(gD), gI)
        st, ct = _leaves(s[0], c[0])
        dt = torch.from_numpy(d[0].astype(np.float64))
        dd = st[:-1] * (dt[1:] - dt[:-1]) * float(np.float32(scale))
        w = torch.exp(-(torch.cumsum(dd, 0) - dd)) * (1 - torch.exp(-dd))
        colour, mask, disparity = (w * ct[:, :-1]).sum(-1), w.sum(), (w / dt[:-1]).sum()
        ((torch.from_numpy(gC) * colour).sum() + float(gM) * mask + float(gD) * disparity + float(gI[0]) * mask).backward()
        _held(st.grad.numpy(), gd[0], md[0], f"Nf {Nf}, density")
        _held(ct.grad.numpy(), gc[0], mc[0], f"Nf {Nf}, colour")


def test_exact_zeros():
    """avatars with a validity byte of 0, screened avatars and every last sample get exact zeros, and so does every
    entry's magnitude there"""
    for K, Nf, n, F in ((3, 5, 67, 1), (5, 13, 67, 2)):
        (depth, density, color, valid), _, ref = _referee(K, Nf, n, F, 0.37 if F == 2 else 1.0)
        for name in ("density", "color"):
            assert not ref[name][..., Nf - 1].any() and not ref["abs"][name][..., Nf - 1].any()
        seen = set()
        for f in range(F):
            for r in range(n):
                kind = SC.kind_of(r, f, n)
                out = [k for k in range(K) if valid[f, k, r] == 0]
                if kind in SC.SKIPPED_BIT:
                    out += [k for k in range(K) if SC.SKIPPED_BIT[kind](K) >> k & 1]
                    seen.add(kind)
                for k in out:
                    assert not ref["density"][f, k, r].any() and not ref["color"][f, k, :, r].any(), (f, r, kind, k)
                if kind in ("all_invalid", "dropped"):
                    assert not ref["density"][f, :, r].any() and not ref["color"][f, :, :, r].any()
                if kind == "interleaved":
                    assert ref["density"][f, :, r, :Nf - 1].all()
        assert seen == set(SC.SKIPPED_BIT)


# ------------------------------------------------------------------------------------------- arguments, no device
def _args(K=2, Nf=4, n=3, F=2):
    return torch.zeros(F, K, n, Nf), torch.zeros(F, K, n, Nf), torch.zeros(F, K, 3, n, Nf), torch.ones(F, K, n, dtype=torch.uint8)


def test_argument_checker_takes_no_device():
    from enarf_gan_amd._sgrad_lib import check_composite_bwd_args as check
    d, s, c, v = _args()
    gC, gM, gD, gI = torch.zeros(2, 3, 3), torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 2, 3)
    assert check(d, s, c, v, gC, gM, gD, gI, ("density", "color")) == (2, 2, 3, 4, True)
    assert check(d[0], s[0], c[0], None, None, gM[0], None, None, ("color",)) == (1, 2, 3, 4, False)
    for only in range(4):                                              # missing upstream gradients are accepted
        up = [g if i == only else None for i, g in enumerate((gC, gM, gD, gI))]
        assert check(d, s, c, v, *up, ("density",))[0] == 2
    assert check(*_args(8, 64, 0, 1), None, torch.zeros(1, 0), None, None, ("density",)) == (1, 8, 0, 64, True)
    with pytest.raises(ValueError, match="no upstream gradient"):
        check(d, s, c, v, None, None, None, None, ("density",))
    for want in ((), ("mask",), ("density", "weight"), 3):
        with pytest.raises(ValueError, match="want"):
            check(d, s, c, v, gC, gM, gD, gI, want)
    for bad in ((d.double(), s, c, v, gC, gM, gD, gI), (d, s[:, :1], c, v, gC, gM, gD, gI), (d, s, c[:, :, :2], v, gC, gM, gD, gI),
                (d, s, c, v.float(), gC, gM, gD, gI), (d, s, c, v[:1], gC, gM, gD, gI), (d, s, c, v, gC[:, :2], gM, gD, gI),
                (d, s, c, v, gC, gM[0], gD, gI), (d, s, c, v, gC, gM, gD.double(), gI), (d, s, c, v, gC, gM, gD, gI[:, :1]),
                (d[0, 0], s[0, 0], c[0, 0], None, gC, gM, gD, gI), (d.numpy(), s, c, v, gC, gM, gD, gI)):
        with pytest.raises(ValueError):
            check(*bad, ("density",))
    for K, Nf in ((9, 4), (2, 129), (8, 65), (1, 1)):
        with pytest.raises(NotImplementedError):
            check(*_args(K, Nf, 1, 1), None, torch.zeros(1, 1), None, None, ("density",))


def test_host_layers_reject_before_any_device():
    d, s, c, v = _args()
    with pytest.raises(ValueError, match="no upstream gradient"):
        ops.scene_composite_bwd(d, s, c, v)
    with pytest.raises(ValueError, match="want"):
        ops.scene_composite_bwd(d, s, c, v, g_mask=torch.zeros(2, 3), want=())
    with pytest.raises(NotImplementedError, match="depth"):
        ops.scene_composite_posable(d.clone().requires_grad_(True), s, c, v)
    with pytest.raises(NotImplementedError, match="gradient"):        # the forward alone keeps refusing
        ops.scene_composite(d, s.clone().requires_grad_(True), c, v)


def test_c_abi_rejects_on_the_host():
    """the entry point's own checks, made before any launch: no device is needed to be turned away"""
    import ctypes as C
    from enarf_gan_amd import _sgrad_lib as G
    lib = G.load()
    one = C.c_void_p(256)                                              # never dereferenced: every call below is rejected

    def call(**kw):
        a = G.CompositeBwdArgs()
        a.F, a.K, a.n, a.Nf, a.render_scale = 1, 2, 4, 8, 1.0
        a.depth = a.density = a.color = a.g_mask = a.g_density = one
        for k, x in kw.items():
            setattr(a, k, x)
        return lib.enarf_sgrad_composite_bwd(C.byref(a), None)

    assert lib.enarf_sgrad_composite_bwd(None, None) == -1
    for kw, code in ((dict(K=0), -2), (dict(K=9), -2), (dict(Nf=1), -2), (dict(Nf=129), -2), (dict(K=8, Nf=65), -2),
                     (dict(F=-1), -1), (dict(F=2 ** 16, n=2 ** 15), -1), (dict(g_mask=None), -1), (dict(g_density=None), -1),
                     (dict(depth=None), -1)):
        assert call(**kw) == code, kw
        assert lib.enarf_sgrad_last_error()
    assert call(n=0) == 0 and call(F=0) == 0                           # nothing to launch
