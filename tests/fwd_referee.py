"""A float64 referee for the forward march and a per-entry bound to hold a kernel's samples and rays to.

Referee: oracle.enarf_oracle.render on float64 copies of the fp32 inputs (grad_referee.render_forward, under no_grad), the
bins replayed. The same render in fp32 is the yardstick: its distance from float64 is what the reference's own arithmetic
costs on each entry. Compared: per sample the coarse and fine density, the fine colour, depth and weight (the debug taps and
the fine_weights / fine_depth outputs), per ray colour, mask and disparity.

Bound (`bound_ratios`). The older forward tests allow 1e-4 of each tensor's maximum. On the band of
tests/test_fwd_referee_cpu.py (32^2 frame, 8 rays of the first row + 40 through the body, Nc 32, Nf 33, sorted random bins)
the fp32 oracle itself is 1e-5 (densities), 5e-5 (fine colour), 1.5e-5 (fine weights), 5e-6 / 1e-6 / 1e-6 (colour, mask,
disparity) of the maximum away from float64, and 77 % of the fine weights lie below 1e-3 of the maximum. So every entry e is
held to its own scale:

    |ours(e) - f64(e)|  <=  A * max over fp32 renders |f32(e) - f64(e)|  +  RTOL * |f64(e)|  +  FLOOR * max|f64|
                            [+ EXP_ULP * T(e) for a fine weight]

per group - a sample's three colour channels, every other entry alone - as the max over the group of each term.
  * Yardstick: the fp32 oracle and DRAWS = 6 fp32 renders on inputs moved by up to one ulp (grad_referee.perturbed_scene /
    perturb: tri-plane, MLP parameters, z_rend; the bins: `moved_bins`). A = 8, as for the gradients.
  * Excluded by rule, never covered by tolerance: rays on which float64 or a draw takes another discrete decision than the
    fp32 oracle (grad_referee.decisions / disagreeing_rays); the last fine sample's density and colour (it only closes the
    last interval; production never queries it); the colour of a sample inside no part's cube (`check_forward`). Rays that
    are dropped (one image, no cube hit) are exact zeros in every output: asserted exactly by the GPU tests.
  * RTOL = 2^-19 (1.9e-6, 32 fp32 half-ulp), derived, not measured: the kernel's part probability is the product of three
    sigmoidf_(v) = rcp(1 + __expf(-v)) (csrc/enarf_device.h). __expf(-v) is v_exp_f32 of -v * log2(e): the rounded product
    moves the result by |v| * 2^-24, v_exp_f32 by 1 ulp (2 * 2^-24); the sum 1 + e rounds by 2^-24; v_rcp_f32 by 1 ulp
    (2 * 2^-24): (5 + |v|) * 2^-24 per sigmoid, 10 * 2^-24 at |v| = 5 (the clamp of clamp_mask; the synthetic planes stay
    below it), x 3 sigmoids + the 2 roundings of their product = 32 * 2^-24 - where the reference's sigmoid is good to an
    ulp. What the MLP makes of that error in its input, the A term scales: fp32 draws amplify their own errors the same way.
  * FLOOR = 1e-9 of the tensor's maximum (1/60 of an ulp of the maximum): fp32 holds no entry smaller than 1.2e-38 (the
    kernel flushes denormals), float64 holds the weights behind an opaque surface down to 1e-320.
  * EXP_ULP = 2^-24 for the fine weights, w = T * (1 - exp(-density * interval)): the exponential, in [0.5, 1) for every
    interval that matters here, is good to 1 ulp = 2^-24 in the kernel's expf as in the reference's exp, the subtraction
    is exact, so w moves by up to 2^-24 * T however small it is - 1e-3 of a weight of 6e-5 on a 3e-4-deep interval. The draws
    do not show it: each calls the same exp on almost the same argument and rounds the same way (seven identical values on
    such entries). Found on the GPU (no_selector, a transparent body: 1.26 x the bound without the term, the kernel's expf
    one ulp from the reference's exp); T(e) = 1 - the float64 weights in front of e, so the term vanishes in an opaque
    ray's tail. The sums over a ray (colour, mask, disparity) get no such term: they pass without it.
  * `f16x3` (the default MLP mode; DESIGN 3.1: "the fp16 pair carries 22 bits") is held to the same bound with another
    yardstick: the fp32 oracle and DRAWS renders whose tri-plane, MLP parameters and z_rend are moved by up to
    F16X3_ULPS = 4 fp32 ulp. Derivation: an operand split into two fp16 values has a 22-bit significand, its unit in the
    last place is 2^-21 of it = 2^(24 - 22) = 4 ulp of fp32's 24 bits; the features (tri-plane), the weights (MLP
    parameters, z_rend) and, through the next layer's weights, the activations are the operands that are split. The
    dropped fourth product of each 3-term split is 2^-24 of the product, below that. The bins move by one ulp as before:
    the mode does not touch them.

`moved_bins`. A sample's density and colour depend on its own bin alone, an interval's weight on its two ends, and one ulp of
a bin (5e-7 of depth) moves a density by up to 4e-4 - more than everything after it costs (the density's slope along the
ray reaches 1e3 per unit). With every bin moved by -1, 0 or +1 ulp at random, as the gradient referee does, six draws leave
8 % of the entries without a draw on one of the three sides, and held-out draws reached 3.1 x the bound (fine weights; 2.2
densities and colour) on the cases of the GPU matrix. So draws 0 - 3 move all bins up, all down, and alternately up / down
both ways; draws 4 and 5 stay random.

Calibration (the oracle alone, never a kernel): for each of the 19 cases of tests/fwd_cases.py (all their kept rays, none
excluded by the decisions), four held-out fp32 renders with other seeds and every bin moved at random, per amplitude.
Worst held-out error / bound per tensor over all cases, 1 ulp | 4 ulp (margin asked: <= 0.9):
    coarse_density 0.47 | 0.30   fine_density 0.37 | 0.36   fine_color 0.30 | 0.49   fine_depth 0.05 | 0.05
    fine_weights   0.41 | 0.43   color        0.36 | 0.60   mask       0.16 | 0.16   disparity  0.15 | 0.16
and per case, over the tensors: b2_style256 0.33 | 0.36, b3_center 0.20 | 0.26, clamp_mask 0.23 | 0.60, density_x_weight
0.22 | 0.31, nc33_nf17 0.25 | 0.36, nc72_nf128 0.23 | 0.34, nc72_nf65 0.27 | 0.49, nf17 0.18 | 0.29, nf2 0.21 | 0.21, nf33
0.24 | 0.36, nf64 0.28 | 0.44, no_selector 0.29 | 0.39, opaque 0.29 | 0.29, p24_style256 0.41 | 0.43, planes24x40 0.27 |
0.39, planes2x2 0.47 | 0.32, planes2x5 0.27 | 0.29, scale0.5 0.32 | 0.38, scale2 0.23 | 0.28. A = 4 would leave 0.95 .. 1.2.
What it accepts and rejects: tests/test_fwd_referee_cpu.py."""
import numpy as np
import torch

import grad_referee as R

A_YARDSTICK = 8.0
DRAWS = 6
RTOL = 2.0 ** -19
FLOOR = 1e-9
EXP_ULP = 2.0 ** -24      # one ulp of exp(-x) in [0.5, 1)
F16X3_ULPS = 4            # 2^(24 - 22): one unit in the last place of a 22-bit significand, in fp32 ulp

PER_SAMPLE = ("coarse_density", "fine_density", "fine_color", "fine_depth", "fine_weights")
PER_RAY = ("color", "mask", "disparity")
NAMES = PER_SAMPLE + PER_RAY
GROUPED = ("fine_color",)          # (.., 3): a sample's three channels are one group
MODE_ULPS = {"f32": 1, "f16x3": F16X3_ULPS}


def _np(x):
    return x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


def tensors(color, mask, disparity, coarse_density, fine_density, fine_color, fine_depth, fine_weights):
    """The eight compared tensors in one layout, float64 numpy, the ray axis second: per sample (B, n, samples) - fine_color
    (B, n, Nf - 1, 3) - and per ray (B, n) - color (B, n, 3). The last fine sample only closes the last interval: production
    never queries it, so it is left out of fine density and colour.
    In: color (B,3,n), mask / disparity (B,n), coarse_density (B,n,Nc), fine_density (B,n,Nf), fine_color (B,3,n,Nf),
    fine_depth (B,n,Nf), fine_weights (B,n,Nf-1)."""
    return {"coarse_density": _np(coarse_density), "fine_density": _np(fine_density)[..., :-1],
            "fine_color": _np(fine_color).transpose(0, 2, 3, 1)[:, :, :-1], "fine_depth": _np(fine_depth),
            "fine_weights": _np(fine_weights), "color": _np(color).transpose(0, 2, 1), "mask": _np(mask),
            "disparity": _np(disparity)}


def oracle_tensors(outs, taps):
    """tensors() of one oracle render: outs = (color, mask, disparity), taps = its taps"""
    return tensors(*outs, taps["coarse_density"], taps["fine_density"], taps["fine_color"], taps["fine_depth"], taps["fine_weights"])


def kernel_tensors(fwd):
    """tensors() of ops.render_fwd(..., debug=True)'s result"""
    t = fwd.taps
    return tensors(fwd.color, fwd.mask, fwd.disparity, t["coarse_density"], t["fine_density"], t["fine_color"],
                   fwd.fine_depth[:, 0], fwd.fine_weights[:, 0])


def moved_bins(bins, i):
    """Draw i's bins, every one moved by up to one ulp. A sample's density and colour depend on its own bin alone and an
    interval's weight on its two ends, and one ulp of a bin can move a density by more than everything after it (the
    density's slope along the ray reaches 1e3 per unit of depth), so the first four draws span that neighbourhood instead of
    leaving it to chance: all bins up, all down, and the two alternations (an interval stretched, and shrunk, by two ulp).
    Later draws (and every held-out draw of the calibration) move each bin by -1, 0 or +1 ulp at random."""
    if i >= 4:
        return R.perturb(bins, 1000 + i).sort(-1).values
    e = torch.arange(bins.shape[-1])
    s = (torch.ones(bins.shape[-1]), -torch.ones(bins.shape[-1]), 1.0 - 2.0 * (e % 2), 2.0 * (e % 2) - 1.0)[i]
    return (bins * (1 + s * 2 ** -23)).sort(-1).values


def draw(sc, coord, Nc, Nf, bins, i, ulps=1, tri=None, render_scale=1.0, **modes):
    """fp32 render number i on inputs moved by up to `ulps` ulp (tri-plane, MLP parameters, z_rend; the bins by up to one
    ulp whatever `ulps`: no arithmetic mode touches them) -> (tensors, decisions)"""
    with torch.no_grad():
        o, _, t = R.render_forward(R.perturbed_scene(sc, i, ulps), coord, Nc, Nf, moved_bins(bins, i), torch.float32,
                                   None if tri is None else R.perturb(tri, 2000 + i, ulps), render_scale, **modes)
    return oracle_tensors(o, t), R.decisions(t)


def referee(sc, coord, Nc, Nf, bins, tri=None, render_scale=1.0, amplitudes=(1,), draws=DRAWS, **modes):
    """The float64 referee, the fp32 oracle and, per amplitude (in ulp), `draws` fp32 renders on moved inputs; no autograd.
    Returns dict(t64, t32, draws {ulps: [tensors]}, keep (B,n) bool numpy: rays on which no render takes another discrete
    decision than the fp32 oracle, live (B,n): rays that are marched, taps32, dec32: the fp32 oracle's decisions)."""
    with torch.no_grad():
        o64, _, p64 = R.render_forward(sc, coord, Nc, Nf, bins, torch.float64, tri, render_scale, **modes)
        o32, _, p32 = R.render_forward(sc, coord, Nc, Nf, bins, torch.float32, tri, render_scale, **modes)
    d32 = R.decisions(p32)
    keep = ~R.disagreeing_rays(R.decisions(p64), d32)
    out = {}
    for u in amplitudes:
        out[u] = []
        for i in range(draws):
            t, d = draw(sc, coord, Nc, Nf, bins, i, u, tri, render_scale, **modes)
            keep &= ~R.disagreeing_rays(d, d32)
            out[u].append(t)
    return dict(t64=oracle_tensors(o64, p64), t32=oracle_tensors(o32, p32), draws=out, keep=keep, live=live_rays(d32["ray_valid"]),
                taps32=p32, dec32=d32)


def live_rays(ray_valid):
    """(B,n) bool: the rays that are marched - with one image, those that hit a cube (the others are dropped: exact zeros);
    in a batch, all"""
    rv = np.asarray(ray_valid, dtype=bool)
    return rv if rv.shape[0] == 1 else np.ones_like(rv)


def from_grad_referee(ref):
    """grad_referee.referee()'s result as referee()'s (amplitude 1). Its draws move every bin at random, not as moved_bins
    does: a narrower yardstick on some entries, which a kernel that forms the fp32 oracle's sample positions still meets."""
    return dict(t64=oracle_tensors(ref["out64"], ref["taps64"]), t32=oracle_tensors(ref["out32"], ref["taps32"]),
                draws={1: [oracle_tensors(o, t) for o, t in ref["fwd_draws"]]}, keep=ref["keep"].numpy().astype(bool),
                live=live_rays(ref["taps32"]["ray_validity"].numpy()), taps32=ref["taps32"], dec32=R.decisions(ref["taps32"]))


def exp_term(name, r64):
    """The term of EXP_ULP for the tensor `name` (None: it has none): for the fine weights, EXP_ULP x the transmittance in front
    of each interval, which float64's own weights give as 1 - the sum of the weights before it."""
    if name != "fine_weights":
        return None
    w = np.asarray(r64, dtype=np.float64)
    return EXP_ULP * np.clip(1.0 - (np.cumsum(w, -1) - w), 0.0, 1.0)


def bound_ratios(name, ours, r64, f32s, rays=None, a=A_YARDSTICK, rtol=RTOL, floor=FLOOR, grouped=None, extra=None):
    """Per group: max|ours - f64| / (a * max over f32s of max|f32 - f64| + rtol * max|f64| + floor * max over the tensor
    |f64| [+ `extra`, per group: exp_term()]); the tensor's maximum is taken over `rays` ((B,n) bool; default all). Every
    ratio must be <= 1. Returns the ratios, one per group, shaped as the tensor without its group axis (`grouped`: the last
    axis is one; default: by name)."""
    grp = (lambda x: np.abs(x).max(-1)) if (name in GROUPED if grouped is None else grouped) else np.abs
    r = np.asarray(r64, dtype=np.float64)
    ek = grp(np.asarray(ours, dtype=np.float64) - r)
    eo = np.zeros_like(ek)
    for f in f32s:
        eo = np.maximum(eo, grp(np.asarray(f, dtype=np.float64) - r))
    sel = r if rays is None else r[rays]
    top = float(np.abs(sel).max()) if sel.size else 0.0
    bound = a * eo + rtol * grp(r) + floor * top + (0.0 if extra is None else extra)
    return np.where(bound > 0, ek / np.where(bound > 0, bound, 1.0), np.where(ek > 0, np.inf, 0.0))


def check_forward(ours, ref, what, ulps=1, names=NAMES, rays=None):
    """Hold every tensor of `ours` (tensors()) to the referee `ref` on the rays that are marched and kept (or `rays`), the
    yardstick the fp32 oracle and the draws of amplitude `ulps`. Returns {name: worst ratio}; raises AssertionError naming
    the tensor and its worst entry.
    The colour of a sample inside no part's cube is left out: its density is zero by rule, so it reaches no output, and the
    reference's value for it (the MLP on a zero feature) is not what a kernel that skips a tile without a valid sample
    exports (zero)."""
    rays = (ref["keep"] & ref["live"]) if rays is None else rays
    in_a_part = ref["dec32"]["fine_valid"][..., :-1] != 0
    worst = {}
    for k in names:
        o, r64, r32 = ours[k], ref["t64"][k], ref["t32"][k]
        assert o.shape == r64.shape, (what, k, o.shape, r64.shape)
        rt = bound_ratios(k, o, r64, [r32] + [d[k] for d in ref["draws"][ulps]], rays, extra=exp_term(k, r64))
        rt = np.where(rays.reshape(rays.shape + (1,) * (rt.ndim - 2)), rt, 0.0)
        rt = np.where(in_a_part, rt, 0.0) if k == "fine_color" else rt
        worst[k] = float(rt.max()) if rt.size else 0.0
        if worst[k] > 1.0:
            i = np.unravel_index(int(np.argmax(rt)), rt.shape)
            raise AssertionError(f"{what}: {k}: entry {tuple(int(j) for j in i)} is {worst[k]:.3g}x its bound; "
                                 f"{int((rt > 1).sum())} of {int(rays.sum()) * int(np.prod(rt.shape[2:]))} entries above; ours "
                                 f"{o[i]} float64 {r64[i]} fp32 {r32[i]}; max |float64| {float(np.abs(r64[rays]).max()):.6g}")
    return worst


def fmt(worst):
    return ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
