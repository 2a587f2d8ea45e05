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
  * `bf16x3` and `bf16` (`check_forward_staged`) are held in two stages, with yardsticks of BF16X3_ULPS = 256 and BF16_ULPS =
    65536 fp32 ulp. Derivation, as for F16X3_ULPS: an operand split into two bf16 values (csrc/enarf_query.h split8: hi =
    bf16_rne(x), lo = bf16_rne(x - hi)) has a 16-bit significand, its unit in the last place is 2^(24 - 16) = 256 ulp of
    fp32's 24 bits; one bf16 value has 8 bits, 2^(24 - 8) = 65536 ulp. The draws of these amplitudes move the operands
    that the modes split and nothing else (`operand_scene`): the tri-plane's feature channels and each layer's
    conv.weight. The part-probability planes, z_rend, the modulation weights and the biases are not split - the
    demodulation runs in fp32 and the biases start the fp32 accumulators - and stay as they are; the bins move by one ulp.
      - Sample stage (`check_samples`): coarse and fine density and the fine colour at the mode's amplitude. The plain
        ensemble bound is degenerate for a density, relu(h) * 10: where h is slightly negative in float64, in fp32 and in
        all six draws the yardstick is zero, and one more realisation of the same noise crosses the kink (the mode model of
        tests/mlp_mode_model.py on p24_style256 in bf16: one coarse density at 1.9e5 x its bound). So a density's
        yardstick is taken on the signed density, h * 10 before the ReLU (the oracle's coarse / fine_signed_density taps):
        ReLU is 1-Lipschitz, so that bounds the density's own error and does not vanish at the kink. A sample inside no
        part's cube has density zero by rule and is compared exactly.
      - Composite stage (`check_composite`, run for all four modes): everything downstream of a density inherits its kink,
        and with 65 samples a ray, leaving out the rays with a sample near it would leave out most rays. So the fine
        weights and the ray's colour, mask and disparity are held to oracle.composite in float64 on the launch's OWN
        per-sample density, colour and depth; yardstick the fp32 composite of the same values and DRAWS more with density
        and colour moved by one ulp (not the depths: the kernel composes from exactly those). The EXP_ULP term of a weight
        carries over to the sums: sum of EXP_ULP * T_i for the mask, of EXP_ULP * T_i / depth_i for the disparity, of
        EXP_ULP * T_i * |c_i| per channel for the colour (`composite_terms`). This stage knows no mode and is sharper than
        the ensemble bound on the same tensors, which stays in force for `f32` and `f16x3`.
    Calibration of both stages against a model of the modes' operand roundings, the kink, corruptions, and what the
    method cannot see (errors below about one unit of the mode's operands per entry): tests/test_fwd_modes_cpu.py.

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
from oracle import enarf_oracle as O

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
BF16X3_ULPS = 256         # 2^(24 - 16): a bf16 pair carries a 16-bit significand
BF16_ULPS = 65536         # 2^(24 - 8): one bf16 carries an 8-bit significand
MODE_ULPS = {"f32": 1, "f16x3": F16X3_ULPS, "bf16x3": BF16X3_ULPS, "bf16": BF16_ULPS}
OPERAND_ULPS = (BF16X3_ULPS, BF16_ULPS)      # amplitudes whose draws move the split operands alone (operand_scene)
STAGED = ("bf16x3", "bf16")                  # modes held by check_forward_staged
SIGNED = {"coarse_density": "coarse_signed_density", "fine_density": "fine_signed_density"}
SAMPLE_STAGE = ("coarse_density", "fine_density", "fine_color")
COMPOSITE = ("fine_weights", "color", "mask", "disparity")


def _np(x):
    return x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


def tensors(color, mask, disparity, coarse_density, fine_density, fine_color, fine_depth, fine_weights, coarse_signed=None,
            fine_signed=None):
    """The eight compared tensors in one layout, float64 numpy, the ray axis second: per sample (B, n, samples) - fine_color
    (B, n, Nf - 1, 3) - and per ray (B, n) - color (B, n, 3). The last fine sample only closes the last interval: production
    never queries it, so it is left out of fine density and colour.
    In: color (B,3,n), mask / disparity (B,n), coarse_density (B,n,Nc), fine_density (B,n,Nf), fine_color (B,3,n,Nf),
    fine_depth (B,n,Nf), fine_weights (B,n,Nf-1). An oracle render adds its densities before the ReLU (coarse_signed,
    fine_signed, shaped as the densities): the yardstick of the two bf16 modes, never compared themselves."""
    t = {"coarse_density": _np(coarse_density), "fine_density": _np(fine_density)[..., :-1],
         "fine_color": _np(fine_color).transpose(0, 2, 3, 1)[:, :, :-1], "fine_depth": _np(fine_depth),
         "fine_weights": _np(fine_weights), "color": _np(color).transpose(0, 2, 1), "mask": _np(mask),
         "disparity": _np(disparity)}
    if coarse_signed is not None:
        t["coarse_signed_density"], t["fine_signed_density"] = _np(coarse_signed), _np(fine_signed)[..., :-1]
    return t


def oracle_tensors(outs, taps):
    """tensors() of one oracle render: outs = (color, mask, disparity), taps = its taps"""
    return tensors(*outs, taps["coarse_density"], taps["fine_density"], taps["fine_color"], taps["fine_depth"], taps["fine_weights"],
                   taps["coarse_signed_density"], taps["fine_signed_density"])


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


def perturb_features(tri, seed, ulps):
    """the tri-plane with its 96 feature channels moved by up to `ulps` ulp, the part-probability planes as they are"""
    out = tri.clone()
    out[:, :96] = R.perturb(tri[:, :96], seed, ulps)
    return out


def operand_scene(sc, i, ulps):
    """A shallow copy of the Scene with the operands that a bf16 mode splits moved by up to `ulps` ulp: the tri-plane's
    feature channels and each layer's conv.weight, nothing else. The part-probability planes, z_rend, the modulation weights
    and biases reach the MLP through fp32 arithmetic in every mode, and the biases start the fp32 accumulators."""
    import copy
    c = copy.copy(sc)
    c.raw = dict(sc.raw)
    c.raw["tri_plane"] = perturb_features(sc.raw["tri_plane"], 3000 + i, ulps)
    c.raw["mlp"] = {k: (R.perturb(v, 4000 + 97 * i + j, ulps) if k.endswith("conv.weight") else v)
                    for j, (k, v) in enumerate(sorted(sc.raw["mlp"].items()))}
    return c


def draw(sc, coord, Nc, Nf, bins, i, ulps=1, tri=None, render_scale=1.0, **modes):
    """fp32 render number i on inputs moved by up to `ulps` ulp (tri-plane, MLP parameters, z_rend - at an amplitude of
    OPERAND_ULPS the split operands alone, operand_scene; the bins by up to one ulp whatever `ulps`: no arithmetic mode
    touches them) -> (tensors, decisions)"""
    operands = ulps in OPERAND_ULPS
    moved = (operand_scene if operands else R.perturbed_scene)(sc, i, ulps)
    if tri is not None:
        tri = perturb_features(tri, 2000 + i, ulps) if operands else R.perturb(tri, 2000 + i, ulps)
    with torch.no_grad():
        o, _, t = R.render_forward(moved, coord, Nc, Nf, moved_bins(bins, i), torch.float32, tri, render_scale, **modes)
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
                taps32=p32, dec32=d32, render_scale=render_scale)


def live_rays(ray_valid):
    """(B,n) bool: the rays that are marched - with one image, those that hit a cube (the others are dropped: exact zeros);
    in a batch, all"""
    rv = np.asarray(ray_valid, dtype=bool)
    return rv if rv.shape[0] == 1 else np.ones_like(rv)


def from_grad_referee(ref, render_scale=1.0):
    """grad_referee.referee()'s result as referee()'s (amplitude 1). Its draws move every bin at random, not as moved_bins
    does: a narrower yardstick on some entries, which a kernel that forms the fp32 oracle's sample positions still meets."""
    return dict(t64=oracle_tensors(ref["out64"], ref["taps64"]), t32=oracle_tensors(ref["out32"], ref["taps32"]),
                draws={1: [oracle_tensors(o, t) for o, t in ref["fwd_draws"]]}, keep=ref["keep"].numpy().astype(bool),
                live=live_rays(ref["taps32"]["ray_validity"].numpy()), taps32=ref["taps32"], dec32=R.decisions(ref["taps32"]),
                render_scale=render_scale)


def exp_term(name, r64):
    """The term of EXP_ULP for the tensor `name` (None: it has none): for the fine weights, EXP_ULP x the transmittance in front
    of each interval, which float64's own weights give as 1 - the sum of the weights before it."""
    if name != "fine_weights":
        return None
    w = np.asarray(r64, dtype=np.float64)
    return EXP_ULP * np.clip(1.0 - (np.cumsum(w, -1) - w), 0.0, 1.0)


def bound_ratios(name, ours, r64, f32s, rays=None, a=A_YARDSTICK, rtol=RTOL, floor=FLOOR, grouped=None, extra=None, yard64=None):
    """Per group: max|ours - f64| / (a * max over f32s of max|f32 - f64| + rtol * max|f64| + floor * max over the tensor
    |f64| [+ `extra`, per group: exp_term()]); the tensor's maximum is taken over `rays` ((B,n) bool; default all). Every
    ratio must be <= 1. Returns the ratios, one per group, shaped as the tensor without its group axis (`grouped`: the last
    axis is one; default: by name). `yard64`: the float64 tensor the f32s are measured from where that is not r64 - the
    signed density, f32s its fp32 renders, for a density."""
    grp = (lambda x: np.abs(x).max(-1)) if (name in GROUPED if grouped is None else grouped) else np.abs
    r = np.asarray(r64, dtype=np.float64)
    y = r if yard64 is None else np.asarray(yard64, dtype=np.float64)
    ek = grp(np.asarray(ours, dtype=np.float64) - r)
    eo = np.zeros_like(ek)
    for f in f32s:
        eo = np.maximum(eo, grp(np.asarray(f, dtype=np.float64) - y))
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


def _worst(what, k, rt, rays, o, r64, r32):
    """the largest ratio of one tensor; raises AssertionError naming the tensor and its worst entry if it is above 1"""
    w = float(rt.max()) if rt.size else 0.0
    if not w <= 1.0:
        i = np.unravel_index(int(np.argmax(rt)), rt.shape)
        raise AssertionError(f"{what}: {k}: entry {tuple(int(j) for j in i)} is {w:.3g}x its bound; "
                             f"{int((rt > 1).sum())} of {int(rays.sum()) * int(np.prod(rt.shape[2:]))} entries above; ours "
                             f"{o[i]} float64 {r64[i]} fp32 {r32[i]}; max |float64| {float(np.abs(r64[rays]).max()):.6g}")
    return w


def _on(rays, rt):
    return np.where(rays.reshape(rays.shape + (1,) * (rt.ndim - 2)), rt, 0.0)


def check_samples(ours, ref, what, ulps, names=SAMPLE_STAGE, rays=None):
    """The sample stage of a bf16 mode: coarse and fine density and the fine colour, the yardstick the fp32 oracle and the
    draws of amplitude `ulps`. A density is held to

        |ours - f64|  <=  A * max over renders |signed_f32 - signed_f64|  +  RTOL * |f64|  +  FLOOR * max|f64|

    signed = the density before its ReLU (the oracle's coarse / fine_signed_density). The density is relu(h) * 10, and where
    h is slightly negative in float64, in fp32 and in every draw, the plain yardstick |f32 - f64| is zero: one more
    realisation of the same noise crosses the kink and is infinitely far outside (p24_style256 in bf16: a coarse density at
    1.9e5 x that bound). ReLU is 1-Lipschitz, so the distance of the signed densities bounds the distance of the densities,
    and it does not vanish at the kink. A sample inside no part's cube has density zero by rule - no arithmetic - and is
    compared exactly. The colour (a tanh: smooth) keeps the plain yardstick; inside no part's cube it is left out, as in
    check_forward."""
    rays = (ref["keep"] & ref["live"]) if rays is None else rays
    in_a_part = {"fine_density": ref["dec32"]["fine_valid"][..., :-1] != 0, "fine_color": ref["dec32"]["fine_valid"][..., :-1] != 0,
                 "coarse_density": ref["taps32"]["coarse_valid"].any(1).numpy()}
    worst = {}
    for k in names:
        o, r64, r32 = ours[k], ref["t64"][k], ref["t32"][k]
        assert o.shape == r64.shape, (what, k, o.shape, r64.shape)
        y = SIGNED.get(k, k)
        rt = bound_ratios(k, o, r64, [ref["t32"][y]] + [d[y] for d in ref["draws"][ulps]], rays, yard64=ref["t64"][y])
        if k in SIGNED:
            rt = np.where(in_a_part[k], rt, np.where(o == 0, 0.0, np.inf))
        else:
            rt = np.where(in_a_part[k], rt, 0.0)
        worst[k] = _worst(what, k, _on(rays, rt), rays, o, r64, r32)
    return worst


def composite_terms(w64, depth, color):
    """The EXP_ULP terms of the composite stage, from the float64 weights of the launch's own taps: a weight gets EXP_ULP x
    the transmittance T in front of it (exp_term); a sum over a ray gets the sum of its weights' terms - the mask sum
    EXP_ULP * T_i, the disparity sum EXP_ULP * T_i / depth_i, the colour, per channel, sum EXP_ULP * T_i * |c_i|."""
    t = exp_term("fine_weights", w64)
    z = depth[..., :-1]
    return {"fine_weights": t, "mask": t.sum(-1), "disparity": np.where(z > 0, t / np.where(z > 0, z, 1.0), 0.0).sum(-1),   # a dropped ray: 0
            "color": (t[..., None] * np.abs(color)).sum(-2)}


def check_composite(ours, ref, what, rays=None, names=COMPOSITE):
    """The composite stage, whatever the MLP's arithmetic: the launch's fine weights and its ray's colour, mask and disparity
    against oracle.composite in float64 on the launch's OWN per-sample results (ours["fine_density"], ["fine_color"],
    ["fine_depth"]: the values the kernel composes from - csrc/enarf_tasks.h ray_composite_stage exports exactly the
    den / cr, cg, cb / fdepth it integrates). Yardstick: the fp32 composite of the same values and DRAWS more with every
    density and colour moved by up to one ulp; the depths are not moved: the kernel composes from exactly those. A, RTOL,
    FLOOR as everywhere, the EXP_ULP terms of composite_terms. Returns {name: worst ratio}; raises as check_forward."""
    rays = (ref["keep"] & ref["live"]) if rays is None else rays
    den = torch.from_numpy(np.concatenate([ours["fine_density"], ours["fine_density"][..., -1:]], -1))     # the last is not read
    col = torch.from_numpy(np.concatenate([ours["fine_color"], ours["fine_color"][:, :, -1:]], 2).transpose(0, 3, 1, 2).copy())
    dep = torch.from_numpy(ours["fine_depth"])

    def comp(d, c, z):
        rc, rm, rd, w = O.composite(d, c, z, ref["render_scale"])
        return {"fine_weights": _np(w), "color": _np(rc).transpose(0, 2, 1), "mask": _np(rm), "disparity": _np(rd)}

    c64 = comp(den, col, dep)
    f32s = [comp(den.float(), col.float(), dep.float())]
    for i in range(DRAWS):
        f32s.append(comp(R.perturb(den.float(), 6000 + i), R.perturb(col.float(), 7000 + i), dep.float()))
    extra = composite_terms(c64["fine_weights"], ours["fine_depth"], ours["fine_color"])
    worst = {}
    for k in names:
        rt = bound_ratios(k, ours[k], c64[k], [f[k] for f in f32s], rays, extra=extra[k])
        worst[k] = _worst(f"{what}: composite stage", k, _on(rays, rt), rays, ours[k], c64[k], f32s[0][k])
    return worst


def check_forward_staged(ours, ref, mode, what=None, rays=None):
    """A bf16 mode in stages: the fine depth as check_forward holds it (no mode touches it, and its yardstick is the same at
    every amplitude: of all that a draw moves, only the bins reach a depth, by one ulp whatever the amplitude; the discrete
    decisions the caller asserts, as for the other modes), the sample stage at the mode's amplitude (check_samples), then
    the composite stage on the launch's own samples (check_composite). A plain ensemble bound on the weights and ray sums
    would inherit the kink of every density in front of them; the composite stage depends on no MLP output but the
    launch's own. Returns {name: worst ratio} over the eight tensors."""
    what = what or mode
    worst = check_forward(ours, ref, what, ulps=MODE_ULPS[mode], names=("fine_depth",), rays=rays)
    worst.update(check_samples(ours, ref, what, MODE_ULPS[mode], rays=rays))
    worst.update(check_composite(ours, ref, what, rays=rays))
    return {k: worst[k] for k in NAMES}


def fmt(worst):
    return ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
