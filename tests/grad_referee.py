"""A float64 referee for the renderer's gradients and a per-element bound to hold a kernel's gradients to.

Referee: autograd through oracle.enarf_oracle on float64 copies of the fp32 inputs (the oracle follows its inputs' dtype),
the kernel's bins replayed. The same graph in fp32 is the yardstick: its distance from float64 is what the reference's own
arithmetic costs on each entry.

Bound (`bound_ratios`). A tensor's gradient entries span ~40 orders of magnitude (float64 carries entries down to ~1e-43 of
the maximum), and a bound relative to the tensor's maximum misses almost all of them: on a 72-ray band of a 32^2 frame
(Nc 48, Nf 32, sorted random bins; the set-up of test_gpu_backward.test_render_backward_matches_oracle_autograd), 93.0 % of
the 578 304 non-zero feature-plane entries and 89.4 % of the 31 321 part-probability entries lie below 1e-3 of the
maximum. So every entry e is held to its own scale:

    |ours(e) - f64(e)|  <=  A * max over fp32 draws |f32(e) - f64(e)|  +  RTOL * |f64(e)|  +  FLOOR * max|f64|

per group - a feature-plane texel's 32 channels, every other entry alone - as the max over the group of each term.
  * A * |f32 - f64|: on that band the fp32 oracle differs from float64 by up to 9.0 % (feature planes) and 5.3 %
    (part-probability planes) element-wise on entries above 1e-6 of the maximum, 0.43 % above 1e-4. That is cancellation
    upstream of the scatter (fine depths from fp32 bins, the compositing prefix / suffix sums, the MLP backward), which a
    bound built from the last linear stage (sum |bilinear weight x upstream|) does not cover. Another fp32 computation makes
    errors of the same size on the same entries: fp32 runs with every input changed by up to 1 ulp came to at most 1.13x
    the yardstick's error in any group of any of the 15 tensors (three draws); the same rays summed as two halves, 1.0x.
    Per group, though, the error of one fp32 draw is a random quantity: a second draw can be 100x the first where the first
    happens to land close to float64. So the yardstick is the largest error over the fp32 oracle and DRAWS = 6 draws on
    inputs moved by up to one ulp (bins, tri-plane, MLP parameters, z_rend). A = 8 over that ensemble: 16 further draws
    with other seeds came to at most 0.90 of the bound (the rays of the GPU matrix at Nf 2, 3, 16 and 33).
  * RTOL * |f64|: where fp32 happens to hit float64 almost exactly, a few hundred ulp of the group's own magnitude.
    RTOL = 1e-4 (the forward's bound), 100x below the 1 % change the self-test must catch.
  * FLOOR * max: fp32 cannot hold float64's smallest entries, nor keep them in a sum with larger ones. FLOOR = 1e-6 of the
    tensor's maximum, three orders below the old max-normalised bound of 1e-3.
What it accepts and rejects (tests/test_grad_referee_cpu.py, same band): fp32 draws outside the yardstick pass; the fp32
oracle with every entry below 1e-3 of the maximum set to zero fails by ~800x; with a 1 % subset of texels scaled by 0.99,
by ~50x."""
import numpy as np
import torch

from oracle import enarf_oracle as O

A_YARDSTICK = 8.0
DRAWS = 6
RTOL = 1e-4
FLOOR = 1e-6

LEAVES = [f"layers.{l}.{k}" for l in range(3) for k in ("conv.weight", "conv.modulation.weight", "conv.modulation.bias", "bias")]


def render_forward(sc, coord, Nc, Nf, bins, dtype, tri=None, render_scale=1.0, **modes):
    """The oracle's render in `dtype` on leaves that require grad. sc: a _helpers.Scene; coord (B,1,3,n) or (B,3,n); bins
    (B,n,Nf) float32; tri: the tri-plane (default: the scene's) - batch 1 with B > 1 is a tri-plane shared by every image
    (its gradient is the sum over images). Returns (outputs (color, mask, disparity), leaves, taps)."""
    s = sc.raw
    B = coord.shape[0]
    t = (s["tri_plane"] if tri is None else tri).to(dtype).clone().requires_grad_(True)
    tri_b = t.expand(B, -1, -1, -1) if t.shape[0] != B else t
    mlp = {k: v.to(dtype).clone().requires_grad_(True) for k, v in s["mlp"].items() if "noise" not in k}
    z = s["z_rend"].to(dtype).clone().requires_grad_(True)
    rc, rm, rd, taps = O.render(coord.to(dtype), sc.pose_parts.to(dtype), sc.bl_parts.to(dtype), s["inv_intrinsics"].to(dtype),
                                sc.cpose.to(dtype), sc.cbl, tri_b, mlp, z, sc.cs, Nc, Nf, render_scale=render_scale,
                                bins=bins.to(dtype), return_taps=True, **modes)
    return (rc, rm, rd), (t, z, mlp), taps


def render_grads(outs, leaves, gc, gm, gd, keep_rays=None):
    """Gradients of sum(color * gc) + sum(mask * gm) + sum(disparity * gd) over the rays in keep_rays ((B,n) bool; the
    others' upstream gradients count as zero) -> {"feat", "mask", "z", *LEAVES}."""
    rc, rm, rd = outs
    t, z, mlp = leaves
    dt = rc.dtype
    k = torch.ones(rm.shape, dtype=dt) if keep_rays is None else keep_rays.to(dt)
    loss = (rc * (gc.to(dt) * k[:, None])).sum() + (rm * (gm.to(dt) * k)).sum() + (rd * (gd.to(dt) * k)).sum()
    g = torch.autograd.grad(loss, [t, z] + [mlp[q] for q in LEAVES], allow_unused=True, retain_graph=True)
    grads = {"feat": g[0][:, :96], "mask": g[0][:, 96:], "z": g[1]}
    for q, v in zip(LEAVES, g[2:]):
        grads[q] = torch.zeros_like(mlp[q]) if v is None else v
    return {q: v.detach() for q, v in grads.items()}


def decisions(taps):
    """The discrete decisions a render takes per ray: validity, the depth range (ends picked from a 32-depth table), the part
    bit mask of every fine sample."""
    from _helpers import bits_of
    return {"ray_valid": taps["ray_validity"].numpy().astype(bool), "fine_valid": bits_of(taps["fine_valid"]),
            "dmin": taps["depth_min"].double().numpy(), "dmax": taps["depth_max"].double().numpy()}


def disagreeing_rays(d64, d32):
    """(B,n) bool: rays on which float64 and fp32 arithmetic take a different discrete decision (a point within rounding of
    a cube face, or a ray grazing one). Such rays are excluded from a comparison by rule, never covered by tolerance."""
    bad = d64["ray_valid"] != d32["ray_valid"]
    for k in ("dmin", "dmax"):
        bad |= np.abs(d64[k] - d32[k]) > 1e-5 * np.abs(d64[k])
    bad |= (d64["fine_valid"] != d32["fine_valid"]).any(axis=-1)
    return bad


def referee(sc, coord, Nc, Nf, bins, gc, gm, gd, tri=None, render_scale=1.0, **modes):
    """The float64 referee and the fp32 yardstick on the same rays, the rays they disagree on excluded (`keep` False).

    Returns dict(out64, out32, g64, g32, draws, keep (B,n) bool tensor, taps64, taps32, fwd_draws) - fwd_draws: the draws'
    forward results [(outputs, taps)], which tests/fwd_referee.py holds the forward to."""
    o64, l64, t64 = render_forward(sc, coord, Nc, Nf, bins, torch.float64, tri, render_scale, **modes)
    o32, l32, t32 = render_forward(sc, coord, Nc, Nf, bins, torch.float32, tri, render_scale, **modes)
    keep = torch.from_numpy(~disagreeing_rays(decisions(t64), decisions(t32)))
    g64 = render_grads(o64, l64, gc, gm, gd, keep)
    g32 = render_grads(o32, l32, gc, gm, gd, keep)
    # more draws of fp32 rounding: every input (bins, tri-plane, MLP parameters, z_rend) moved by up to one ulp, so the
    # fine depths, their differences and every product round another way
    draws, fwd_draws = [], []
    for i in range(DRAWS):
        op, lp, tp = render_forward(perturbed_scene(sc, i), coord, Nc, Nf, perturb(bins, 1000 + i).sort(-1).values, torch.float32,
                                    None if tri is None else perturb(tri, 2000 + i), render_scale, **modes)
        keep &= torch.from_numpy(~disagreeing_rays(decisions(tp), decisions(t32)))
        draws.append((op, lp))
        fwd_draws.append((tuple(o.detach() for o in op), _detached(tp)))
    gd32 = [render_grads(op, lp, gc, gm, gd, keep) for op, lp in draws]
    if not bool(keep.all()):                     # a ray dropped by a later draw: the first two again without it
        g64, g32 = render_grads(o64, l64, gc, gm, gd, keep), render_grads(o32, l32, gc, gm, gd, keep)
    return dict(out64=tuple(o.detach() for o in o64), out32=tuple(o.detach() for o in o32), g64=g64, g32=g32, draws=gd32,
                keep=keep, taps64=_detached(t64), taps32=t32, fwd_draws=fwd_draws)


def _detached(taps):
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in taps.items()}


def perturb(t, seed, ulps=1):
    """t with every element moved by -ulps, 0 or +ulps ulp (at random; float32)"""
    g = torch.Generator().manual_seed(seed)
    return t * (1 + torch.randint(-1, 2, t.shape, generator=g).float() * (ulps * 2 ** -23))


def perturbed_scene(sc, i, ulps=1):
    """a shallow copy of the Scene whose tri-plane, MLP parameters and z_rend are moved by up to `ulps` ulp"""
    import copy
    c = copy.copy(sc)
    c.raw = dict(sc.raw)
    c.raw["tri_plane"] = perturb(sc.raw["tri_plane"], 3000 + i, ulps)
    c.raw["mlp"] = {k: perturb(v, 4000 + 97 * i + j, ulps) for j, (k, v) in enumerate(sorted(sc.raw["mlp"].items()))}
    c.raw["z_rend"] = perturb(sc.raw["z_rend"], 5000 + i, ulps)
    return c


def _groups(name, x, signed=False):
    """|x| (x with signed=True) as (groups, members): a feature-plane texel's 32 channels form one group, every other entry
    its own."""
    a = np.asarray(x, dtype=np.float64)
    a = a if signed else np.abs(a)
    if name == "feat":
        Bt, C, H, W = a.shape
        return a.reshape(Bt, 3, 32, H * W).transpose(0, 1, 3, 2).reshape(-1, 32)
    return a.reshape(-1, 1)


def bound_ratios(name, ours, g64, g32, a=A_YARDSTICK, rtol=RTOL, floor=FLOOR, draws=()):
    """Per group: max|ours - f64| / (a * max|f32 - f64| + rtol * max|f64| + floor * max over the tensor |f64|), the fp32
    term the largest over the fp32 oracle and its perturbed `draws`. Every ratio must be <= 1. Returns the ratios."""
    r = np.asarray(g64, dtype=np.float64)
    ek = _groups(name, np.asarray(ours, dtype=np.float64) - r).max(1)
    eo = _groups(name, np.asarray(g32, dtype=np.float64) - r).max(1)
    for d in draws:
        eo = np.maximum(eo, _groups(name, np.asarray(d, dtype=np.float64) - r).max(1))
    sc = _groups(name, r).max(1)
    top = float(np.abs(r).max()) if r.size else 0.0
    bound = a * eo + rtol * sc + floor * top
    return np.where(bound > 0, ek / np.where(bound > 0, bound, 1.0), np.where(ek > 0, np.inf, 0.0))


def check_grads(ours, ref, what, names=None):
    """Hold every gradient tensor of `ours` (dict name -> tensor, any device) to the referee `ref` (referee()'s dict).
    Returns {name: worst ratio}; raises AssertionError naming the tensor and its worst group."""
    worst = {}
    for k in (names or ref["g64"].keys()):
        o = ours[k].detach().cpu().numpy() if torch.is_tensor(ours[k]) else np.asarray(ours[k])
        r64, r32 = ref["g64"][k].numpy(), ref["g32"][k].numpy()
        assert o.size == r64.size, (what, k, o.shape, r64.shape)
        rt = bound_ratios(k, o.reshape(r64.shape), r64, r32, draws=[d[k].numpy() for d in ref.get("draws", ())])
        i = int(np.argmax(rt)) if rt.size else 0
        worst[k] = float(rt[i]) if rt.size else 0.0
        if worst[k] > 1.0:
            ch = int(np.argmax(_groups(k, o.reshape(r64.shape) - r64)[i]))
            at = lambda x: float(_groups(k, np.asarray(x).reshape(r64.shape), signed=True)[i, ch])
            raise AssertionError(f"{what}: d {k}: group {i} is {worst[k]:.3g}x its bound; {int((rt > 1).sum())} of {rt.size} "
                                 f"groups above; worst entry (member {ch}): ours {at(o):.9g} float64 {at(r64):.9g} fp32 "
                                 f"{at(r32):.9g}; max |float64| {float(np.abs(r64).max()):.6g}")
    return worst
