"""A float64 referee for the query's gradients with respect to its sample points and its part frames, in the manner of
tests/grad_referee.py, whose bound (form and constants) it uses.

Referee: autograd through oracle.enarf_oracle.query on float64 copies of the fp32 inputs, differentiated with respect to
`points` (B,3,N), `pose_scaled` (B,P,4,4) and `scale` (B,P) (leaves="record") - or with respect to the 24 joints
`pose_to_camera` (B,24,4,4) and `bone_length` carried through O.transform_pose / O.scale_pose_translation /
O.canonical_scale (leaves="joints"), or to the unscaled part frames and their bone lengths (leaves="frames"). The same
graph in fp32 is the yardstick, with DRAWS further fp32 runs on inputs moved by up to one ulp. What is differentiated is
what the reference's autograd returns, MyReLU's backward rule included, not the derivative.

Exclusion, a rule and never a tolerance. A point is excluded when fp32 (the yardstick or any draw) and float64 disagree on
a validity bit, on the floor of any tap coordinate of a valid (part, point) pair, or - with multiply_density_with_weight -
on which part is the arg-max of the weight. A fourth decision of the same kind is on the list: the side of the
LeakyReLU's kink each of the MLP's 64 + 64 + 4 pre-activations is on (the last one is also MyReLU's region). Without it the
referee fails its own self-test: with Scene(32, 2) and 512 points an image, a held-out fp32 draw (inputs moved by one ulp)
differs from float64 by 9 % on one point's gradient, 92x the bound, while every decision above agrees - pre-activation
93 of that point lies within an ulp of zero, and the draw puts it on the other side, where the reference's own gradient
has another slope. An excluded point's upstream gradients are zero on both sides (`keep`), so its own gradient and its
share of every part-frame entry are zero on both sides. At most MAX_EXCLUDED of the points may be excluded (7 of 2000 are,
on the GPU tests' points, 1 of them by the first three decisions).

Bound: grad_referee.bound_ratios with A_YARDSTICK, RTOL and FLOOR as they stand, every entry its own group."""
import numpy as np
import torch

import grad_referee as R
from oracle import enarf_oracle as O

MAX_EXCLUDED = 0.01

# the four modes: name -> (keywords of O.query, keywords of ops.query_fwd / ops.query_pose_bwd)
MODES = {
    "default": ({}, {}),
    "clamp_mask": (dict(clamp_mask=True), dict(clamp_mask=True)),
    "no_selector": (dict(no_selector=True), dict(uniform_part_weight=True)),
    "multiply_density_with_weight": (dict(multiply_density_with_weight=True), dict(multiply_density_with_weight=True)),
}


def scene_points(sc, n, seed=0, radius=0.1):
    """(B,3,n) fp32 points of the scaled space drawn around the part centres: point i belongs to part i % P and lies at a
    uniform offset of up to `radius` (canonical units, per axis) from that part's origin, carried to the camera frame by
    the part's own transform. Neighbouring cubes overlap there, so most points lie in several."""
    g = torch.Generator().manual_seed(seed)
    B, P = sc.pose_scaled.shape[:2]
    k = torch.arange(n) % P
    off = (torch.rand(B, n, 3, generator=g) * 2 - 1) * radius
    Rc, Rm, t = sc.cpose[k, :3, :3], sc.pose_scaled[:, k, :3, :3], sc.pose_scaled[:, k, :3, 3]
    local = torch.einsum("nji,bnj->bni", Rc, off) / sc.scale[:, k, None]            # l = Rc^T off / s
    return (t + torch.einsum("bnij,bnj->bni", Rm, local)).permute(0, 2, 1).contiguous().float()


def outside_points(sc, n):
    """(B,3,n) fp32 points far outside every cube"""
    g = torch.Generator().manual_seed(11)
    return (torch.rand(sc.B, 3, n, generator=g) + 50.0).float()


def upstream(B, n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g), torch.randn(B, 3, n, generator=g)


def parts_record_grad(g_pose, g_scale):
    """gradients of pose_scaled (B,P,4,4) and scale (B,P) laid out as the (B,P,16) part record: R row-major, t, s, zeros"""
    B, P = g_scale.shape
    out = torch.zeros(B, P, 16, dtype=g_pose.dtype)
    out[:, :, :9] = g_pose[:, :, :3, :3].reshape(B, P, 9)
    out[:, :, 9:12] = g_pose[:, :, :3, 3]
    out[:, :, 12] = g_scale
    return out


def _inputs(sc, pts, dtype, draw=None):
    """the query's inputs in `dtype`, every fp32 input moved by up to one ulp for draw >= 0"""
    s = sc.raw
    mv = (lambda t, seed: t) if draw is None else (lambda t, seed: R.perturb(t, seed + draw))
    mlp = {k: mv(v, 4000 + 97 * j).to(dtype) for j, (k, v) in enumerate(sorted(s["mlp"].items()))}
    return dict(points=mv(pts, 6000).to(dtype), pose_to_camera=mv(s["pose_to_camera"], 7000).to(dtype),
                bone_length=mv(s["bone_length"], 8000).to(dtype), pose_scaled=mv(sc.pose_scaled, 7500).to(dtype),
                scale=mv(sc.scale, 8500).to(dtype), pose_parts=mv(sc.pose_parts, 7700).to(dtype),
                bl_parts=mv(sc.bl_parts, 8700).to(dtype), tri=mv(s["tri_plane"], 3000).to(dtype),
                weights=O.modulated_weights(mlp, mv(s["z_rend"], 5000).to(dtype)))


def forward(sc, pts, dtype, mode, leaves="record", draw=None, drop_w_term=False):
    """O.query in `dtype` on leaves that require grad -> dict(density (B,N), color (B,3,N), leaves, decisions).
    drop_w_term: the part weights detached (what a backward that forgets dw/dc computes; the self-test's negative)."""
    x = _inputs(sc, pts, dtype, draw)
    p = x["points"].clone().requires_grad_(True)
    if leaves == "joints":
        a, bl = x["pose_to_camera"].clone().requires_grad_(True), x["bone_length"].clone().requires_grad_(True)
        pose_parts, bl_parts = O.transform_pose(a, bl, sc.ol, sc.raw["parents"])
        pose, scale = O.scale_pose_translation(pose_parts, sc.cs), O.canonical_scale(sc.cbl, bl_parts, sc.cs)
        leaves = {"g_points": p, "pose_to_camera": a, "bone_length": bl}
    elif leaves == "frames":
        pp, blp = x["pose_parts"].clone().requires_grad_(True), x["bl_parts"].clone().requires_grad_(True)
        pose, scale = O.scale_pose_translation(pp, sc.cs), O.canonical_scale(sc.cbl, blp, sc.cs)
        leaves = {"g_points": p, "pose_parts": pp, "bl_parts": blp}
    else:
        pose, scale = x["pose_scaled"].clone().requires_grad_(True), x["scale"].clone().requires_grad_(True)
        leaves = {"g_points": p, "pose": pose, "scale": scale}
    kw = dict(MODES[mode][0])
    if drop_w_term:
        den, col = _query_detached_weight(p, pose, scale, sc.cpose.to(dtype), x["tri"], x["weights"], **kw)
        return dict(density=den[:, 0], color=col, leaves=leaves, decisions=None)
    den, col, valid, taps = O.query(p, pose, scale, sc.cpose.to(dtype), x["tri"], x["weights"], return_taps=True, **kw)
    H, W = x["tri"].shape[2:]
    c = taps["canonical"].detach()
    cells = torch.stack([torch.floor(O._unnormalize(c, W)), torch.floor(O._unnormalize(c, H))], dim=-1)     # (B,P,3,N,2)
    cells = cells * valid[:, :, None, :, None]                                       # only valid pairs are sampled
    dec = dict(valid=valid.detach(), cells=cells.to(torch.int64), argmax=taps["weight"].detach().argmax(dim=1),
               units=_unit_signs(taps["feature"].detach(), x["weights"]))
    return dict(density=den[:, 0], color=col, leaves=leaves, decisions=dec)


def _unit_signs(feature, weights):
    """(B,132,N) bool: which of the MLP's 64 + 64 + 4 pre-activations are positive (the side of the LeakyReLU's kink each
    unit is on; the last one is also MyReLU's region). Same operations as O.styled_mlp, so the same values."""
    h, signs = feature, []
    for (w, bias) in weights:
        z = torch.bmm(w.detach(), h) + bias.detach()[None, :, None]
        signs.append(z > 0)
        h = torch.nn.functional.leaky_relu(z, 0.2) * 2 ** 0.5
    return torch.cat(signs, dim=1)


def _query_detached_weight(points, pose, scale, cpose, tri, weights, **kw):
    """O.query with the part weights treated as constants"""
    local, canonical = O.to_local_and_canonical(points, pose, scale, cpose)
    valid = O.validity(local, canonical)
    if kw.get("no_selector"):
        w = torch.full(valid.shape, 1.0 / pose.shape[1], dtype=points.dtype)
    else:
        w = O.part_prob(tri[:, 96:], canonical, valid, False, kw.get("clamp_mask", False)).detach()
    feat = O.weighted_feature(tri[:, :96], canonical, w, valid)
    h = O.styled_mlp(feat, weights)
    den = O.MyReLU.apply(h[:, 3:])
    den = den * (10 * w.max(dim=1, keepdim=True)[0]) if kw.get("multiply_density_with_weight") else den * 10
    return den * valid.any(dim=1, keepdim=True), torch.tanh(h[:, :3])


def disagreeing_points(d_a, d_b, with_argmax):
    """(B,N) bool: points on which two runs take a different discrete decision"""
    bad = (d_a["valid"] != d_b["valid"]).any(dim=1)
    bad |= (d_a["cells"] != d_b["cells"]).flatten(1, 2).any(dim=1).any(dim=-1)
    if with_argmax:
        bad |= d_a["argmax"] != d_b["argmax"]
    bad |= (d_a["units"] != d_b["units"]).any(dim=1)
    return bad


def point_loss(gd, gc):
    """sum(density gd keep) + sum(colour gc keep) as a loss(fw, keep); gd (B,N) or None, gc (B,3,N) or None"""
    def loss(fw, keep):
        dt = fw["density"].dtype
        k = keep.to(dt)
        total = fw["density"].sum() * 0
        if gd is not None:
            total = total + (fw["density"] * (gd.to(dt) * k)).sum()
        if gc is not None:
            total = total + (fw["color"] * (gc.to(dt) * k[:, None])).sum()
        return total
    return loss


def grads(fw, loss_fn, keep):
    """gradients of loss_fn(fw, keep) for the leaves of a forward() -> {name: tensor}; with the leaves pose / scale also
    "g_parts", the (B,P,16) record layout"""
    loss = loss_fn(fw, keep)
    names = list(fw["leaves"])
    g = torch.autograd.grad(loss, [fw["leaves"][n] for n in names], allow_unused=True, retain_graph=True)
    out = {n: (torch.zeros_like(fw["leaves"][n]) if v is None else v.detach()) for n, v in zip(names, g)}
    if "pose" in out:
        out["g_parts"] = parts_record_grad(out["pose"], out["scale"])
    return out


class Referee:
    """The float64 referee, the fp32 yardstick and its draws for one (scene, points, mode): the forwards run once, the
    gradients per request. `keep` (B,N) bool is False for the excluded points."""

    def __init__(self, sc, pts, mode, leaves="record"):
        self.sc, self.pts, self.mode, self.leaves = sc, pts, mode, leaves
        self.f64 = forward(sc, pts, torch.float64, mode, leaves)
        self.f32 = forward(sc, pts, torch.float32, mode, leaves)
        self.draws = [forward(sc, pts, torch.float32, mode, leaves, draw=i) for i in range(R.DRAWS)]
        am = mode == "multiply_density_with_weight"
        bad = disagreeing_points(self.f64["decisions"], self.f32["decisions"], am)
        for d in self.draws:
            bad |= disagreeing_points(self.f64["decisions"], d["decisions"], am)
        self.keep = ~bad
        self.excluded = float(bad.float().mean())
        assert self.excluded <= MAX_EXCLUDED, f"{mode}: {self.excluded * 100:.2f} % of the points excluded, cap 1 %"
        self._cache = {}

    def valid_bits(self):
        from _helpers import bits_of
        return bits_of(self.f32["decisions"]["valid"])

    def grads(self, gd, gc, n=None):
        """dict(g64, g32, draws, keep) of the loss sum(density gd) + sum(colour gc) over the first n points (all by
        default): the others' upstream gradients are zero"""
        key = (n, None if gd is None else gd.data_ptr(), None if gc is None else gc.data_ptr())
        if key not in self._cache:
            keep = self.keep.clone()
            if n is not None:
                keep[:, n:] = False
            self._cache[key] = self.grads_of(point_loss(gd, gc), keep)
        return self._cache[key]

    def grads_of(self, loss_fn, keep=None):
        """dict(g64, g32, draws, keep) of any loss_fn(fw, keep) of a forward()'s density (B,N) and colour (B,3,N)"""
        keep = self.keep if keep is None else keep
        return dict(g64=grads(self.f64, loss_fn, keep), g32=grads(self.f32, loss_fn, keep),
                    draws=[grads(d, loss_fn, keep) for d in self.draws], keep=keep)


def check(ours, ref, what, names):
    """Hold `ours` (name -> tensor or array) to a Referee.grads() dict on `names`, every entry to its own scale; returns
    {name: worst ratio}, AssertionError naming the tensor and its worst entry."""
    worst = {}
    for k in names:
        o = ours[k].detach().cpu().numpy() if torch.is_tensor(ours[k]) else np.asarray(ours[k])
        r64, r32 = ref["g64"][k].numpy(), ref["g32"][k].numpy()
        assert o.shape == r64.shape, (what, k, o.shape, r64.shape)
        rt = R.bound_ratios(k, o, r64, r32, draws=[d[k].numpy() for d in ref["draws"]])
        i = int(np.argmax(rt)) if rt.size else 0
        worst[k] = float(rt[i]) if rt.size else 0.0
        if worst[k] > 1.0:
            raise AssertionError(f"{what}: {k}: entry {np.unravel_index(i, r64.shape)} is {worst[k]:.3g}x its bound; "
                                 f"{int((rt > 1).sum())} of {rt.size} above; ours {o.reshape(-1)[i]:.9g} float64 "
                                 f"{r64.reshape(-1)[i]:.9g} fp32 {r32.reshape(-1)[i]:.9g}; max |float64| {np.abs(r64).max():.6g}")
    return worst
