"""The renderer backward (csrc/enarf_render_bwd.hip) entry by entry against a float64 referee (tests/grad_referee.py).

Every gradient entry - feature planes per texel, part-probability planes, z_rend and the 12 StyledMLP leaves through
enarf_prepare_bwd - is held to its own scale: A x the fp32 oracle's own error on that entry + 1e-4 of its magnitude + 1e-6
of the tensor's maximum, where the older tests bound only 1e-3 of each tensor's maximum. The matrix reaches what those tests
do not: both render_bwd_kernel instantiations over ragged fine counts (Nf 2 .. 128), P 23 / 24, style_dim 20 / 256,
render_scale != 1, rays that hit no cube, per-image tri-planes under group_frames, a forced drop_invalid_rays, non-square and
2 x 2 planes, the density modes, a tri-plane shared by three images and the channel-last feature gradient. enarf_query_bwd runs on points placed in
canonical space (long runs of samples on one texel, texel centres and edges, the plane border), enarf_weight_grad and
enarf_prepare_bwd on synthetic inputs. The forward launch of every render case is held entry by entry as well
(tests/fwd_referee.py), on the same referee's float64 and fp32 renders."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fwd_referee as FR
import grad_referee as R
from _helpers import DeviceScene, Scene, assert_close, bits_of
from fwd_cases import query_points as _query_points, rays as _rays
from oracle import enarf_oracle as O

pytestmark = pytest.mark.gpu

ATOMIC_TOL = 2e-5       # of max |gradient|: re-ordered float sums (atomics, split-K partials); tests/test_gpu_backward_sizes.py


def _kernel_grads(ds, coord_d, Nf, bins_d, gc, gm, gd, **kw):
    """enarf_render_bwd (+ enarf_weight_grad) + enarf_prepare_bwd -> {"feat", "mask", "z", *LEAVES} on the device"""
    from enarf_gan_amd import ops
    r = ops.render_bwd(coord_d, ds.inv_K, ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, Nf, bins_d, gc.to(ds.dev),
                       gm.to(ds.dev), gd.to(ds.dev), **kw)
    grad_tri, dW, db = r[:3]
    pg, dz = ops.prepare_bwd(ds.sc.raw["z_rend"].to(ds.dev), ds.mlp, dW)
    out = {"feat": grad_tri[:, :96], "mask": grad_tri[:, 96:], "z": dz}
    for l in range(3):
        out[f"layers.{l}.bias"] = db[l]
        for leaf in ("conv.weight", "conv.modulation.weight", "conv.modulation.bias"):
            out[f"layers.{l}.{leaf}"] = pg[f"layers.{l}.{leaf}"]
    if len(r) == 4:
        out["feat_cl"] = r[3]
    return out


def _case(sc, ids, Nc, Nf, render_scale=1.0, seed=7, modes=None, bwd_kw=None, what=""):
    """Forward (kernel bins, debug taps) + referee + backward on the rays `ids` of every image; returns (ratios, grads,
    context) after every check."""
    modes = modes or {}
    kflags = dict(multiply_density_with_weight=modes.get("multiply_density_with_weight", False),
                  clamp_mask=modes.get("clamp_mask", False), uniform_part_weight=modes.get("no_selector", False))
    ds = DeviceScene(sc)
    B = sc.B
    coord = sc.raw["image_coord"].reshape(B, 3, -1)[..., ids].contiguous()
    n = coord.shape[-1]
    fwd = ds.render(coord, Nc, Nf, None, seed=seed, debug=True, mlp_mode="f32", render_scale=render_scale, **kflags)
    bins = fwd.taps["bins"].cpu()
    g = torch.Generator().manual_seed(Nf + 100 * B)
    gc, gm, gd = torch.randn(B, 3, n, generator=g), torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    tri1 = sc.raw["tri_plane"] if sc.raw["tri_plane"].shape[0] == B else sc.raw["tri_plane"][:1]
    ref = R.referee(sc, coord, Nc, Nf, bins, gc, gm, gd, tri=tri1, render_scale=render_scale, **modes)
    # the kernel takes the fp32 oracle's discrete decisions on every ray
    t32 = ref["taps32"]
    rv = fwd.taps["ray_validity"].cpu().numpy().astype(bool)
    assert (rv == t32["ray_validity"].numpy()).all(), f"{what}: ray validity differs from the oracle's"
    assert (~rv).any() and rv.any(), what
    fv_k, fv_o = fwd.taps["fine_valid"].cpu().numpy().astype(np.uint32), bits_of(t32["fine_valid"])
    march = np.ones_like(rv) if B > 1 else rv            # dropped rays (B == 1) are never marched
    assert (fv_k[march] == fv_o[march]).all(), f"{what}: fine sample validity differs from the oracle's"
    for k in ("depth_min", "depth_max"):                 # the depth range: ends picked from the same 32-depth table
        dk, do = fwd.taps[k].cpu().numpy()[rv], t32[k].numpy()[rv]
        assert np.allclose(dk, do, rtol=1e-6, atol=0), f"{what}: {k} differs from the oracle's"
    keep = ref["keep"]
    assert float(keep.float().mean()) > 0.9, f"{what}: float64 and fp32 disagree on {int((~keep).sum())} of {keep.numel()} rays"
    # forward values against float64: every sample and ray output entry by entry (tests/fwd_referee.py), on the referee's draws
    fwd_ratios = FR.check_forward(FR.kernel_tensors(fwd), FR.from_grad_referee(ref), f"{what}: forward")
    print(f"{what}: forward, worst error / bound per tensor: {FR.fmt(fwd_ratios)}")
    assert float(ref["out64"][1].max()) > 0.3, what
    kd = keep.float()
    ours = _kernel_grads(ds, coord.to(ds.dev), Nf, bins.to(ds.dev), gc * kd[:, None], gm * kd, gd * kd,
                         render_scale=render_scale, **kflags, **(bwd_kw or {}))
    torch.cuda.synchronize()
    ratios = R.check_grads(ours, ref, what)
    print(f"{what}: worst error / bound per tensor: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    return ratios, ours, dict(ds=ds, coord=coord, bins=bins, gc=gc * kd[:, None], gm=gm * kd, gd=gd * kd, ref=ref, kflags=kflags,
                              rv=rv)


# ------------------------------------------------------------------------------------------------ render_bwd, the matrix
@pytest.mark.parametrize("Nf", [2, 3, 16, 17, 33, 64, 65, 127, 128])
def test_render_bwd_fine_counts_vs_float64(Nf):
    """render_bwd_kernel<1> (Nf <= 64) and <2> (each wave recomputes two fine tiles), a ragged last tile for every Nf that is
    not a multiple of 16; 8 rays miss every cube (B = 1: dropped, as the reference drops them)."""
    sc = Scene(32, 1, "center_fixed", 20)
    _case(sc, _rays(32, 40 if Nf <= 64 else 24, 8, Nf), 32, Nf, what=f"Nf {Nf}")


@pytest.mark.parametrize("ol,style_dim,B", [("center+head", 256, 1), ("center_fixed", 256, 2), ("center+head", 20, 2)])
def test_render_bwd_parts_style_and_batch_vs_float64(ol, style_dim, B):
    """P = 24 (center+head) and P = 23, style_dim 20 and 256; B = 2 with per-image tri-planes keeps the rays that hit no cube
    (their upstream gradients reach nothing)."""
    sc = Scene(32, B, ol, style_dim)
    _case(sc, _rays(32, 32, 8, B), 32, 33, what=f"{ol} style {style_dim} B {B}")


@pytest.mark.parametrize("render_scale", [0.5, 2.0])
def test_render_bwd_render_scale_vs_float64(render_scale):
    """render_scale scales every density x delta in the compositing (rendering.py:316-321) and so every d sigma."""
    sc = Scene(32, 1, "center_fixed", 20)
    _case(sc, _rays(32, 40, 4, 3), 32, 48, render_scale=render_scale, what=f"render_scale {render_scale}")


@pytest.mark.parametrize("modes", [dict(clamp_mask=True), dict(multiply_density_with_weight=True),
                                   dict(no_selector=True, multiply_density_with_weight=True)])
def test_render_bwd_density_modes_vs_float64(modes):
    sc = Scene(32, 1, "center_fixed", 20)
    if modes.get("clamp_mask"):
        sc.raw["tri_plane"] = sc.raw["tri_plane"].clone()
        sc.raw["tri_plane"][:, 96:] *= 3.0                  # plane samples beyond [-2, 5]: the straight-through clamp
    ratios, ours, _ = _case(sc, _rays(32, 40, 4, 5), 32, 32, modes=modes, what=str(modes))
    if modes.get("no_selector"):
        assert float(ours["mask"].abs().max()) == 0.0


@pytest.mark.parametrize("H,W", [(24, 40), (2, 2), (2, 5)])
def test_render_bwd_non_square_and_tiny_planes_vs_float64(H, W):
    """Planes resampled from the scene's to H x W: the footprint of a sample is clamped at every border; on 2 x 2 planes the
    four texels take every sample of a ray."""
    sc = Scene(32, 1, "center_fixed", 20)
    sc.raw["tri_plane"] = F.interpolate(sc.raw["tri_plane"], size=(H, W), mode="bilinear", align_corners=False).contiguous()
    _case(sc, _rays(32, 40, 4, H * W), 32, 24, what=f"planes {H}x{W}")


def test_render_bwd_shared_triplane_three_images_vs_float64():
    """One tri-plane (batch 1) for B = 3 images: the three images' atomics land on the same plane."""
    sc = Scene(32, 3, "center_fixed", 20)
    sc.raw["tri_plane"] = sc.raw["tri_plane"][:1].contiguous()
    ratios, ours, _ = _case(sc, _rays(32, 24, 4, 9), 32, 32, what="shared tri-plane B 3")
    assert ours["feat"].shape[0] == 1


def test_render_bwd_feature_gradient_channel_last():
    """feat_grad_channel_last=True: the channel-last feature gradient against the referee, against an NCHW call (another
    atomic order: ATOMIC_TOL), and enarf_triplane_unpack_add of that same result against a torch permute, bit for bit."""
    from enarf_gan_amd import ops
    sc = Scene(32, 1, "center_fixed", 20)
    _, base, c = _case(sc, _rays(32, 40, 4, 19), 32, 32, what="NCHW feature gradient")
    cl = _kernel_grads(c["ds"], c["coord"].to(c["ds"].dev), 32, c["bins"].to(c["ds"].dev), c["gc"], c["gm"], c["gd"],
                       feat_grad_channel_last=True)
    gfeat = cl["feat_cl"]                                               # (B, 3, H, W, 32)
    assert float(cl["feat"].abs().max()) == 0.0                         # not folded into grad_tri
    B, _, H, W, C = gfeat.shape
    perm = gfeat.permute(0, 1, 4, 2, 3).reshape(B, 3 * C, H, W)
    R.check_grads({"feat": perm}, c["ref"], "channel-last feature gradient", names=["feat"])
    assert_close(perm.cpu(), base["feat"].cpu(), "channel-last vs NCHW call", ATOMIC_TOL)
    for k in base:
        if k != "feat":
            assert_close(cl[k].cpu(), base[k].cpu(), f"channel-last call: {k}", ATOMIC_TOL)
    tgt = torch.randn(B, c["ds"].tri.shape[1], H, W, generator=torch.Generator().manual_seed(1)).to(gfeat.device)
    want = tgt.clone()
    want[:, :96] += perm
    ops.triplane_unpack_add(gfeat, tgt)
    assert torch.equal(tgt, want)


def test_render_bwd_group_frames_vs_float64_and_each_other():
    """Per-image tri-planes, B = 3, group_frames 0, 1 and 3: each passes the referee, and they agree with each other to
    the atomic-reorder bound."""
    sc = Scene(32, 3, "center_fixed", 256)
    _, g0, ctx = _case(sc, _rays(32, 24, 4, 11), 32, 40, what="group_frames 0")
    for gf in (1, 3):
        c = ctx
        gg = _kernel_grads(c["ds"], c["coord"].to(c["ds"].dev), 40, c["bins"].to(c["ds"].dev), c["gc"], c["gm"], c["gd"],
                           group_frames=gf)
        R.check_grads(gg, c["ref"], f"group_frames {gf}")
        for k in g0:
            assert_close(gg[k].cpu(), g0[k].cpu(), f"group_frames {gf} vs 0: {k}", ATOMIC_TOL)


def test_render_bwd_drop_invalid_rays_forced():
    """drop_invalid_rays forced on for B = 2 (default: off). A ray that hits no cube has zero weight on every sample, so its
    upstream gradients reach nothing whether it is dropped or marched: the gradients with the flag on equal those with it
    off, and changing the dropped rays' upstream gradients leaves them unchanged - both up to the atomic order. What this
    catches is the compaction of the dropped rays (an index that shifts the kept rays' gradients), not an ignored flag,
    which no gradient can show; the default B = 1 drop (the referee's rule) is checked against float64 above."""
    sc = Scene(32, 2, "center_fixed", 20)
    ds = DeviceScene(sc)
    ids = _rays(32, 32, 16, 13)
    coord = sc.raw["image_coord"].reshape(2, 3, -1)[..., ids].contiguous()
    n = coord.shape[-1]
    fwd = ds.render(coord, 32, 32, None, seed=3, debug=True, mlp_mode="f32", drop_invalid_rays=True)
    rv = fwd.taps["ray_validity"].bool()
    assert (~rv).sum() >= 16 and rv.sum() > 0
    g = torch.Generator().manual_seed(17)
    gc, gm, gd = torch.randn(2, 3, n, generator=g), torch.randn(2, n, generator=g), torch.randn(2, n, generator=g)
    a = _kernel_grads(ds, coord.to(ds.dev), 32, fwd.taps["bins"], gc, gm, gd, drop_invalid_rays=True)
    inv = (~rv).cpu().float()
    b = _kernel_grads(ds, coord.to(ds.dev), 32, fwd.taps["bins"], gc + 5 * inv[:, None], gm - 3 * inv, gd + 7 * inv,
                      drop_invalid_rays=True)
    off = _kernel_grads(ds, coord.to(ds.dev), 32, fwd.taps["bins"], gc, gm, gd, drop_invalid_rays=False)
    for k in a:
        assert float(a[k].abs().max()) > 0 or k == "mask", k
        assert_close(b[k].cpu(), a[k].cpu(), f"dropped rays' upstream gradients changed: {k}", ATOMIC_TOL)
        assert_close(off[k].cpu(), a[k].cpu(), f"drop_invalid_rays on vs off: {k}", ATOMIC_TOL)


# ------------------------------------------------------------------------------------------ query_bwd on placed points
_QUERY_BWD = {}


def query_bwd_case(modes):
    """the scene, placed points, upstream gradients and float64 / fp32 autograd gradients of the query: once per flag set"""
    key = tuple(sorted(modes.items()))
    if key in _QUERY_BWD:
        return _QUERY_BWD[key]
    sc = Scene(32, 2, "center_fixed", 20)
    if modes.get("clamp_mask"):
        sc.raw["tri_plane"] = sc.raw["tri_plane"].clone()
        sc.raw["tri_plane"][:, 96:] *= 3.0
    H, W = sc.raw["tri_plane"].shape[2:]
    pts = torch.stack([_query_points(sc, b, H, W) for b in range(2)]).contiguous()
    N = pts.shape[-1]
    g = torch.Generator().manual_seed(21)
    gD, gC = torch.randn(2, 1, N, generator=g), torch.randn(2, 3, N, generator=g)
    # where the points land (fp32, the kernel's arithmetic): mostly valid for part 5, the far ones for none
    loc, can = O.to_local_and_canonical(pts, sc.pose_scaled, sc.scale, sc.cpose)
    valid = O.validity(loc, can)
    assert bool(valid[:, 5, :-7].all()) and not bool(valid[..., -7:].any())
    for b in range(2):                                        # the runs: one bilinear footprint, then two (fp32 taps)
        for r in range(6):
            u = r // 2
            ix = torch.floor(((can[b, 5, u, 16 * r:16 * r + 16] + 1) * W - 1) / 2)
            assert len(torch.unique(ix)) == (1 if r % 2 == 0 else 2), (b, r, ix)
    grads = {}
    for dt in (torch.float64, torch.float32):
        tri = sc.raw["tri_plane"].to(dt).clone().requires_grad_(True)
        mlp = {q: v.to(dt).clone().requires_grad_(True) for q, v in sc.raw["mlp"].items() if "noise" not in q}
        z = sc.raw["z_rend"].to(dt).clone().requires_grad_(True)
        den, col, _ = O.query(pts.to(dt), sc.pose_scaled.to(dt), sc.scale.to(dt), sc.cpose.to(dt), tri,
                              O.modulated_weights(mlp, z), **modes)
        gr = torch.autograd.grad((den * gD.to(dt)).sum() + (col * gC.to(dt)).sum(), [tri, z] + [mlp[q] for q in R.LEAVES])
        grads[dt] = {"feat": gr[0][:, :96], "mask": gr[0][:, 96:], "z": gr[1], **dict(zip(R.LEAVES, gr[2:]))}
    _QUERY_BWD[key] = (sc, pts, gD, gC, {"g64": grads[torch.float64], "g32": grads[torch.float32]})
    return _QUERY_BWD[key]


def query_bwd_grads(ds, pts_d, gD_d, gC_d, modes):
    """enarf_query_bwd (+ enarf_weight_grad) + enarf_prepare_bwd -> {"feat", "mask", "z", *LEAVES} on the device"""
    from enarf_gan_amd import ops
    kflags = dict(multiply_density_with_weight=modes.get("multiply_density_with_weight", False),
                  clamp_mask=modes.get("clamp_mask", False))
    grad_tri, dW, db = ops.query_bwd(pts_d, ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, gD_d, gC_d, **kflags)
    pg, dz = ops.prepare_bwd(ds.sc.raw["z_rend"].to(ds.dev), ds.mlp, dW)
    ours = {"feat": grad_tri[:, :96], "mask": grad_tri[:, 96:], "z": dz}
    for l in range(3):
        ours[f"layers.{l}.bias"] = db[l]
        for leaf in ("conv.weight", "conv.modulation.weight", "conv.modulation.bias"):
            ours[f"layers.{l}.{leaf}"] = pg[f"layers.{l}.{leaf}"]
    return ours


@pytest.mark.parametrize("modes", [{}, dict(multiply_density_with_weight=True, clamp_mask=True)])
def test_query_bwd_placed_points_vs_float64(modes):
    sc, pts, gD, gC, ref = query_bwd_case(modes)
    ours = query_bwd_grads(DeviceScene(sc), pts.cuda(), gD.cuda(), gC.cuda(), modes)
    ratios = R.check_grads(ours, ref, f"query_bwd {modes}")
    print(f"query_bwd {modes}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ------------------------------------------------------------------------------------------- weight gradients alone
@pytest.mark.parametrize("B,tiles", [(1, [1]), (1, [37]), (3, [23, 0, 61]), (3, [0, 400, 5])])
def test_weight_grad_vs_float64(B, tiles):
    """enarf_weight_grad on synthetic compact rows (x: 32 features, dz3: 4 output gradients; some rows with zero dz3):
    16-row tiles dealt unevenly over the split-K workgroups, an image that exports nothing (exactly zero dW), the
    reduction over the partials - against the same MLP forward + backward in float64."""
    from enarf_gan_amd import ops
    sc = Scene(32, B, "center_fixed", 20)
    ds = DeviceScene(sc)
    rows = 16 * max(tiles) + 32
    g = torch.Generator().manual_seed(sum(tiles))
    x = torch.randn(B, rows, 32, generator=g) * 0.5
    dz3 = torch.randn(B, rows, 4, generator=g)
    dz3[:, ::7] = 0.0
    blocks = torch.tensor(tiles, dtype=torch.int32)
    bufs = {"x": x.cuda().contiguous(), "dz3": dz3.cuda().contiguous()}
    dW, db = ops._weight_grad(bufs, blocks.cuda(), ds.pack, B, rows, ds.dev)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ws = O.modulated_weights({k: v.to(dt) for k, v in sc.raw["mlp"].items()}, sc.raw["z_rend"].to(dt))
        Wl = [w.clone().requires_grad_(True) for w, _ in ws]
        bl = [bb.clone().requires_grad_(True) for _, bb in ws]
        loss = 0
        for b in range(B):
            m = 16 * tiles[b]
            h = x[b, :m].T.to(dt)
            for l in range(3):
                zl = Wl[l][b] @ h + bl[l][:, None]
                h = F.leaky_relu(zl, 0.2) * 2 ** 0.5
            loss = loss + (zl * dz3[b, :m].T.to(dt)).sum()
        gr = torch.autograd.grad(loss, Wl + bl)
        ref[dt] = {**{f"dW{l}": gr[l] for l in range(3)}, **{f"db{l}": gr[3 + l] for l in range(3)}}
    ours = {**{f"dW{l}": dW[l] for l in range(3)}, **{f"db{l}": db[l] for l in range(3)}}
    ratios = R.check_grads(ours, {"g64": ref[torch.float64], "g32": ref[torch.float32]}, f"weight_grad {tiles}")
    print(f"weight_grad {tiles}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for b in range(B):
        if tiles[b] == 0:
            for l in range(3):
                assert float(dW[l][b].abs().max()) == 0.0


@pytest.mark.parametrize("B,style_dim", [(1, 20), (3, 256)])
def test_prepare_bwd_vs_float64(B, style_dim):
    """enarf_prepare_bwd alone: dW' of the demodulated weights -> conv.weight, modulation.{weight,bias} and z_rend, against
    autograd through the oracle's modulated_weights in float64."""
    from enarf_gan_amd import ops
    sc = Scene(32, B, "center_fixed", style_dim)
    g = torch.Generator().manual_seed(B)
    dW = [torch.randn(B, 64, 32, generator=g), torch.randn(B, 64, 64, generator=g), torch.randn(B, 4, 64, generator=g)]
    ref = {}
    for dt in (torch.float64, torch.float32):
        mlp = {k: v.to(dt).clone().requires_grad_(True) for k, v in sc.raw["mlp"].items() if "noise" not in k}
        z = sc.raw["z_rend"].to(dt).clone().requires_grad_(True)
        ws = O.modulated_weights(mlp, z)
        loss = sum((ws[l][0] * dW[l].to(dt)).sum() for l in range(3))
        keys = [k for k in R.LEAVES if not k.endswith(".bias") or "modulation" in k]
        gr = torch.autograd.grad(loss, [z] + [mlp[k] for k in keys])
        ref[dt] = {"z": gr[0], **dict(zip(keys, gr[1:]))}
    pg, dz = ops.prepare_bwd(sc.raw["z_rend"].cuda(), {k: v.cuda() for k, v in sc.raw["mlp"].items()}, [d.cuda() for d in dW])
    ours = {"z": dz, **{k: pg[k] for k in ref[torch.float64] if k != "z"}}
    ratios = R.check_grads(ours, {"g64": ref[torch.float64], "g32": ref[torch.float32]}, f"prepare_bwd B {B}")
    print(f"prepare_bwd B {B}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
