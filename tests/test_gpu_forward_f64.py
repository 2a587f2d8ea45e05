"""The forward march (render_kernel / march_kernel, csrc/enarf_render.hip) entry by entry against a float64 referee
(tests/fwd_referee.py): every sample's coarse and fine density, colour, depth and weight and every ray's colour, mask and
disparity is held to its own scale - A x the fp32 oracle's own error on that entry + a few ulp of its magnitude + 1e-9 of the
tensor's maximum - where the older forward tests bound 1e-4 of each tensor's maximum and compare the per-sample colour with
nothing. The cases (tests/fwd_cases.py) run in all four MLP modes, each under both march kernels; a case's referee (four
yardstick amplitudes) is computed once and shared by its eight launches. `f32` and `f16x3` are held by check_forward, the
two bf16 modes in stages by check_forward_staged (the densities against a yardstick taken before the ReLU), and every
launch's compositing by check_composite on its own per-sample results. enarf_query_fwd is held to the same bounds on points
placed in canonical space."""
import numpy as np
import pytest
import torch

import fwd_cases as FC
import fwd_referee as FR
import grad_referee as R
from _helpers import DeviceScene, Scene, bits_of
from oracle import enarf_oracle as O

pytestmark = pytest.mark.gpu

_CASES = {}


@pytest.fixture(scope="module")
def ops():
    from enarf_gan_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def _case(name):
    """the case, its referee (one yardstick per mode) and its device scene: built once per module"""
    if name not in _CASES:
        c = FC.build(name)
        ref = FR.referee(c["sc"], c["coord"], c["Nc"], c["Nf"], c["bins"], render_scale=c["render_scale"],
                         amplitudes=sorted(set(FR.MODE_ULPS.values())), **c["modes"])
        _CASES[name] = (c, ref, DeviceScene(c["sc"]))
    return _CASES[name]


def assert_decisions(fwd, ref, what):
    """the kernel takes the fp32 oracle's discrete decisions on every ray: ray validity, the fine samples' part bit masks, the
    depth range (ends picked from the same 32-depth table)"""
    t32 = ref["taps32"]
    rv = fwd.taps["ray_validity"].cpu().numpy().astype(bool)
    assert (rv == t32["ray_validity"].numpy()).all(), f"{what}: ray validity differs from the oracle's"
    fv_k, fv_o = fwd.taps["fine_valid"].cpu().numpy().astype(np.uint32), bits_of(t32["fine_valid"])
    live = ref["live"]
    assert (fv_k[live] == fv_o[live]).all(), f"{what}: fine sample validity differs from the oracle's"
    for k in ("depth_min", "depth_max"):
        dk, do = fwd.taps[k].cpu().numpy()[rv], t32[k].numpy()[rv]
        assert np.allclose(dk, do, rtol=1e-6, atol=0), f"{what}: {k} differs from the oracle's"
    return rv


def assert_dropped_rays_are_zero(fwd, ref, what):
    """one image: a ray that hits no cube is dropped - exact zeros in every output"""
    dead = torch.from_numpy(~ref["live"])
    if not bool(dead.any()):
        return 0
    for k in ("color", "mask", "disparity", "fine_weights", "fine_depth"):
        t = getattr(fwd, k).cpu()
        t = t[:, 0] if k.startswith("fine_") else t
        v = t.permute(0, 2, 1)[dead] if k == "color" else t[dead]
        assert float(v.abs().max()) == 0.0, f"{what}: {k} of a dropped ray is not zero"
    return int(dead.sum())


_RAY = {}       # (case, mode) -> tensors of the bf16-mode launch under march "ray", for the bit comparison of "task"


def _launch(ds, c, mode, march):
    return ds.render(c["coord"], c["Nc"], c["Nf"], c["bins"], mlp_mode=mode, march=march, debug=True,
                     render_scale=c["render_scale"], **c["kflags"])


@pytest.mark.parametrize("march", ["ray", "task"])
@pytest.mark.parametrize("mode", list(FR.MODE_ULPS))
@pytest.mark.parametrize("name", list(FC.CASES))
def test_forward_march_vs_float64(ops, name, mode, march):
    """render_kernel<0|1|2|3, 1|2> (march "ray") and march_kernel<0|1|2|3, 1|2, 12> ("task") on every case of
    tests/fwd_cases.py. Worst error / bound on the MI355X: DESIGN 4, profiles/r20_forward_modes.log."""
    c, ref, ds = _case(name)
    what = f"{name} {mode} {march}"
    fwd = _launch(ds, c, mode, march)
    torch.cuda.synchronize()
    rv = assert_decisions(fwd, ref, what)
    keep = ref["keep"]
    assert keep.mean() >= 0.9 and (keep & rv).sum() >= 16 and (~rv).any(), what
    if c["sc"].B == 1:
        assert assert_dropped_rays_are_zero(fwd, ref, what) > 0
    ours = FR.kernel_tensors(fwd)
    if mode in FR.STAGED:
        worst = FR.check_forward_staged(ours, ref, mode, what)
        if march == "ray":
            _RAY[(name, mode)] = ours
        else:           # the two marches share every stage: the same bits on every compared tensor (launched here if run alone)
            ray = _RAY.get((name, mode)) or FR.kernel_tensors(_launch(ds, c, mode, "ray"))
            for k in FR.NAMES:
                assert np.array_equal(ours[k], ray[k]), f"{what}: {k} differs from march ray's"
    else:
        worst = FR.check_forward(ours, ref, what, ulps=FR.MODE_ULPS[mode])
        worst.update({"composite." + k: v for k, v in FR.check_composite(ours, ref, what).items()})
    print(f"{what}: worst error / bound per tensor: {FR.fmt(worst)}")


# -------------------------------------------------------------------------------------------- query_fwd on placed points
def _query_tensors(den, col, weight, canonical, signed=None):
    t = {"density": FR._np(den)[:, 0], "color": FR._np(col).transpose(0, 2, 1), "weight": FR._np(weight).transpose(0, 2, 1),
         "canonical": FR._np(canonical).transpose(0, 3, 1, 2)}             # the point axis second; colour (B, N, 3) one group
    if signed is not None:
        t["signed_density"] = FR._np(signed)[:, 0]                         # an oracle's: the yardstick of the bf16 modes
    return t


def _oracle_query(sc, pts, dt, modes):
    s = sc.raw
    with torch.no_grad():
        mlp = {q: v.to(dt) for q, v in s["mlp"].items() if "noise" not in q}
        den, col, valid, taps = O.query(pts.to(dt), sc.pose_scaled.to(dt), sc.scale.to(dt), sc.cpose.to(dt), s["tri_plane"].to(dt),
                                        O.modulated_weights(mlp, s["z_rend"].to(dt)), return_taps=True, **modes)
    return _query_tensors(den, col, taps["weight"], taps["canonical"], taps["signed_density"]), valid


_QUERY = {}


def _query_ref(clamp):
    """points, float64 referee, fp32 oracle and its draws per amplitude for the placed points: once per flag set"""
    if clamp not in _QUERY:
        modes = dict(multiply_density_with_weight=True, clamp_mask=True) if clamp else {}
        sc = Scene(32, 2, "center_fixed", 20)
        if clamp:
            sc.raw["tri_plane"] = sc.raw["tri_plane"].clone()
            sc.raw["tri_plane"][:, 96:] *= 3.0
        H, W = sc.raw["tri_plane"].shape[2:]
        pts = torch.stack([FC.query_points(sc, b, H, W) for b in range(2)]).contiguous()
        t64, v64 = _oracle_query(sc, pts, torch.float64, modes)
        t32, v32 = _oracle_query(sc, pts, torch.float32, modes)
        draws = {u: [_oracle_query((FR.operand_scene if u in FR.OPERAND_ULPS else R.perturbed_scene)(sc, i, u), pts,
                                   torch.float32, modes)[0] for i in range(FR.DRAWS)] for u in sorted(set(FR.MODE_ULPS.values()))}
        keep = (v64 == v32).all(1).numpy()                               # (B, N): points on which validity agrees
        _QUERY[clamp] = (sc, pts, modes, t64, t32, draws, keep, v32)
    return _QUERY[clamp]


@pytest.mark.parametrize("mode", list(FR.MODE_ULPS))
@pytest.mark.parametrize("clamp", [False, True])
def test_query_fwd_placed_points_vs_float64(ops, clamp, mode):
    """enarf_query_fwd's (query_kernel<0|1|2|3, true>) density, colour, part probabilities and canonical coordinates, entry
    by entry, on the points of test_gpu_backward_f64.test_query_bwd_placed_points_vs_float64: texel centres and edges, the
    plane border, the faces of the valid region, points far from every part. In the bf16 modes the density's yardstick is
    taken on the signed density and a point inside no part's cube is zero exactly (fwd_referee.check_samples)."""
    sc, pts, modes, t64, t32, draws, keep, v32 = _query_ref(clamp)
    assert keep.mean() > 0.9 and bool(v32[:, 5, :-7].all()) and not bool(v32[..., -7:].any())
    ds = DeviceScene(sc)
    den, col, vb, dc, dw = ds.query(pts, mlp_mode=mode, debug=True, **modes)
    torch.cuda.synchronize()
    worst = check_query(den, col, vb, dc, dw, clamp, mode)
    print(f"query_fwd {mode} {modes}: worst error / bound per tensor: {FR.fmt(worst)}")


def check_query(den, col, vb, dc, dw, clamp, mode):
    """the outputs of query_fwd(debug=True) on _query_ref(clamp)'s points against its referee -> worst error / bound per tensor"""
    sc, pts, modes, t64, t32, draws, keep, v32 = _query_ref(clamp)
    assert np.array_equal(vb.cpu().numpy().view(np.uint32), bits_of(v32)), "validity bit masks differ from the oracle's"
    ours = _query_tensors(den, col, dw, dc)
    in_a_part = v32.any(1).numpy()
    worst = {}
    for k in ours:
        y = "signed_density" if (k == "density" and mode in FR.STAGED) else k
        ulps = FR.MODE_ULPS[mode] if k in ("density", "color") else (1 if mode in FR.STAGED else FR.MODE_ULPS[mode])   # no bf16 split in front of them
        rt = FR.bound_ratios(k, ours[k], t64[k], [t32[y]] + [d[y] for d in draws[ulps]], keep, grouped=(k == "color"), yard64=t64[y])
        if y != k:
            rt = np.where(in_a_part, rt, np.where(ours[k] == 0, 0.0, np.inf))
        rt = np.where(keep.reshape(keep.shape + (1,) * (rt.ndim - 2)), rt, 0.0)
        worst[k] = float(rt.max())
        i = np.unravel_index(int(np.argmax(rt)), rt.shape)
        assert worst[k] <= 1.0, (f"query {mode} {modes}: {k}: entry {tuple(int(j) for j in i)} is {worst[k]:.3g}x its bound, "
                                 f"{int((rt > 1).sum())} above; ours {ours[k][i]} float64 {t64[k][i]} fp32 {t32[k][i]}")
    return worst
