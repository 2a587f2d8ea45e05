"""The cases of tests/test_gpu_poison.py and the map from the C ABI of the HIP libraries to them.

POISON_CASES: every function a public header declares (libraries.declared, over every row of build.LIBRARIES and
build.SIDE_LIBRARIES) -> the names of the cases below that call it; HOST_ONLY: the functions that launch nothing, each with
its reason; INDIRECT: functions no Python wrapper calls, reached from inside another entry point; NOT_RUN: entry points left
out because a poisoned run faulted or hung and the cause was not found (none so far). tests/test_poison_cpu.py requires the
three sets and the map to account for every declared function, so a new entry point fails there until it has a case.

A case takes no arguments, builds its inputs, snapshots them (_begin), calls the public Python wrapper and returns
(inputs, outputs, check): `outputs` maps a name to every tensor the wrapper returned, `check(outputs)` holds them to the
restatement the library's own GPU test uses, at that test's tolerance (imported, never copied). `check.atomic` names the
outputs accumulated with float atomics: two runs of those agree to ATOMIC_TOL (tests/test_gpu_backward_f64.py), all others bit
for bit. The shapes are the smallest with a ragged tail in every tiled extent."""
import numpy as np
import torch

from enarf_gan_amd import build

ALL_STEMS = list(build.ALL_LIBRARIES)
SNAPSHOT = {}


def _begin(inputs):
    """clones of the inputs, taken before the wrapper is called: the test compares the inputs with them afterwards"""
    SNAPSHOT.clear()
    SNAPSHOT.update({k: t.detach().clone() for k, t in inputs.items()})
    return inputs


def _d(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: shared case tables are read-only


def _checked(fn, atomic=()):
    fn.atomic = frozenset(atomic)
    return fn


# ================================================================================================= libenarf_hip.so
# ---- the march: enarf_prepare, enarf_triplane_pack, enarf_render_fwd, enarf_render_bwd, enarf_weight_grad, enarf_prepare_bwd
_MARCH = {}


def _march_ref(name):
    """the case of tests/fwd_cases.py, upstream gradients and the float64 referee of forward and backward: once per name"""
    if name not in _MARCH:
        import fwd_cases as FC
        import grad_referee as R
        c = FC.build(name)
        B, n = c["coord"].shape[0], c["coord"].shape[-1]
        g = torch.Generator().manual_seed(c["Nf"] + 100 * B)
        gc, gm, gd = torch.randn(B, 3, n, generator=g), torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
        ref = R.referee(c["sc"], c["coord"], c["Nc"], c["Nf"], c["bins"], gc, gm, gd, render_scale=c["render_scale"], **c["modes"])
        kd = ref["keep"].float()
        _MARCH[name] = (c, ref, (gc * kd[:, None], gm * kd, gd * kd))
    return _MARCH[name]


def _clear_render_workspace():
    """the cached render workspace (ops._render_workspace: per stream, only grows) is allocated again by the next call"""
    from enarf_gan_amd import ops
    ops._render_ws.clear()
    ops._render_epoch.clear()
    ops._render_shape.clear()


def _fwd_tensors(prefix, fwd):
    out = {prefix + k: getattr(fwd, k) for k in ("color", "mask", "disparity", "fine_weights", "fine_depth")}
    out.update({prefix + "taps." + k: v for k, v in fwd.taps.items()})
    return out


class _Fwd:
    """RenderOutputs again, from the names of _fwd_tensors"""

    def __init__(self, out, prefix):
        for k in ("color", "mask", "disparity", "fine_weights", "fine_depth"):
            setattr(self, k, out[prefix + k])
        self.taps = {k[len(prefix) + 5:]: v for k, v in out.items() if k.startswith(prefix + "taps.")}


def _check_march(name, what):
    import fwd_referee as FR
    import grad_referee as R
    from test_gpu_forward_f64 import assert_decisions, assert_dropped_rays_are_zero
    c, ref, _ = _march_ref(name)
    fref = FR.from_grad_referee(ref, c["render_scale"])

    def check(out):
        for prefix in ("first.", "second."):           # the two launches use the workspace's two queue headers
            fwd = _Fwd(out, prefix)
            rv = assert_decisions(fwd, fref, what)
            assert fref["keep"].mean() >= 0.9 and (fref["keep"] & rv).sum() >= 16 and (~rv).any(), what
            if c["sc"].B == 1:
                assert assert_dropped_rays_are_zero(fwd, fref, what) > 0
            ours = FR.kernel_tensors(fwd)
            FR.check_forward(ours, fref, what + " " + prefix)
            FR.check_composite(ours, fref, what + " " + prefix)
        grads = {k[5:]: v for k, v in out.items() if k.startswith("grad.")}
        if grads:
            R.check_grads(grads, ref, what)
    return check


def _march(name, march, backward):
    from _helpers import DeviceScene
    from test_gpu_backward_f64 import _kernel_grads
    c, ref, ups = _march_ref(name)
    _clear_render_workspace()
    ds = DeviceScene(c["sc"])                        # enarf_prepare and enarf_triplane_pack
    dev = ds.dev
    inputs = _begin(dict(coord=c["coord"].to(dev), bins=c["bins"].to(dev), tri=ds.tri, feat_cl=ds.feat_cl, parts=ds.parts,
                         pack=ds.pack, inv_K=ds.inv_K, cpose=ds.cpose, gc=ups[0].to(dev), gm=ups[1].to(dev), gd=ups[2].to(dev)))
    kw = dict(mlp_mode="f32", march=march, debug=True, render_scale=c["render_scale"], **c["kflags"])
    out = _fwd_tensors("first.", ds.render(inputs["coord"], c["Nc"], c["Nf"], inputs["bins"], **kw))
    out.update(_fwd_tensors("second.", ds.render(inputs["coord"], c["Nc"], c["Nf"], inputs["bins"], **kw)))
    atomic = []
    if backward:
        g = _kernel_grads(ds, inputs["coord"], c["Nf"], inputs["bins"], inputs["gc"], inputs["gm"], inputs["gd"],
                          render_scale=c["render_scale"], **c["kflags"])
        out.update({"grad." + k: v for k, v in g.items()})
        atomic = ["grad." + k for k in g]            # atomics into the planes; the weight gradients' rows follow their order
    return inputs, out, _checked(_check_march(name, f"{name} {march}"), atomic)


def march_ray_nc33_nf17():
    """render_kernel<0, 1>: ragged coarse and fine tiles, 8 of the 48 rays dropped; then the backward on the same rays"""
    return _march("nc33_nf17", "ray", True)


def march_task_nc33_nf17():
    """march_kernel<0, 1, 12> on the same rays"""
    return _march("nc33_nf17", "task", False)


def march_ray_b2_style256():
    """B = 2 with per-image tri-planes: the rays that miss every cube are marched; the backward on the same rays"""
    return _march("b2_style256", "ray", True)


def march_task_b2_style256():
    return _march("b2_style256", "task", False)


def render_step_nc33_nf17():
    """enarf_render_step_fwd: re-layout, prepare and ray set-up in one launch, then the march, into poisoned parts, pack and
    channel-last planes; against the same referee, and the pre-march launch's three results against the separate calls'"""
    from _helpers import DeviceScene
    from enarf_gan_amd import ops
    c, ref, _ = _march_ref("nc33_nf17")
    sc, s = c["sc"], c["sc"].raw
    _clear_render_workspace()
    d = torch.device("cuda:0")
    mlp = {k: v.to(d) for k, v in s["mlp"].items()}
    inputs = _begin(dict(pose=s["pose_to_camera"].to(d), bl=s["bone_length"].to(d), cbl=sc.cbl.to(d), z=s["z_rend"].to(d),
                         coord=c["coord"].to(d), inv_K=s["inv_intrinsics"].to(d), cpose=sc.cpose.to(d),
                         tri=s["tri_plane"].to(d).contiguous(), bins=c["bins"].to(d), **{"mlp." + k: v for k, v in mlp.items()}))
    feat = torch.empty(1, 3, *inputs["tri"].shape[2:], 32, device=d)
    out = {}
    for prefix in ("first.", "second."):
        st = ops.RenderStep(inputs["pose"], inputs["bl"], inputs["cbl"], inputs["z"], mlp, s["parents"], sc.ol, sc.cs,
                            inputs["coord"], inputs["inv_K"], inputs["cpose"], inputs["tri"], feat, c["Nc"], c["Nf"],
                            bins=inputs["bins"], debug=True, mlp_mode="f32", render_scale=c["render_scale"], **c["kflags"])
        out.update(_fwd_tensors(prefix, st.run()))
    out.update(parts=st.parts, pack=st.pack, feat_cl=feat)
    march_check = _check_march("nc33_nf17", "render_step nc33_nf17")

    def check(o):
        march_check(o)
        ds = DeviceScene(sc)
        assert torch.equal(o["parts"], ds.parts) and torch.equal(o["pack"], ds.pack) and torch.equal(o["feat_cl"], ds.feat_cl)
    return inputs, out, _checked(check)


# ---- enarf_prepare, enarf_mlp_unpack, enarf_prepare_bwd
def prepare_and_unpack():
    """tests/test_gpu_parity.py::test_prepare_matches_oracle on its smallest scene (P = 24, style_dim 20)"""
    from _helpers import Scene, assert_close
    from enarf_gan_amd import ops
    from test_gpu_parity import MODULATED_WEIGHT_RTOL
    sc = Scene(32, 1, "center+head", 20)
    s, d = sc.raw, torch.device("cuda:0")
    mlp = {k: v.to(d) for k, v in s["mlp"].items()}
    inputs = _begin(dict(pose=s["pose_to_camera"].to(d), bl=s["bone_length"].to(d), cbl=sc.cbl.to(d), z=s["z_rend"].to(d),
                         **{"mlp." + k: v for k, v in mlp.items()}))
    parts, pack = ops.prepare(inputs["pose"], inputs["bl"], inputs["cbl"], inputs["z"], mlp, s["parents"], sc.ol, sc.cs)
    pack_only = ops.prepare_mlp(inputs["z"], mlp)
    dense = ops.mlp_unpack(pack[0])
    out = dict(parts=parts, pack=pack, pack_only=pack_only, **{f"dense{i}": t for i, t in enumerate(dense)})

    def check(o):
        p = o["parts"].cpu()
        assert torch.equal(p[:, :, :9], sc.pose_scaled[:, :, :3, :3].reshape(1, sc.P, 9)), "part rotations must be copied exactly"
        assert torch.equal(p[:, :, 9:12], sc.pose_scaled[:, :, :3, 3]), "scaled part translations must be bit-exact"
        assert torch.equal(p[:, :, 12], sc.scale), "canonical scale must be bit-exact"
        assert torch.equal(o["pack_only"], o["pack"])
        for l, (w, bias) in enumerate(sc.weights()):
            assert_close(o[f"dense{l}"].cpu(), w[0], "modulated weight", MODULATED_WEIGHT_RTOL)
            assert torch.equal(o[f"dense{3 + l}"].cpu(), bias)
    return inputs, out, _checked(check)


def prepare_bwd_b3_style256():
    """tests/test_gpu_backward_f64.py::test_prepare_bwd_vs_float64, B = 3 (the per-image results are summed), style_dim 256"""
    import grad_referee as R
    from _helpers import Scene
    from enarf_gan_amd import ops
    from oracle import enarf_oracle as O
    B = 3
    sc = Scene(32, B, "center_fixed", 256)
    g = torch.Generator().manual_seed(B)
    dW = [torch.randn(B, 64, 32, generator=g), torch.randn(B, 64, 64, generator=g), torch.randn(B, 4, 64, generator=g)]
    mlp = {k: v.cuda() for k, v in sc.raw["mlp"].items()}
    inputs = _begin(dict(z=sc.raw["z_rend"].cuda(), dW0=dW[0].cuda(), dW1=dW[1].cuda(), dW2=dW[2].cuda(),
                         **{"mlp." + k: v for k, v in mlp.items()}))
    pg, dz = ops.prepare_bwd(inputs["z"], mlp, [inputs["dW0"], inputs["dW1"], inputs["dW2"]])
    out = {"z": dz, **pg}

    def check(o):
        ref = {}
        for dt in (torch.float64, torch.float32):
            leaves = {k: v.to(dt).clone().requires_grad_(True) for k, v in sc.raw["mlp"].items() if "noise" not in k}
            z = sc.raw["z_rend"].to(dt).clone().requires_grad_(True)
            ws = O.modulated_weights(leaves, z)
            loss = sum((ws[l][0] * dW[l].to(dt)).sum() for l in range(3))
            keys = [k for k in R.LEAVES if not k.endswith(".bias") or "modulation" in k]
            gr = torch.autograd.grad(loss, [z] + [leaves[k] for k in keys])
            ref[dt] = {"z": gr[0], **dict(zip(keys, gr[1:]))}
        assert set(o) == set(ref[torch.float64])
        R.check_grads(o, {"g64": ref[torch.float64], "g32": ref[torch.float32]}, "prepare_bwd B 3")
    return inputs, out, _checked(check)


# ---- enarf_query_fwd, enarf_query_bwd
def query_fwd_placed_points():
    """tests/test_gpu_forward_f64.py::test_query_fwd_placed_points_vs_float64: B = 2, N % 64 != 0, with every optional output"""
    from _helpers import DeviceScene
    from test_gpu_forward_f64 import _query_ref, check_query
    sc, pts = _query_ref(False)[:2]
    assert pts.shape[-1] % 64 != 0
    ds = DeviceScene(sc)
    inputs = _begin(dict(pts=pts.cuda(), parts=ds.parts, pack=ds.pack, tri=ds.tri, feat_cl=ds.feat_cl, cpose=ds.cpose))
    den, col, vb, dc, dw = ds.query(inputs["pts"], mlp_mode="f32", debug=True)
    plain = ds.query(inputs["pts"], mlp_mode="f32")                      # density and colour alone: no optional output
    out = dict(density=den, color=col, valid_bits=vb, canonical=dc, weight=dw, plain_density=plain[0], plain_color=plain[1])

    def check(o):
        check_query(o["density"], o["color"], o["valid_bits"], o["canonical"], o["weight"], False, "f32")
        assert torch.equal(o["plain_density"], o["density"]) and torch.equal(o["plain_color"], o["color"])
    return inputs, out, _checked(check)


def query_fwd_lattice():
    """enarf_query_fwd with points == NULL: the 5^3 lattice of create_mesh generated in the kernel (125 points), density
    alone, against the same points as a tensor (bit for bit) and the oracle (tests/test_gpu_api.py's density sweep)"""
    from _helpers import DeviceScene, Scene, assert_close
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NARF.mesh_rendering import _grid_chunk
    from oracle import enarf_oracle as O
    sc = Scene(32, 1, "center_fixed", 20)
    ds = DeviceScene(sc)
    D = 5
    center = torch.tensor([0.02, -0.03, 1.0]) + sc.pose_parts[0, :, :3, 3].mean(0) - torch.tensor([0.0, 0.0, 1.0])
    inputs = _begin(dict(parts=ds.parts, pack=ds.pack, tri=ds.tri, feat_cl=ds.feat_cl, cpose=ds.cpose))
    den, col = ops.query_fwd(None, ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, need_color=False, grid=(D, center.tolist(), sc.cs))
    assert col is None
    pts = _grid_chunk(D, 0, D ** 3, center, sc.cs, ds.dev)
    same, _ = ds.query(pts, need_color=False)

    def check(o):
        assert o["density"].shape == (1, 1, D ** 3) and torch.equal(o["density"], o["density_of_points"])
        want, _, valid = O.query(pts.cpu(), sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], sc.weights())
        assert int(valid.any(dim=1).sum()) > 5
        assert_close(o["density"].cpu().reshape(-1), want.reshape(-1), "lattice density")
    return inputs, dict(density=den, density_of_points=same), _checked(check)


def query_bwd_placed_points():
    """tests/test_gpu_backward_f64.py::test_query_bwd_placed_points_vs_float64"""
    import grad_referee as R
    from _helpers import DeviceScene
    from test_gpu_backward_f64 import query_bwd_case, query_bwd_grads
    sc, pts, gD, gC, ref = query_bwd_case({})
    ds = DeviceScene(sc)
    inputs = _begin(dict(pts=pts.cuda(), gD=gD.cuda(), gC=gC.cuda(), parts=ds.parts, pack=ds.pack, tri=ds.tri, feat_cl=ds.feat_cl))
    out = query_bwd_grads(ds, inputs["pts"], inputs["gD"], inputs["gC"], {})
    return inputs, out, _checked(lambda o: R.check_grads(o, ref, "query_bwd"), out)


# ---- the tri-plane sampler: enarf_triplane_sample_fwd / _bwd / _ex_fwd / _ex_bwd
def _sampler(C, ws):
    import sampler_reference as R
    from test_gpu_sampler_referee import PADS, _hold
    H, W, h, w = 24, 40, 7, 11
    grid = R.structured_grid(H, W, 2, 23, h * w)
    assert grid.shape == (2, h * w, 3)
    inp, go = R.random_f32((2, 3 * C, H, W), 10), R.random_f32((2, C, h * w), 11)
    from enarf_gan_amd import ops
    inputs = _begin(dict(inp=_d(inp), grid=_d(grid).reshape(2, h, w, 3), go=_d(go).reshape(2, C, h, w)))
    out = {}
    for padding in range(3):
        p = PADS[padding]
        out[f"{p}.out"] = ops.triplane_sample_fwd(inputs["inp"], inputs["grid"], 0, padding, False, use_workspace=ws)
        out[f"{p}.grad_input"], out[f"{p}.grad_grid"] = ops.triplane_sample_bwd(inputs["go"], inputs["inp"], inputs["grid"], 0, padding,
                                                                                 False, True, True, use_workspace=ws)
    only = ops.triplane_sample_bwd(inputs["go"], inputs["inp"], inputs["grid"], 0, 0, False, False, True, use_workspace=ws)
    assert only[0] is None
    out["zeros.grad_grid_alone"] = only[1]

    def check(o):
        for padding in range(3):
            p = PADS[padding]
            _hold(f"C={C} ws={ws} {p} fwd", o[f"{p}.out"], *R.sample(inp, grid, R.BILINEAR, padding, False))
            g = R.sample_grads(go, inp, grid, R.BILINEAR, padding, False)
            _hold(f"C={C} ws={ws} {p} grad_input", o[f"{p}.grad_input"], g["grad_input"], g["gi_S"], g["gi_k"])
            _hold(f"C={C} ws={ws} {p} grad_grid", o[f"{p}.grad_grid"], g["grad_grid"], g["gg_S"], g["gg_k"])
            if padding == 0:
                _hold(f"C={C} ws={ws} grad_grid alone", o["zeros.grad_grid_alone"], g["grad_grid"], g["gg_S"], g["gg_k"])
    return inputs, out, _checked(check, [f"{p}.grad_input" for p in PADS])


def sampler_c32_workspace():
    """pack_kernel<32> + sample_fwd_cl<4>, sample_bwd_cl32 + unpack_add_kernel: planes 24 x 40, 7 x 11 points, B = 2"""
    return _sampler(32, True)


def sampler_c5_direct():
    """sample_fwd_direct / sample_bwd_direct: C = 5 has no channel-last form and takes no workspace"""
    return _sampler(5, False)


def _sampler_ex(separate):
    import sampler_reference as R
    from enarf_gan_amd import ops
    from test_gpu_sampler_referee import _hold, _point_image_case
    inp, grid, ids, off = _point_image_case()
    C, n = inp.shape[1] // 3, grid.shape[1]
    go = R.random_f32((1, 3, C, n) if separate else (1, C, n), 7)
    inputs = _begin(dict(inp=_d(inp), grid=_d(grid), ids=_d(ids), go=_d(go)))
    fwd = ops.triplane_sample_ex_fwd(inputs["inp"], inputs["grid"], separate=separate, point_image=inputs["ids"])
    gi, gg = ops.triplane_sample_ex_bwd(inputs["go"], inputs["inp"], inputs["grid"], separate, inputs["ids"], True, True)

    def check(o):
        _hold(f"ex fwd separate={separate}", o["out"], *R.sample(inp, grid, R.BILINEAR, R.ZEROS, False, separate=separate, point_image=ids))
        assert not o["out"].cpu().numpy()[..., off].any()
        g = R.sample_grads(go, inp, grid, R.BILINEAR, R.ZEROS, False, separate=separate, point_image=ids)
        _hold(f"ex bwd separate={separate} grad_input", o["grad_input"], g["grad_input"], g["gi_S"], g["gi_k"])
        _hold(f"ex bwd separate={separate} grad_grid", o["grad_grid"], g["grad_grid"], g["gg_S"], g["gg_k"])
        assert not o["grad_grid"].cpu().numpy()[0, off].any()
    return inputs, dict(out=fwd, grad_input=gi, grad_grid=gg), _checked(check, ["grad_input"])


def sampler_ex_separate():
    """sample_fwd_direct<true> and sample_bwd_direct's `separate` branch with per-point image ids, some outside the batch"""
    return _sampler_ex(True)


def sampler_ex_point_image():
    return _sampler_ex(False)


# ---- enarf_triplane_pack, enarf_triplane_unpack_add, enarf_triplane_warp_fwd / _bwd
def pack_and_unpack_add():
    """pack_kernel / unpack_add_kernel on 24 x 40 planes, B = 2: a pure permutation and its inverse added in place"""
    from enarf_gan_amd import ops
    g = torch.Generator().manual_seed(0)
    tri = torch.randn(2, 96 + 6, 24, 40, generator=g)
    grad_cl = torch.randn(2, 3, 24, 40, 32, generator=g)
    base = torch.randn(2, 96 + 6, 24, 40, generator=g)
    inputs = _begin(dict(tri=tri.cuda(), grad_cl=grad_cl.cuda()))
    cl = ops.triplane_pack(inputs["tri"])
    acc = ops.triplane_unpack_add(inputs["grad_cl"], base.cuda())

    def check(o):
        assert torch.equal(o["feat_cl"].cpu(), tri[:, :96].reshape(2, 3, 32, 24, 40).permute(0, 1, 3, 4, 2))
        want = base.clone()
        want[:, :96] += grad_cl.permute(0, 1, 4, 2, 3).reshape(2, 96, 24, 40)
        assert torch.equal(o["accumulated"].cpu(), want)
    return inputs, dict(feat_cl=cl, accumulated=acc), _checked(check)


def warp_5x7():
    """warp_fwd_kernel / warp_bwd_kernel: H W = 35, no multiple of 32 nor of 8, B = 2 (test_warp_on_decisions_and_tails)"""
    import sampler_reference as R
    from enarf_gan_amd import ops
    from test_gpu_sampler_referee import _hold
    B, C, H, W = 2, 32, 5, 7
    rng = np.random.default_rng(H * W)
    flow = (3.0 * rng.standard_normal((B, 6, H, W))).astype(np.float32)
    kind = rng.integers(0, 8, flow.shape)
    flow = np.where(kind == 0, np.rint(flow), flow)
    flow = np.where(kind == 1, np.rint(flow) + 0.5, flow)
    flow = np.where(kind == 2, flow - (max(H, W) + 2), flow)
    flow = np.where(kind == 3, flow + (max(H, W) + 2), flow).astype(np.float32)
    src, go = R.random_f32((3, H, W, C), 16), R.random_f32((B, 3, H, W, C), 17)
    inputs = _begin(dict(src=_d(src)[None], flow=_d(flow), go=_d(go)))
    fwd = ops.triplane_warp_fwd(inputs["src"], inputs["flow"])
    gs, gf = ops.triplane_warp_bwd(inputs["go"], inputs["src"], inputs["flow"])
    only = ops.triplane_warp_bwd(inputs["go"], inputs["src"], inputs["flow"], need_src=False)
    assert only[0] is None

    def check(o):
        _hold("warp fwd", o["out"], *R.warp(src, flow))
        g = R.warp_grads(go, src, flow)
        _hold("warp g_src", o["g_src"], g["g_src"], g["gs_S"], g["gs_k"])
        _hold("warp g_flow", o["g_flow"], g["g_flow"], g["gf_S"], g["gf_k"])
        _hold("warp g_flow alone", o["g_flow_alone"], g["g_flow"], g["gf_S"], g["gf_k"])
    return inputs, dict(out=fwd, g_src=gs, g_flow=gf, g_flow_alone=only[1]), _checked(check, ["g_src"])


# ---- enarf_mask_dilate_topk
def mask_topk_19x23():
    """window_max_kernel + topk_select_kernel: a 19 x 23 mask, k = 37, B = 2, radius 5"""
    import sampler_reference as R
    from enarf_gan_amd import ops
    from test_gpu_sampler_referee import _check_topk, _mask_noise
    B, h, w, k, radius = 2, 19, 23, 37, 5
    mask, noise = _mask_noise(B, h, w, h * w + k)
    inputs = _begin(dict(mask=_d(mask), noise=_d(noise)))
    ids = ops.mask_dilate_topk(inputs["mask"], inputs["noise"], k, radius)
    # include/enarf_hip.h: "as flat pixel ids y * w + x, unordered (torch.topk(sorted=False))": the order of the k ids is
    # not specified, so the ids are compared as a sorted list (a row that was not written still shows: its ids leave the image)
    out = dict(ids=ids.sort(dim=1).values)

    def check(o):
        score, thr = R.dilate_topk(mask, noise, k, radius)
        _check_topk("topk 19x23", o["ids"], score, thr, k)
    return inputs, out, _checked(check)


# ---- enarf_bias_act, enarf_upfirdn2d
def _bias_act(shape, bias):
    """forward, the derivative form (`ref` = the forward's output, reached through a backward) and that form applied again"""
    from enarf_gan_amd.libraries.custom_stylegan2 import op
    from oracle import gan_ops_oracle as third
    from test_gpu_gan2d import BIAS_ACT_RTOL, _rel
    slope, gain = 0.2, 2 ** 0.5
    g = torch.Generator().manual_seed(sum(shape))
    x, gy, ggx = (torch.randn(shape, generator=g) for _ in range(3))
    b = torch.randn(shape[1], generator=g) if bias else None
    inputs = _begin(dict(x=x.cuda(), gy=gy.cuda(), ggx=ggx.cuda(), **({"b": b.cuda()} if bias else {})))
    xx, gyy = inputs["x"].detach().requires_grad_(True), inputs["gy"].clone().requires_grad_(True)
    y = op.fused_leaky_relu(xx, inputs.get("b"), slope, gain)
    (gx,) = torch.autograd.grad(y, xx, gyy, create_graph=True)
    (g2,) = torch.autograd.grad(gx, gyy, inputs["ggx"])

    def check(o):
        t = x.double() + (b.double().view([1, -1] + [1] * (x.dim() - 2)) if bias else 0.0)
        d = gain * torch.where(t > 0, 1.0, slope)
        assert _rel(o["y"], third.fused_leaky_relu(x.double(), b.double() if bias else None, slope, gain)) < BIAS_ACT_RTOL
        assert _rel(o["gx"], gy.double() * d) < BIAS_ACT_RTOL
        assert _rel(o["g2"], ggx.double() * d) < BIAS_ACT_RTOL
    return inputs, dict(y=y.detach(), gx=gx.detach(), g2=g2), _checked(check)


def bias_act_scalar_with_bias():
    """bias_act_kernel<1>: inner = 117 is odd"""
    return _bias_act((2, 5, 9, 13), True)


def bias_act_scalar_without_bias():
    return _bias_act((2, 5, 9, 13), False)


def bias_act_vector_with_bias():
    """bias_act_kernel<4>: inner = 108, 270 vectors (a ragged last workgroup)"""
    return _bias_act((2, 5, 9, 12), True)


def _upfirdn(planes, H, W, kh, kw, up, down, pad, absorbed=None, ppw=None):
    from enarf_gan_amd.libraries.custom_stylegan2 import op
    from oracle import gan_ops_oracle as third
    from test_gpu_gan2d import UPFIRDN_RTOL, _cus, _random_filter, _rel
    plan = op.upfirdn2d_plan(planes[0] * planes[1], H, W, kh, kw, up, down, pad, num_cus=_cus())
    if absorbed is not None:
        assert absorbed in (plan["ex"], plan["ey"]), plan
    if ppw is not None:
        assert plan["ppw"] >= ppw and planes[0] * planes[1] % plan["ppw"] != 0, plan
    k = _random_filter(kh, kw, H * W)
    x = torch.randn(*planes, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    inputs = _begin(dict(x=x.cuda(), k=k.cuda()))
    got = op.upfirdn2d(inputs["x"], inputs["k"], up=up, down=down, pad=pad)

    def check(o):
        want = third.upfirdn2d(x.double(), k.double(), up=up, down=down, pad=pad)
        assert o["out"].shape == want.shape
        assert _rel(o["out"], want) < UPFIRDN_RTOL
    return inputs, dict(out=got), _checked(check)


def upfirdn2d_absorbed_row():
    """UPFIRDN_BOUNDARY_CASES: 65 x 40, narrow-tall, a 1-row remainder absorbed by the last tile row; 6 planes"""
    return _upfirdn((2, 3), 65, 40, 4, 4, 1, 1, (1, 2), absorbed=1)


def upfirdn2d_absorbed_8_rows():
    """72 x 40: an 8-row remainder absorbed; 5 planes"""
    return _upfirdn((1, 5), 72, 40, 4, 4, 1, 1, (1, 2), absorbed=8)


def upfirdn2d_absorbed_column():
    """33 x 129, wide: 1 column and 1 row absorbed"""
    return _upfirdn((2, 3), 33, 129, 4, 4, 1, 1, (1, 2), absorbed=1)


def upfirdn2d_absorbed_8_columns():
    """40 x 136: 8 columns and 8 rows absorbed"""
    return _upfirdn((1, 5), 40, 136, 4, 4, 1, 1, (1, 2), absorbed=8)


def upfirdn2d_up_9x13():
    """the generic up-sampler, a 4 x 3 filter on 9 x 13 planes, 6 of them"""
    return _upfirdn((2, 3), 9, 13, 4, 3, 2, 1, (2, 1))


def upfirdn2d_down_9x13():
    """the generic decimator, 5 planes"""
    return _upfirdn((1, 5), 9, 13, 4, 3, 1, 2, (1, 1))


def upfirdn2d_pipeline_planes():
    """UPFIRDN_PIPELINE_CASES[0]: 2 * 4096 + 3 planes of 10 x 12, two and more planes per workgroup with a remainder"""
    return _upfirdn((2 * 4096 + 3, 1), 10, 12, 4, 4, 2, 1, (2, 1), ppw=2)


# ================================================================================================= libenarf_mesh.so
def _mesh(vol, iso, empty=False):
    import mc_reference as M
    from enarf_gan_amd.libraries.NARF.mesh_rendering import marching_cubes
    from test_gpu_mesh import _assert_vertices_within_2ulp
    inputs = _begin(dict(volume=_d(vol)))
    v, t = marching_cubes(inputs["volume"], iso)

    def check(o):
        rv, rt = M.marching_cubes(vol, iso)
        gv, gt = o["vertices"].cpu().numpy(), o["triangles"].cpu().numpy()
        assert gv.dtype == np.float32 and gt.dtype == np.int64 and gv.shape[1:] == (3,) and gt.shape[1:] == (3,)
        assert np.array_equal(gt, rt), f"triangles differ ({len(gt)} vs {len(rt)})"
        _assert_vertices_within_2ulp(gv, rv, "marching cubes")
        assert (len(rt) == 0) == empty
    return inputs, dict(vertices=v, triangles=t), _checked(check)


def mesh_noise_17x19x23():
    vol = np.random.default_rng(7).standard_normal((17, 19, 23)).astype(np.float32)
    return _mesh(vol, 0.1)


def mesh_2x2x2():
    return _mesh(np.array([1, -1, -1, 2, 0.5, -3, 4, -1], np.float32).reshape(2, 2, 2), 0.0)


def mesh_all_outside():
    """V = T = 0: enarf_mesh_count alone, nothing to emit"""
    return _mesh(-np.ones((5, 6, 7), np.float32), 0.0, empty=True)


# ================================================================================================= libenarf_raster.so
def _raster(R, empty=False):
    import raster_reference as RR
    from enarf_gan_amd.libraries.NARF.mesh_rendering import rasterize_mesh
    from test_gpu_raster import CAMERAS, _K, _check, _hand_mesh
    _, img, fx, fy, cx, cy = CAMERAS[R]
    K = _K(fx, fy, cx, cy)
    verts, tris = (np.ones((5, 3), np.float32), np.zeros((0, 3), np.int64)) if empty else _hand_mesh()
    inputs = _begin(dict(vertices=_d(verts), triangles=_d(tris), K=_d(K).reshape(1, 3, 3)))
    res = rasterize_mesh(inputs["vertices"], inputs["triangles"], inputs["K"], img, R)

    def check(o):
        got = {k: v.cpu().numpy() for k, v in o.items()}
        if empty:
            assert (got["image"] == 255).all() and (got["pix_to_face"] == -1).all() and (got["zbuf"] == -1).all()
            assert (got["bary"] == -1).all() and (got["normals"] == 0).all()
        else:
            _check(got, RR.rasterize(verts, tris, K, img, R), f"hand-placed R={R}")
    return inputs, {k: getattr(res, k) for k in res._fields}, _checked(check)


def raster_hand_mesh_64():
    return _raster(64)


def raster_hand_mesh_257():
    return _raster(257)


def raster_empty_mesh():
    return _raster(64, empty=True)


# ================================================================================================= libenarf_pose.so
def _bone_masks(outputs):
    import bone_mask_reference as R
    from enarf_gan_amd.dataset.utils_3d import bone_masks
    from test_gpu_pose import _check_bits, _poses
    B, S, t = 3, 7, 0.5                                 # 49 pixels a frame: every extent ragged
    poses, K = _poses(B, S, seed=100 + B)
    inputs = _begin(dict(poses=_d(poses), K=_d(K)))
    out = bone_masks(inputs["poses"], inputs["K"], S, t, outputs)

    def check(o):
        ref = R.batch(poses, K, S, t)
        assert set(o) == set(outputs)
        _check_bits({k: v.cpu().numpy() for k, v in o.items()}, {k: ref[k] for k in o}, slice(None), f"bone masks {outputs}")
    return inputs, dict(out), _checked(check)


def pose_bone_masks_all_outputs():
    from test_gpu_pose import ALL
    return _bone_masks(ALL)


def pose_bone_masks_mask_only():
    return _bone_masks(("mask",))


# ================================================================================================= libenarf_photo.so
def _photo_loss(with_mask):
    import photo_reference as R
    from enarf_gan_amd import ops
    from test_gpu_photo import G_COLOR, G_MASK, _loss_case, _within_ulp
    B, S, N, cc, mc = 2, 9, 63, 1.7, 0.6
    inp = _loss_case(B, S, N, seed=S + N)
    inputs = _begin({k: _d(v) for k, v in inp.items()})
    out = {}
    for loss_type in ("mse", "mae"):
        sc, sm = inputs["sparse_color"].clone().requires_grad_(), inputs["sparse_mask"].clone().requires_grad_()
        lc, lm = ops.photometric_loss(inputs["grid"], sc, sm, inputs["color"], inputs["mask"] if with_mask else None, loss_type,
                                      cc, mc)
        (G_COLOR * lc + G_MASK * lm).backward()
        out.update({f"{loss_type}.loss_color": lc.detach(), f"{loss_type}.d_sparse_color": sc.grad})
        if with_mask:
            out.update({f"{loss_type}.loss_mask": lm.detach(), f"{loss_type}.d_sparse_mask": sm.grad})
        else:
            assert sm.grad is None

    def check(o):
        for loss_type in ("mse", "mae"):
            args = (inp["grid"], inp["sparse_color"], inp["sparse_mask"], inp["color"], inp["mask"] if with_mask else None,
                    loss_type, cc, mc)
            ref = dict(zip(("loss_color", "loss_mask"), R.loss(*args)))
            ref.update(zip(("d_sparse_color", "d_sparse_mask"), R.loss_grad(*args, g_color=G_COLOR, g_mask=G_MASK)))
            for k in ("loss_color", "d_sparse_color") + (("loss_mask", "d_sparse_mask") if with_mask else ()):
                _within_ulp(o[f"{loss_type}.{k}"].cpu().numpy(), ref[k], f"photo {loss_type} {k}")
    return inputs, out, _checked(check)


def photo_loss_with_mask():
    """photo_loss_kernel, photo_loss_finish_kernel and photo_loss_bwd_kernel: B = 2, N = 63 rays on a 9 x 9 frame"""
    return _photo_loss(True)


def photo_loss_without_mask():
    return _photo_loss(False)


def _photo_metrics(masks):
    from enarf_gan_amd import ops
    from test_gpu_photo import _check_metric_values
    rng = np.random.default_rng(11)
    B, H, W = 2, 19, 23
    img = rng.uniform(-1, 1, (B, 3, H, W)).astype(np.float32)
    gen = np.clip(img + rng.normal(0, 0.2, img.shape), -1, 1).astype(np.float32)
    mask, gen_mask = (rng.uniform(0, 1, (B, H, W)).astype(np.float32) for _ in range(2))
    names = ("img", "gen") + (("mask", "gen_mask") if masks else ())
    inputs = _begin({k: _d(v) for k, v in zip(names, (img, gen, mask, gen_mask))})
    out = ops.image_metrics(inputs["img"], inputs["gen"], inputs.get("mask"), inputs.get("gen_mask"))

    def check(o):
        _check_metric_values(o["metrics"], img, gen, mask if masks else None, gen_mask if masks else None, None,
                             f"metrics masks={masks}")
    return inputs, dict(metrics=out), _checked(check)


def photo_metrics_with_masks():
    """photo_metrics_kernel + photo_metrics_finish_kernel on 19 x 23 frames, B = 2"""
    return _photo_metrics(True)


def photo_metrics_without_masks():
    return _photo_metrics(False)


# ================================================================================================= libenarf_guide.so
def _guide(ratio):
    import mask_guidance_reference as R
    from enarf_gan_amd import ops
    from test_gpu_mask_guidance import COEF, UP, _within_ulp
    rng = np.random.default_rng(2)
    mask = (np.floor(rng.uniform(0, 1, (3, 7, 7)) * 64) / 64).astype(np.float32)         # 147 values with ties
    bone = (rng.uniform(0, 1, (3, 14, 14)) > 0.9).astype(np.float32)
    inputs = _begin(dict(mask=_d(mask), bone=_d(bone)))
    m = inputs["mask"].clone().requires_grad_()
    loss, push, bone_term = ops.mask_guidance_loss(m, inputs["bone"], ratio, COEF, return_terms=True)
    (UP * loss).backward()

    def check(o):
        r_push, r_bone = R.terms(mask, bone, ratio)
        _within_ulp(o["loss"].item(), R.loss(mask, bone, ratio, COEF), "guide loss")
        _within_ulp(o["push"].item(), r_push, "guide push")
        _within_ulp(o["bone"].item(), r_bone, "guide bone")
        _within_ulp(o["d_mask"].cpu().numpy(), R.loss_grad(mask, bone, ratio, COEF, UP), "guide d fake_mask")
    return inputs, dict(loss=loss.detach(), push=push, bone=bone_term, d_mask=m.grad), _checked(check)


def guide_loss_with_push():
    """guide_hist_kernel, guide_sum_kernel, guide_finish_kernel, guide_bwd_kernel: 3 x 7 x 7 masks under 14 x 14 bone masks"""
    return _guide(0.7)


def guide_loss_without_push():
    """ratio 0: the push term and its histogram passes are left out"""
    return _guide(0.0)


# ================================================================================================= libenarf_anim.so
def _interpolate(everything):
    import anim_reference as A
    from enarf_gan_amd import ops
    from test_gpu_anim import PARENTS, _check
    keys, num, loop, _, f64, d = A.golden_case(0)
    orbit = np.linspace(0.0, 2 * np.pi, num, endpoint=False)
    f64, d = A.gap(keys, PARENTS, num, loop, orbit)
    inputs = _begin(dict(keys=_d(keys), orbit=_d(orbit)))
    if everything:
        p64, p32, bone = ops.interpolate_pose(inputs["keys"], PARENTS, num, loop, orbit=inputs["orbit"], return_f32=True,
                                              return_bone_length=True)
        out = dict(poses=p64, poses_f32=p32, bone_length=bone)
    else:
        out = dict(poses=ops.interpolate_pose(inputs["keys"], PARENTS, num, loop, orbit=inputs["orbit"]))

    def check(o):
        if everything:
            _check("poison", tuple(o[k].cpu().numpy() for k in ("poses", "poses_f32", "bone_length")), keys, PARENTS, num, loop, f64, d)
        else:
            p = o["poses"].cpu().numpy()
            assert p.shape == f64.shape and p.dtype == np.float64 and np.isfinite(p).all() and np.abs(p - f64).max() <= A.FACTOR * d
    return inputs, out, _checked(check)


def anim_interpolate_all_outputs():
    """the pose kernel on the first recorded case with an orbit, the fp32 copy and the bone lengths"""
    return _interpolate(True)


def anim_interpolate_poses_only():
    return _interpolate(False)


def _compose(masks):
    import anim_reference as A
    from enarf_gan_amd import ops
    F, S = 3, 5                                        # n = 25: a tail, and groups of four pixels that straddle two frames
    rng = np.random.default_rng(100 * F + S)
    color = rng.uniform(-1.3, 1.3, (F, 3, S * S)).astype(np.float32)
    mask = rng.uniform(-0.1, 1.1, (F, S * S)).astype(np.float32)
    mask[rng.uniform(size=mask.shape) < 0.2] = 0.0
    mask[rng.uniform(size=mask.shape) < 0.2] = 1.0
    bg = rng.uniform(-1.2, 1.2, (F, 3, S, S)).astype(np.float32)
    inputs = _begin(dict(color=_d(color).reshape(F, 3, S, S), mask=_d(mask).reshape(F, S, S), background=_d(bg)))
    res = ops.compose_frames(inputs["color"], inputs["mask"], inputs["background"], return_masks=masks)
    out = dict(frames=res[0], masks=res[1]) if masks else dict(frames=res)

    def check(o):
        want_frames, want_masks = A.compose_frames(color, mask, bg)
        assert np.array_equal(o["frames"].cpu().numpy(), want_frames)
        assert not masks or np.array_equal(o["masks"].cpu().numpy(), want_masks)
    return inputs, out, _checked(check)


def anim_compose_with_masks():
    return _compose(True)


def anim_compose_frames_only():
    return _compose(False)


# ================================================================================================= libenarf_seg.so
def _seg_labels(bits):
    import seg_reference as R
    from enarf_gan_amd import ops
    from test_gpu_seg import _check_labels, _scene
    M = 63
    sc, ds = _scene(2, "center_fixed")
    g = torch.Generator().manual_seed(M)
    centres = sc.pose_scaled[:, torch.randint(0, sc.P, (M,), generator=g), :3, 3].permute(0, 2, 1)
    pts = (centres + torch.randn(2, 3, M, generator=g) * 0.4).contiguous()
    inputs = _begin(dict(pts=pts.to(ds.dev), parts=ds.parts, tri=ds.tri, cpose=ds.cpose))
    res = ops.part_labels(inputs["pts"], inputs["parts"], inputs["cpose"], inputs["tri"], return_valid_bits=bits)
    out = dict(zip(("label", "top", "second", "valid_bits"), res))

    def check(o):
        ref = R.labels(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"])
        assert len(o) == (4 if bits else 3) and all(tuple(t.shape) == (2, M) for t in o.values())
        if bits:
            assert np.array_equal(o["valid_bits"].cpu().numpy().view(np.uint32), R.bits(ref["valid"]))
        _check_labels([o[k].cpu().numpy() for k in ("label", "top", "second")], ref, f"M={M}", cap=False)
    return inputs, out, _checked(check)


def seg_labels_with_valid_bits():
    """seg_label_kernel on 63 explicit points an image, B = 2"""
    return _seg_labels(True)


def seg_labels_without_valid_bits():
    return _seg_labels(False)


def seg_composite_nf65():
    """seg_composite_kernel: Nf = 65, 37 rays x 2 images (no multiple of the 4 rays of a workgroup), as
    test_composite_sample_counts_and_edge_rays plants them"""
    import seg_reference as R
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.rendering import semantic_palette
    from test_gpu_seg import _check_composite
    nf, B, n, P = 65, 2, 37, 24
    g = torch.Generator().manual_seed(nf)
    labels = torch.randint(-1, P, (B, n, nf), generator=g, dtype=torch.int32)
    labels[0, 3] = torch.randint(0, 3, (nf,), generator=g, dtype=torch.int32)
    labels[1, 5, ::2] = 99
    w = torch.rand(B, 1, n, nf - 1, generator=g) / nf
    w[0, 0, 7] = 0.0
    labels[1, 9] = -1
    pal = semantic_palette(P)
    inputs = _begin(dict(labels=labels.cuda(), weights=w.cuda(), palette=pal.cuda()))
    res = ops.semantic_composite(inputs["labels"], inputs["weights"], inputs["palette"])

    def check(o):
        got = (o["color"], o["part_map"], o["part_mass"])
        _check_composite(got, R.composite(labels.numpy(), w.numpy(), pal), f"Nf={nf}", cap=False)
        for b, r in ((0, 7), (1, 9)):
            assert int(got[1][b, r]) == -1 and float(got[2][b, r]) == 0 and bool((got[0][b, :, r] == 0).all())
    return inputs, dict(zip(("color", "part_map", "part_mass"), res)), _checked(check)


# ================================================================================================= libenarf_paint.so
_GEO = ("pix_to_face", "bary", "normals", "vertices", "triangles")


def _hand_fragments():
    """the 8 x 8 hand-written fragment buffer of tests/paint_cases.py cut to 7 x 7: 49 pixels, no multiple of 64"""
    import paint_cases as PC
    h = dict(PC.hand_buffer())
    for k in ("pix_to_face", "bary", "normals"):
        h[k] = np.ascontiguousarray(h[k][:7, :7])
    return h


def _paint(labels):
    import paint_reference as PR
    from enarf_gan_amd import ops
    from test_gpu_paint import _check
    h = _hand_fragments()
    mode = dict(vertex_labels=h["vertex_labels"], palette=h["palette"]) if labels else dict(vertex_colors=h["vertex_colors"])
    kw = dict(lit=True, background=(0.1, 0.2, 0.3), neutral=(0.6, 0.5, 0.4))
    inputs = _begin({k: _d(h[k]) for k in _GEO + tuple(mode)})
    res = ops.shade_fragments(*(inputs[k] for k in _GEO), **{k: inputs[k] for k in mode}, **kw)

    def check(o):
        ref = PR.shade(**{k: h[k] for k in _GEO}, **mode, **kw)
        assert ref["drawn"].sum() > 30 and (~ref["drawn"]).sum() > 5
        _check({k: v.cpu().numpy() for k, v in o.items()}, ref, f"hand buffer labels={labels}", exact_albedo=labels)
    return inputs, {k: getattr(res, k) for k in res._fields}, _checked(check)


def paint_vertex_colors():
    """paint_shade_kernel on the hand-written fragments: face ids outside [0, T), vertices outside [0, V), a NaN barycentric"""
    return _paint(False)


def paint_vertex_labels():
    return _paint(True)


# ================================================================================================= libenarf_bake.so
def bake_points_hand_mesh():
    """bake_points_kernel: the five hand triangles in an atlas of 21 x 21 texels (441, cells of 10 with a margin of one)"""
    import bake_cases as BC
    import bake_reference as BR
    from enarf_gan_amd import ops
    from test_gpu_bake import _check_points
    (v, t), A = BC.hand_mesh(5), 21
    inputs = _begin(dict(vertices=_d(v), triangles=_d(t)))
    res = ops.bake_points(inputs["vertices"], inputs["triangles"], A)

    def check(o):
        own = _check_points({k: x.cpu().numpy() for k, x in o.items()}, BR.points(v, t, A), A, "hand mesh 21")
        assert 0 < own.sum() < own.size
    return inputs, dict(points=res.points, texel_face=res.texel_face), _checked(check)


def _bake_resolve(want_float):
    import bake_cases as BC
    import bake_reference as BR
    from enarf_gan_amd import ops
    from test_gpu_bake import _check_resolved
    face, color, labels, palette = BC.resolve_inputs()                      # 5 x 13 texels
    fill, neutral = (0.2, 0.4, 0.6), (0.6, 0.5, 0.4)
    inputs = _begin(dict(face=_d(face), color=_d(color), labels=_d(labels), palette=_d(palette)))
    a = ops.bake_resolve(inputs["face"], color=inputs["color"], fill=fill, want_float=want_float)
    b = ops.bake_resolve(inputs["face"], labels=inputs["labels"], palette=inputs["palette"], fill=fill, neutral=neutral,
                         want_float=want_float)
    out = {"color.texture": a.texture, "labels.texture": b.texture}
    if want_float:
        out.update({"color.texture_f32": a.texture_f32, "labels.texture_f32": b.texture_f32})
    else:
        assert a.texture_f32 is None and b.texture_f32 is None

    def check(o):
        for what, data, kw in (("color", dict(color=color), {}), ("labels", dict(labels=labels, palette=palette), dict(neutral=neutral))):
            _check_resolved(o[what + ".texture"].cpu().numpy(), o[what + ".texture_f32"].cpu().numpy() if want_float else None,
                            BR.resolve(face, **data, fill=fill, **kw), face, what)
    return inputs, out, _checked(check)


def bake_resolve_with_float_texture():
    """bake_resolve_kernel on 5 x 13 texels, colours and labels, with the optional fp32 texture"""
    return _bake_resolve(True)


def bake_resolve_bytes_only():
    return _bake_resolve(False)


def _bake_shade(which):
    import bake_cases as BC
    import bake_reference as BR
    from enarf_gan_amd import ops
    from test_gpu_paint import _check
    h, texture = _hand_fragments(), BC.hand_textures(16)[which]
    kw = dict(lit=True, background=(0.1, 0.2, 0.3))
    inputs = _begin({**{k: _d(h[k]) for k in _GEO}, "texture": _d(texture)})
    res = ops.shade_textured(*(inputs[k] for k in _GEO), inputs["texture"], **kw)

    def check(o):
        ref = BR.shade(**{k: h[k] for k in _GEO}, texture=texture, **kw)
        _check({k: v.cpu().numpy() for k, v in o.items()}, ref, f"hand buffer, {texture.dtype} texture")
    return inputs, {k: getattr(res, k) for k in res._fields}, _checked(check)


def bake_shade_rgba8_texture():
    """bake_shade_kernel on the hand-written fragments over a 16 x 16 texture"""
    return _bake_shade(0)


def bake_shade_float_texture():
    return _bake_shade(1)


# ================================================================================================= libenarf_simp.so
def _simplify(case, placement):
    import paint_cases as PC
    import simp_cases as SC
    from enarf_gan_amd import ops
    from test_gpu_simp import _compare
    if case in SC.HAND:
        v, t, h, o = SC.mesh(case)
    else:
        (v, t), h, o = PC.sphere(), SC.sphere_cell(case), None
    inputs = _begin(dict(vertices=_d(np.array(v)), triangles=_d(np.array(t))))
    res = ops.simplify_mesh(inputs["vertices"], inputs["triangles"], h, origin=o, placement=placement)

    class _Got:
        pass

    def check(out):
        got = _Got()
        for k, x in out.items():
            setattr(got, k, x)
        _compare(got, SC.referee(case, placement), f"{case} {placement}")
    return inputs, {k: getattr(res, k) for k in res._fields}, _checked(check)


def simp_wedge_quadric():
    """simp_keys / simp_corners / simp_place on the hand mesh whose quadric placement is clamped to the cell's box"""
    return _simplify("wedge", "quadric")


def simp_sphere_mean():
    """the 33^3 sphere in cells of six voxels (94 clusters of up to 72 vertices), placed at the mean"""
    return _simplify(6, "mean")


def simp_sphere_quadric():
    return _simplify(6, "quadric")


# ================================================================================================= libenarf_geom.so
def _geom_hand(want):
    import geom_cases as GC
    import geom_reference as GR
    from enarf_gan_amd import ops
    from test_gpu_geom import FIELDS, _check
    q, m, K = GC.hand_buffer(7)                        # 49 pixels: one partial tile
    inputs = _begin(dict(disparity=_d(q[None]), mask=_d(m[None]), K=_d(K)))
    kw = dict(shade="lit", background=(0.1, 0.2, 0.3))
    res = ops.geometry_buffers(inputs["disparity"], inputs["mask"], inputs["K"], want=want, **kw)
    assert all((getattr(res, k) is None) == (k not in want) for k in FIELDS)

    def check(o):
        ref = GR.buffers(q[None], m[None], K, **kw)
        if set(want) == set(FIELDS):
            _check({k: v.cpu().numpy() for k, v in o.items()}, ref, "hand buffer 7 x 7")
        else:
            assert tuple(o) == ("flags",) and np.array_equal(o["flags"].cpu().numpy(), ref["flags"])
    return inputs, {k: getattr(res, k) for k in want}, _checked(check)


def geom_buffers_every_output():
    """geom_buffers_kernel on the hand-written 7 x 7 buffer: invalid pixels, one-sided differences at them and at the border"""
    from test_gpu_geom import FIELDS
    return _geom_hand(FIELDS)


def geom_buffers_flags_only():
    return _geom_hand(("flags",))


def geom_buffers_scenes_37x53():
    """B = 2 with a matrix per image, 37 x 53: partial tiles on both axes"""
    import geom_reference as GR
    from enarf_gan_amd import ops
    from test_gpu_geom import _batch, _check
    _, q, m, K = _batch(37, 53)
    inputs = _begin(dict(disparity=_d(q), mask=_d(m), K=_d(K)))
    res = ops.geometry_buffers(inputs["disparity"], inputs["mask"], inputs["K"])
    return (inputs, {k: getattr(res, k) for k in res._fields},
            _checked(lambda o: _check({k: v.cpu().numpy() for k, v in o.items()}, GR.buffers(q, m, K), "scenes 37 x 53")))


def _depth_error(with_mask):
    import geom_cases as GC
    import geom_reference as GR
    from enarf_gan_amd import ops
    from test_gpu_geom import _check_depth_error
    shape = (3, 37, 53)                                # 5883 pixels: three records, the last one ragged
    batches = [GC.error_batch(shape, seed) for seed in (11, 12)]
    inputs = _begin({f"{k}{i}": _d(a) for i, b in enumerate(batches) for k, a in zip(("disparity", "target", "mask"), b)})
    err = ops.DepthError()
    for i in range(2):
        err.update(inputs[f"disparity{i}"], inputs[f"target{i}"], inputs[f"mask{i}"] if with_mask else None)

    def check(o):
        ref = GR.merge([GR.depth_error(q, g, m if with_mask else None) for q, g, m in batches])
        mine = ops.DepthError()
        mine._state = o["state"]
        _check_depth_error(mine.result(), ref, shape)
    return inputs, dict(state=err.state()), _checked(check)


def geom_depth_error_with_mask():
    """geom_err_update: two updates of 3 x 37 x 53 pixels into the running state, through the record workspace"""
    return _depth_error(True)


def geom_depth_error_without_mask():
    return _depth_error(False)


# ================================================================================================= libenarf_pgrad.so, libenarf_nrm.so
_POSE_REF = []


def _pose_ref():
    """the scene of tests/test_gpu_pgrad.py and test_gpu_nrm.py, 65 of its points an image (a wave and one lane), their
    upstream gradients, the float64 referee on those points and the all-ones upstream whose g_points is the field gradient:
    once for the pgrad and nrm cases"""
    if not _POSE_REF:
        import pgrad_reference as PR
        from _helpers import Scene
        n = 65
        sc = Scene(32, 2)
        pts = PR.scene_points(sc, 1000)[:, :, :n].contiguous()
        gd, gc = PR.upstream(sc.B, 1000)
        _POSE_REF.extend([sc, pts, gd[:, :n].contiguous(), gc[:, :, :n].contiguous(), PR.Referee(sc, pts, "default"),
                          torch.ones(sc.B, n)])
    return _POSE_REF


def _pgrad(gd_given, gc_given):
    import pgrad_reference as PR
    from _helpers import DeviceScene
    from enarf_gan_amd import ops
    sc, pts, gd, gc, ref, _ = _pose_ref()
    ds = DeviceScene(sc)
    gd, gc = (gd if gd_given else None), (gc if gc_given else None)
    inputs = dict(pts=pts.to(ds.dev), parts=ds.parts, pack=ds.pack, tri=ds.tri, feat_cl=ds.feat_cl)
    if gd_given:
        inputs["gd"] = (gd * ref.keep).contiguous().to(ds.dev)
    if gc_given:
        inputs["gc"] = (gc * ref.keep[:, None]).contiguous().to(ds.dev)
    _begin(inputs)
    g_points, g_parts = ops.query_pose_bwd(inputs["pts"], ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, inputs.get("gd"),
                                           inputs.get("gc"))
    none = ops.query_pose_bwd(inputs["pts"][:, :, :0], ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack, None, None)   # N = 0

    def check(o):
        assert o["g_points"].shape == pts.shape and o["g_parts"].shape == (2, 23, 16)
        assert o["no_points.g_parts"].shape == (2, 23, 16) and not bool(o["no_points.g_parts"].any()), "N = 0: g_parts is zeros"
        PR.check({k: v.cpu() for k, v in o.items()}, ref.grads(gd, gc), "pgrad N = 65", ("g_points", "g_parts"))
        assert float(o["g_parts"][:, :, 13:].abs().max()) == 0.0
    return inputs, {"g_points": g_points, "g_parts": g_parts, "no_points.g_parts": none[1]}, _checked(check)


def pgrad_both_upstream_gradients():
    """pgrad_query: 65 points an image, B = 2, through the fp64 workspace of the per-block part gradients"""
    return _pgrad(True, True)


def pgrad_color_gradient_only():
    return _pgrad(False, True)


def nrm_field_gradient_n65():
    """nrm_gradient_kernel on the same 65 points an image: the gradient is the pose gradient's g_points for g_density = 1"""
    import pgrad_reference as PR
    from _helpers import DeviceScene, assert_close
    from enarf_gan_amd import ops
    sc, pts, _, _, ref, ones = _pose_ref()
    ds = DeviceScene(sc)
    inputs = _begin(dict(pts=pts.to(ds.dev), parts=ds.parts, pack=ds.pack, tri=ds.tri, feat_cl=ds.feat_cl))
    density, gradient = ops.field_gradient(inputs["pts"], ds.parts, ds.cpose, ds.tri, ds.feat_cl, ds.pack)

    def check(o):
        assert o["density"].shape == pts.shape[::2] and o["gradient"].shape == pts.shape
        PR.check({"g_points": o["gradient"].cpu() * ref.keep[:, None]}, ref.grads(ones, None), "field gradient N = 65", ("g_points",))
        assert float(o["gradient"].abs().max()) > 0.0
        assert_close(o["density"].cpu(), ref.f64["density"].detach(), "density vs the float64 forward")
    return inputs, dict(density=density, gradient=gradient), _checked(check)


def _ray_normals(everything):
    import nrm_reference as NR
    from enarf_gan_amd import ops
    from test_gpu_nrm import _check_ray_normals
    n, Nf = 65, 33
    c = NR.ray_case(n, Nf)
    names = ("gradient", "weights", "mask") + (("fallback", "flags", "points") if everything else ())
    inputs = _begin({k: _d(np.array(c[k])) for k in names})
    if everything:
        kw = dict(shade="lit", background=(0.1, 0.2, 0.3))
        res = ops.ray_normals(inputs["gradient"], inputs["weights"], inputs["mask"], fallback=inputs["fallback"], flags=inputs["flags"],
                              points=inputs["points"], want_magnitude=True, **kw)
    else:
        res = ops.ray_normals(inputs["gradient"], inputs["weights"], inputs["mask"], mask_threshold=0.05)
        assert res.magnitude is None and res.image is None

    def check(o):
        if everything:
            ref = NR.ray_normals(c["gradient"], c["weights"], c["mask"], c["fallback"], c["flags"], c["points"], **kw)
            _check_ray_normals(NR_result(**o), ref, n, "lit", "ray normals n = 65, Nf = 33")
        else:
            field = np.isin(c["kind"], (0, 3, 4))
            assert np.array_equal(o["flags"].cpu().numpy(), field.astype(np.uint8) * 4)
            assert not bool(o["normals"].cpu()[torch.from_numpy(~field)].any())
            ref = NR.ray_normals(c["gradient"], c["weights"], c["mask"], mask_threshold=0.05)
            _check_ray_normals(NR_result(magnitude=None, image=None, **o), ref, n, None, "bare ray normals n = 65, Nf = 33")
    from enarf_gan_amd._nrm_lib import RayNormals as NR_result
    return inputs, {k: getattr(res, k) for k in res._fields if getattr(res, k) is not None}, _checked(check)


def nrm_ray_normals_every_option():
    """nrm_ray_kernel: 65 rays of 33 samples, B = 2, with a fallback, flags, points, the lit image and the magnitude"""
    return _ray_normals(True)


def nrm_ray_normals_bare():
    return _ray_normals(False)


# ================================================================================================= libenarf_scene.so, libenarf_sgrad.so
_SCENE_SHAPE = (2, 2, 67, 2)                            # K, Nf, n, F: the smallest shape that carries the planted rays


def _scene_composite(want):
    from enarf_gan_amd import ops
    from test_gpu_scene import FIELDS, _case, _check
    (depth, density, color, valid), scale, ref = _case(*_SCENE_SHAPE)
    inputs = _begin(dict(depth=_d(np.array(depth)), density=_d(np.array(density)), color=_d(np.array(color)), valid=_d(np.array(valid))))
    res = ops.scene_composite(inputs["depth"], inputs["density"], inputs["color"], inputs["valid"], render_scale=scale, want=want)
    assert all((getattr(res, k) is None) == (k not in want) for k in FIELDS)

    def check(o):
        assert set(o) == set(want)
        _check({k: v.cpu().numpy() for k, v in o.items()}, ref, f"scene {_SCENE_SHAPE} {want}")
    return inputs, {k: getattr(res, k) for k in want}, _checked(check)


def scene_composite_every_output():
    """scene_composite_kernel: two avatars of two samples on 67 rays, two frames, with the merged samples"""
    from test_gpu_scene import FIELDS
    return _scene_composite(FIELDS)


def scene_composite_mask_only():
    return _scene_composite(("mask",))


def _scene_bwd(want):
    from enarf_gan_amd import ops
    from test_gpu_sgrad import NAMES, _case, _check
    inp, scale, up, ref = _case(*_SCENE_SHAPE)
    inputs = _begin({**{k: _d(np.array(a)) for k, a in zip(("depth", "density", "color", "valid"), inp)},
                     **{k: _d(np.array(g)) for k, g in zip(("g_color", "g_mask", "g_disparity", "g_instance_mass"), up)}})
    res = ops.scene_composite_bwd(inputs["depth"], inputs["density"], inputs["color"], inputs["valid"], scale, inputs["g_color"],
                                  inputs["g_mask"], inputs["g_disparity"], inputs["g_instance_mass"], want=want)
    assert all((getattr(res, k) is None) == (k not in want) for k in NAMES)
    return (inputs, {k: getattr(res, k) for k in want},
            _checked(lambda o: _check({k: v.cpu().numpy() for k, v in o.items()}, ref, f"sgrad {_SCENE_SHAPE}", names=want)))


def sgrad_density_and_color():
    """sgrad_composite_bwd on the same shape, all four upstream gradients"""
    return _scene_bwd(("density", "color"))


def sgrad_density_only():
    return _scene_bwd(("density",))


# ================================================================================================= libenarf_skin.so
def _skin_weights(K, bits):
    import skin_reference as SK
    from enarf_gan_amd import ops
    from test_gpu_skin import _check_weights, _scene
    V = 63
    sc, ds = _scene("center_fixed")
    g = torch.Generator().manual_seed(V)
    centres = sc.pose_scaled[0, torch.randint(0, sc.P, (V,), generator=g), :3, 3].t()
    pts = (centres + torch.randn(3, V, generator=g) * 0.4)[None].contiguous()
    inputs = _begin(dict(vertices=pts[0].t().contiguous().to(ds.dev), parts=ds.parts, tri=ds.tri, cpose=ds.cpose))
    res = ops.skin_weights(inputs["vertices"], ds.parts, ds.cpose, ds.tri, max_influences=K, coordinate_scale=1.0,
                           return_valid_bits=bits)
    out = dict(zip(("joints", "weights", "kept_mass", "valid_bits"), res))

    def check(o):
        ref = SK.weights(pts, sc.pose_scaled, sc.scale, sc.cpose, sc.raw["tri_plane"], K)
        got = [o["joints"], o["weights"], o["kept_mass"]]
        if bits:
            got.append(o["valid_bits"])
        else:                                           # the validity bits are the referee's: what is left is checked as before
            assert len(o) == 3
            import seg_reference as SR
            got.append(torch.from_numpy(SR.bits(torch.from_numpy(ref["valid"])[None])[0].view(np.int32)))
        _check_weights(got, ref, sc.P, K, f"V={V} K={K}", cap=False)
    return inputs, out, _checked(check)


def skin_weights_k4_with_valid_bits():
    """skin_weights_kernel<4> on 63 vertices"""
    return _skin_weights(4, True)


def skin_weights_k8_without_valid_bits():
    """skin_weights_kernel<8>"""
    return _skin_weights(8, False)


def _skin_pose(K):
    import skin_reference as SK
    from enarf_gan_amd import _skin_lib, ops
    from test_gpu_skin import _check_posed, _pose_case
    V, P, F = 63, 23, _skin_lib.FRAMES_PER_GROUP + 1     # a group of frames and one more
    v, joints, w, rest, tgt, cs = _pose_case(V, P, F, K, seed=1000 * V + 10 * P + F)
    inputs = _begin(dict(vertices=_d(v), joints=_d(joints), weights=_d(w), rest=_d(rest), parts=_d(tgt)))
    got = ops.skin_pose(inputs["vertices"], inputs["joints"], inputs["weights"], inputs["rest"], inputs["parts"], coordinate_scale=cs)

    def check(o):
        assert o["posed"].shape == (F, V, 3) and o["posed"].dtype == torch.float32
        _check_posed(o["posed"], SK.pose(v, joints, w, rest, tgt, cs), (P, F))
    return inputs, dict(posed=got), _checked(check)


def skin_pose_k4():
    """skin_pose_kernel<4>: 63 vertices in a group of frames and one more"""
    return _skin_pose(4)


def skin_pose_k8():
    return _skin_pose(8)


# ================================================================================================= the map
HOST_ONLY = {
    **{("enarf_abi_version" if s == "hip" else f"enarf_{s}_abi_version"): "returns a constant" for s in ALL_STEMS},
    **{("enarf_last_error" if s == "hip" else f"enarf_{s}_last_error"): "returns the last call's message" for s in ALL_STEMS},
    "enarf_version": "returns a constant",
    "enarf_device_status": "reads a word of pinned host memory",
    "enarf_triplane_sample_workspace_bytes": "host arithmetic",
    "enarf_triplane_sample_bwd_workspace_bytes": "host arithmetic",
    "enarf_mlp_pack_bytes": "returns a constant",
    "enarf_render_workspace_bytes": "host arithmetic",
    "enarf_render_bwd_rows_per_image": "host arithmetic",
    "enarf_query_bwd_rows_per_image": "host arithmetic",
    "enarf_weight_grad_workspace_bytes": "host arithmetic",
    "enarf_mask_topk_workspace_bytes": "host arithmetic",
    "enarf_upfirdn2d_out_size": "host arithmetic",
    "enarf_upfirdn2d_plan": "the launch plan, without touching a device",
    "enarf_mesh_workspace_bytes": "host arithmetic",
    "enarf_raster_workspace_bytes": "host arithmetic",
    "enarf_pgrad_workspace_bytes": "host arithmetic",
    "enarf_bake_layout": "the atlas layout of T triangles: host arithmetic into two host integers",
    "enarf_geom_err_records": "host arithmetic (the binding restates it and never calls it)",
}

# launched from inside another entry point; no Python wrapper calls them, so the recorder of the ctypes attributes cannot see
# them: the cases listed are those whose entry point makes the call
INDIRECT = {
    "enarf_near_far": "enarf_render_fwd, enarf_render_step_fwd and enarf_render_bwd call it on the workspace's near / far "
                      "slot whenever args.near_far is NULL, which is what ops.py always passes",
}

# entry points whose poisoned run faulted or hung on the device and whose cause was not found: name -> reason
NOT_RUN = {}

_MARCH_CASES = ["march_ray_nc33_nf17", "march_task_nc33_nf17", "march_ray_b2_style256", "march_task_b2_style256"]
_BWD_CASES = ["march_ray_nc33_nf17", "march_ray_b2_style256"]
_SAMPLER = ["sampler_c32_workspace", "sampler_c5_direct"]
_UPFIRDN = ["upfirdn2d_absorbed_row", "upfirdn2d_absorbed_8_rows", "upfirdn2d_absorbed_column", "upfirdn2d_absorbed_8_columns",
            "upfirdn2d_up_9x13", "upfirdn2d_down_9x13", "upfirdn2d_pipeline_planes"]
_MESH = ["mesh_noise_17x19x23", "mesh_2x2x2"]
_RASTER = ["raster_hand_mesh_64", "raster_hand_mesh_257", "raster_empty_mesh"]
_SIMP = ["simp_wedge_quadric", "simp_sphere_mean", "simp_sphere_quadric"]

POISON_CASES = {
    # ---- libenarf_hip.so
    "enarf_prepare": _MARCH_CASES + ["prepare_and_unpack", "query_fwd_placed_points", "query_fwd_lattice", "query_bwd_placed_points"],
    "enarf_mlp_unpack": ["prepare_and_unpack"],
    "enarf_triplane_pack": _MARCH_CASES + ["pack_and_unpack_add"],
    "enarf_render_fwd": _MARCH_CASES,
    "enarf_near_far": _MARCH_CASES + ["render_step_nc33_nf17"],
    "enarf_render_step_fwd": ["render_step_nc33_nf17"],
    "enarf_render_bwd": _BWD_CASES,
    "enarf_weight_grad": _BWD_CASES + ["query_bwd_placed_points"],
    "enarf_prepare_bwd": _BWD_CASES + ["query_bwd_placed_points", "prepare_bwd_b3_style256"],
    "enarf_triplane_unpack_add": _BWD_CASES + ["query_bwd_placed_points", "pack_and_unpack_add"],
    "enarf_query_fwd": ["query_fwd_placed_points", "query_fwd_lattice"],
    "enarf_query_bwd": ["query_bwd_placed_points"],
    "enarf_triplane_sample_fwd": _SAMPLER,
    "enarf_triplane_sample_bwd": _SAMPLER,
    "enarf_triplane_sample_ex_fwd": ["sampler_ex_separate", "sampler_ex_point_image"],
    "enarf_triplane_sample_ex_bwd": ["sampler_ex_separate", "sampler_ex_point_image"],
    "enarf_triplane_warp_fwd": ["warp_5x7"],
    "enarf_triplane_warp_bwd": ["warp_5x7"],
    "enarf_mask_dilate_topk": ["mask_topk_19x23"],
    "enarf_bias_act": ["bias_act_scalar_with_bias", "bias_act_scalar_without_bias", "bias_act_vector_with_bias"],
    "enarf_upfirdn2d": _UPFIRDN,
    # ---- libenarf_mesh.so, libenarf_raster.so, libenarf_pose.so, libenarf_photo.so, libenarf_guide.so
    "enarf_mesh_count": _MESH + ["mesh_all_outside"],
    "enarf_mesh_emit": _MESH,
    "enarf_raster_mesh": _RASTER,
    "enarf_pose_bone_masks": ["pose_bone_masks_all_outputs", "pose_bone_masks_mask_only"],
    "enarf_photo_loss_fwd": ["photo_loss_with_mask", "photo_loss_without_mask"],
    "enarf_photo_loss_bwd": ["photo_loss_with_mask", "photo_loss_without_mask"],
    "enarf_photo_metrics": ["photo_metrics_with_masks", "photo_metrics_without_masks"],
    "enarf_guide_loss_fwd": ["guide_loss_with_push", "guide_loss_without_push"],
    "enarf_guide_loss_bwd": ["guide_loss_with_push", "guide_loss_without_push"],
    # ---- the side libraries
    "enarf_anim_interpolate_pose": ["anim_interpolate_all_outputs", "anim_interpolate_poses_only"],
    "enarf_anim_compose_frames": ["anim_compose_with_masks", "anim_compose_frames_only"],
    "enarf_seg_labels": ["seg_labels_with_valid_bits", "seg_labels_without_valid_bits"],
    "enarf_seg_composite": ["seg_composite_nf65"],
    "enarf_paint_shade": ["paint_vertex_colors", "paint_vertex_labels"],
    "enarf_bake_points": ["bake_points_hand_mesh"],
    "enarf_bake_resolve": ["bake_resolve_with_float_texture", "bake_resolve_bytes_only"],
    "enarf_bake_shade": ["bake_shade_rgba8_texture", "bake_shade_float_texture"],
    "enarf_simp_keys": _SIMP,
    "enarf_simp_corners": _SIMP,
    "enarf_simp_place": _SIMP,
    "enarf_geom_buffers": ["geom_buffers_every_output", "geom_buffers_flags_only", "geom_buffers_scenes_37x53"],
    "enarf_geom_err_update": ["geom_depth_error_with_mask", "geom_depth_error_without_mask"],
    "enarf_pgrad_query": ["pgrad_both_upstream_gradients", "pgrad_color_gradient_only"],
    "enarf_nrm_field_gradient": ["nrm_field_gradient_n65"],
    "enarf_nrm_ray_normals": ["nrm_ray_normals_every_option", "nrm_ray_normals_bare"],
    "enarf_scene_composite": ["scene_composite_every_output", "scene_composite_mask_only"],
    "enarf_sgrad_composite_bwd": ["sgrad_density_and_color", "sgrad_density_only"],
    "enarf_skin_weights": ["skin_weights_k4_with_valid_bits", "skin_weights_k8_without_valid_bits"],
    "enarf_skin_pose": ["skin_pose_k4", "skin_pose_k8"],
}

CASE_NAMES = sorted({c for cases in POISON_CASES.values() for c in cases})
