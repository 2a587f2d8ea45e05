"""GPU tests of the DSO supervision (libenarf_photo.so): the photometric loss and its gradients, the image metrics,
bit-reproducibility, and the train / validation loop pieces of models/dso.py. The referee is the float64 restatement
of tests/photo_reference.py, never a kernel.

Bounds. A loss, an MSE or a gradient element is one fp64 expression over <= 2^20 terms (relative error <= 2^20 * 2^-53 =
2^-33, as the referee's) rounded to fp32 once: it lies within one fp32 ulp of the referee, |out - ref| <= 2^-23 |ref|
(ULP below). PSNR adds 10 / ln 10 times the MSE's 2^-33: the same bound. SSIM is an fp64 mean of values in [-1, 1]
(cancellation in vx = uxx - ux^2 costs <= 49 * 2^-53 against C2 = 9e-4) rounded to fp32, so its deviation is the
rounding of a value below 1, <= 2^-25 = 3.0e-8; SSIM_TOL is four times that, far below the 1e-5 the figure is
reported to. Measured on the MI355X over the cases below: largest SSIM deviation 2.5e-8, largest relative deviation of
any other figure 2^-24 = 6.0e-8 (profiles/r08_photo.log).
"""
import types

import numpy as np
import pytest
import torch

import photo_reference as R
from _helpers import Scene
from test_host_cpu import Cfg, _nerf_cfg
from test_photo_cpu import golden, golden_cases

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SSIM_TOL = 4 * 2.0 ** -25
G_COLOR, G_MASK = 0.75, 1.25          # upstream gradients (exact in fp32)


def _dev(a):
    return None if a is None else torch.as_tensor(a).cuda()


def _within_ulp(out, ref, what):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    err = np.abs(out - ref)
    tol = ULP * np.abs(ref) + 1e-44                                # + the smallest fp32 subnormal
    worst = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max relative deviation {worst:.3e} (bound {ULP:.3e})")
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} values beyond one fp32 ulp, worst {worst:.3e}"


def _loss_case(B, S, N, seed):
    """random frame, mask, ray ids (with duplicates) and rendered values that stay clear of the MAE threshold (built
    0.001 away from it; rounding the rendered value to fp32 moves that by less than 1e-7)"""
    rng = np.random.default_rng(seed)
    color = rng.uniform(-1, 1, (B, 3, S, S)).astype(np.float32)
    mask = (rng.uniform(0, 1, (B, S, S)) > 0.5).astype(np.float32)
    grid = rng.integers(0, S * S, (B, N)).astype(np.int64)
    grid[:, 1] = grid[:, 0]
    target, _ = R.gather(color, None, grid)
    delta = rng.uniform(-0.5, 0.5, (B, 3, N))
    small = rng.uniform(0, 1, delta.shape) < 0.3
    delta = np.where(small, rng.uniform(-0.009, 0.009, delta.shape), np.sign(delta) * (np.abs(delta) + 0.011))
    sparse_color = (target + delta).astype(np.float32)
    sparse_mask = rng.uniform(0, 1, (B, N)).astype(np.float32)
    assert R.mae_tie_margin(grid, sparse_color, color) > 0.999e-3
    assert grid.min() >= 0 and grid.max() < S * S
    return dict(color=color, mask=mask, grid=grid, sparse_color=sparse_color, sparse_mask=sparse_mask)


def _run_loss(inp, loss_type, with_mask, cc, mc, via_class=False):
    from enarf_gan_amd import ops
    from enarf_gan_amd.libraries.NeRF.loss import PhotometricLoss
    sc = _dev(inp["sparse_color"]).requires_grad_()
    sm = _dev(inp["sparse_mask"]).requires_grad_()
    mask = _dev(inp["mask"]) if with_mask else None
    if via_class:
        cfg = types.SimpleNamespace(nerf_loss_type=loss_type, color_coef=cc, mask_coef=mc)
        lc, lm = PhotometricLoss(cfg)(_dev(inp["grid"]), sc, sm, _dev(inp["color"]), mask)
    else:
        lc, lm = ops.photometric_loss(_dev(inp["grid"]), sc, sm, _dev(inp["color"]), mask, loss_type, cc, mc, check_ids=True)
    assert lc.dtype == torch.float32 and lc.dim() == 0
    if not with_mask:
        assert isinstance(lm, int) and lm == 0
    (G_COLOR * lc + G_MASK * lm).backward()
    return lc, lm, sc.grad, sm.grad


def _check_loss(inp, loss_type, with_mask, cc, mc, what, via_class=False):
    lc, lm, dc, dm = _run_loss(inp, loss_type, with_mask, cc, mc, via_class)
    mask = inp["mask"] if with_mask else None
    args = (inp["grid"], inp["sparse_color"], inp["sparse_mask"], inp["color"], mask, loss_type, cc, mc)
    rc, rm = R.loss(*args)
    rdc, rdm = R.loss_grad(*args, g_color=G_COLOR, g_mask=G_MASK)
    _within_ulp(lc.item(), rc, f"{what} loss_color")
    _within_ulp(dc.cpu().numpy(), rdc, f"{what} d sparse_color")
    if with_mask:
        _within_ulp(lm.item(), rm, f"{what} loss_mask")
        _within_ulp(dm.cpu().numpy(), rdm, f"{what} d sparse_mask")
    else:
        assert dm is None
    return lc, lm, dc, dm


@pytest.mark.parametrize("S,N", [(128, 4096), (512, 1000)])
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("loss_type", ["mse", "mae"])
def test_loss_matches_restatement(loss_type, with_mask, S, N):
    """photo_loss_kernel + photo_loss_finish_kernel and photo_loss_bwd_kernel, B = 6, at the DSO default ray batch on a
    128^2 frame and at N = 1000 on a 512^2 frame."""
    inp = _loss_case(6, S, N, seed=S + N)
    _check_loss(inp, loss_type, with_mask, 1.7, 0.6, f"{loss_type} mask={with_mask} {S}^2 x {N}")
    if S == 128:                                       # the mirror class, and already gathered targets (grid = None)
        _check_loss(inp, loss_type, with_mask, 1.0, 1.0, "PhotometricLoss", via_class=True)
        from enarf_gan_amd.libraries.NeRF.loss import PhotometricLoss
        cfg = types.SimpleNamespace(nerf_loss_type=loss_type, color_coef=1.7, mask_coef=0.6)
        t_color, t_mask = R.gather(inp["color"], inp["mask"] if with_mask else None, inp["grid"])
        lc, lm = PhotometricLoss(cfg).img_mask_loss(_dev(t_color.astype(np.float32)), _dev(inp["sparse_color"]),
                                                    None if t_mask is None else _dev(t_mask.astype(np.float32)),
                                                    _dev(inp["sparse_mask"]))
        rc, rm = R.loss(inp["grid"], inp["sparse_color"], inp["sparse_mask"], inp["color"],
                        inp["mask"] if with_mask else None, loss_type, 1.7, 0.6)
        _within_ulp(lc.item(), rc, "img_mask_loss colour")
        _within_ulp(float(lm), rm, "img_mask_loss mask")


def test_loss_matches_reference_fixture():
    """the recorded float64 losses and autograd gradients of the reference's PhotometricLoss (B = 1 and 3, N = 200 and
    333, duplicated ids): the loss kernels and the backward kernel to one fp32 ulp"""
    g = golden()
    cc, mc = float(g["color_coef"]), float(g["mask_coef"])
    assert (float(g["g_color"]), float(g["g_mask"])) == (G_COLOR, G_MASK)
    for key, inp, loss_type, with_mask in golden_cases(g):
        lc, lm, dc, dm = _run_loss(inp, loss_type, with_mask, cc, mc)
        _within_ulp(lc.item(), float(g[key + "_loss_color"]), f"{key} loss_color")
        _within_ulp(float(lm), float(g[key + "_loss_mask"]), f"{key} loss_mask")
        _within_ulp(dc.cpu().numpy(), g[key + "_d_sparse_color"], f"{key} d sparse_color")
        if with_mask:
            _within_ulp(dm.cpu().numpy(), g[key + "_d_sparse_mask"], f"{key} d sparse_mask")
        else:
            assert dm is None


def test_loss_with_one_unused_output_and_many_rays():
    """a backward that reaches only one of the two losses (the other upstream gradient is absent), and more rays than
    ENARF_PHOTO_LOSS_MAX_BLOCKS * 256 (the grid-stride loop of photo_loss_kernel)"""
    from enarf_gan_amd import ops
    inp = _loss_case(2, 64, 1024 * 256 // 2 + 77, seed=9)
    args = (inp["grid"], inp["sparse_color"], inp["sparse_mask"], inp["color"], inp["mask"], "mse", 1.0, 1.0)
    sc, sm = _dev(inp["sparse_color"]).requires_grad_(), _dev(inp["sparse_mask"]).requires_grad_()
    lc, lm = ops.photometric_loss(_dev(inp["grid"]), sc, sm, _dev(inp["color"]), _dev(inp["mask"]), "mse")
    rc, rm = R.loss(*args)
    _within_ulp(lc.item(), rc, "many rays loss_color")
    _within_ulp(lm.item(), rm, "many rays loss_mask")
    lm.backward()
    rdc, rdm = R.loss_grad(*args, g_color=0.0, g_mask=1.0)
    assert not sc.grad.any()
    _within_ulp(sm.grad.cpu().numpy(), rdm, "mask-only backward")


# ------------------------------------------------------------------------------------------------- metrics
def _rendered_frame(S=64):
    sc = Scene(S, 1, "center_fixed", 20)
    gen = _dso_generator(sc, S)
    s = sc.raw
    with torch.no_grad():
        color, mask, _ = gen.render_entire_img(s["pose_to_camera"].cuda(), s["inv_intrinsics"].cuda(), torch.tensor([0.37]).cuda(),
                                               s["bone_length"].cuda(), None, S)
    return (color + -1.0 * (1 - mask))[None].contiguous(), mask[None].contiguous()


def _blob_images(B, H, W, rng):
    """background at exactly -1 with a textured ellipse: large constant regions, where vx = uxx - ux^2 cancels"""
    yy, xx = np.mgrid[:H, :W]
    img = np.full((B, 3, H, W), -1.0, np.float32)
    gen = img.copy()
    mask = np.zeros((B, H, W), np.float32)
    for b in range(B):
        inside = ((yy - H * (0.4 + 0.05 * b)) / (H * 0.3)) ** 2 + ((xx - W * 0.5) / (W * 0.2)) ** 2 < 1
        tex = rng.uniform(-0.8, 0.9, (3, H, W)).astype(np.float32)
        img[b][:, inside] = tex[:, inside]
        gen[b][:, inside] = (tex + rng.normal(0, 0.05, tex.shape).astype(np.float32))[:, inside]
        mask[b] = inside
    return img, np.clip(gen, -1, 1), mask, np.clip(mask * 0.9 + 0.02, 0, 1).astype(np.float32)


def _check_metrics(img, gen, mask, gen_mask, bbox, what):
    from enarf_gan_amd import ops
    return _check_metric_values(ops.image_metrics(_dev(img), _dev(gen), _dev(mask), _dev(gen_mask), bbox=bbox), img, gen, mask,
                                gen_mask, bbox, what)


def _check_metric_values(out, img, gen, mask, gen_mask, bbox, what):
    """the (B, 4) result of image_metrics on these host arrays against the referee"""
    assert out.shape == (len(img), 4) and out.dtype == torch.float32
    out = out.cpu().numpy().astype(np.float64)
    boxes = [None] * len(img) if bbox is None else ([bbox] * len(img) if not hasattr(bbox[0], "__len__") else bbox)
    worst = 0.0
    for b, box in enumerate(boxes):
        ref = R.image_metrics(img[b], gen[b], None if mask is None else mask[b], None if gen_mask is None else gen_mask[b], box)
        dev = abs(out[b, 0] - ref[0])
        worst = max(worst, dev)
        assert dev <= SSIM_TOL, f"{what} image {b}: SSIM {out[b, 0]!r} vs {ref[0]!r}"
        _within_ulp(out[b, 1], ref[1], f"{what} image {b} mse_color")
        if np.isinf(ref[2]):
            assert out[b, 2] == ref[2]
        else:
            _within_ulp(out[b, 2], ref[2], f"{what} image {b} psnr")
        if mask is None:
            assert np.isnan(out[b, 3])
        else:
            _within_ulp(out[b, 3], ref[3], f"{what} image {b} mse_mask")
    print(f"{what}: largest SSIM deviation {worst:.3e} (tolerance {SSIM_TOL:.3e})")
    return worst


def test_metrics_match_restatement():
    """photo_metrics_kernel + photo_metrics_finish_kernel on whole frames: random images (128^2 and 512^2, the latter
    more tiles than the finishing workgroup has threads), a rendered frame against a perturbed copy and against itself,
    and frames that are mostly the constant background -1."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for B, S in ((5, 128), (1, 512)):
        img = rng.uniform(-1, 1, (B, 3, S, S)).astype(np.float32)
        gen = np.clip(img + rng.normal(0, 0.2, img.shape), -1, 1).astype(np.float32)
        mask = rng.uniform(0, 1, (B, S, S)).astype(np.float32)
        gen_mask = rng.uniform(0, 1, (B, S, S)).astype(np.float32)
        worst = max(worst, _check_metrics(img, gen, mask, gen_mask, None, f"random {B} x {S}^2"))
        worst = max(worst, _check_metrics(img, gen, None, None, None, f"random {B} x {S}^2, no masks"))
    frame, fmask = _rendered_frame()
    frame, fmask = frame.cpu().numpy(), fmask.cpu().numpy()
    assert fmask.max() > 0.2
    noisy = np.clip(frame + rng.normal(0, 0.03, frame.shape), -1, 1).astype(np.float32)
    worst = max(worst, _check_metrics(frame, noisy, fmask, (fmask * 0.9).astype(np.float32), None, "rendered vs perturbed"))
    from enarf_gan_amd import ops
    same = ops.image_metrics(_dev(frame), _dev(frame)).cpu().numpy()[0]
    assert same[0] == 1.0 and same[1] == 0.0 and np.isposinf(same[2])
    img, gen, mask, gen_mask = _blob_images(3, 128, 96, rng)
    worst = max(worst, _check_metrics(img, gen, mask, gen_mask, None, "constant background"))
    worst = max(worst, _check_metrics(np.full((1, 3, 40, 40), -1, np.float32), np.full((1, 3, 40, 40), 0.25, np.float32),
                                      None, None, None, "two constant images"))
    print(f"largest SSIM deviation over the whole-frame cases {worst:.3e}")


def test_metrics_rectangles():
    """rectangles read in place: odd sizes down to 7 x 7, at every border of the frame, one per image for B = 5 and
    B = 1, and a `gen` that is already cropped to the rectangle"""
    rng = np.random.default_rng(13)
    H, W = 100, 83
    img, gen, mask, gen_mask = _blob_images(5, H, W, rng)
    img[3:] = rng.uniform(-1, 1, img[3:].shape).astype(np.float32)
    boxes = [(0, 0, 7, 7), (W - 7, H - 9, W, H), (10, 0, 41, 23), (0, 31, W, 64), (76, 5, 83, 100)]
    worst = _check_metrics(img, gen, mask, gen_mask, boxes, "B = 5, one rectangle per image")
    for box in boxes + [(17, 29, 50, 46), (0, 0, W, H)]:
        worst = max(worst, _check_metrics(img[:1], gen[:1], mask[:1], gen_mask[:1], box, f"B = 1 {box}"))
    worst = max(worst, _check_metrics(img, gen, None, None, (5, 6, 38, 51), "one rectangle for all"))
    x0, y0, x1, y1 = 9, 14, 62, 77
    worst = max(worst, _check_metrics(img[:2], np.ascontiguousarray(gen[:2, :, y0:y1, x0:x1]), mask[:2],
                                      np.ascontiguousarray(gen_mask[:2, y0:y1, x0:x1]), (x0, y0, x1, y1), "gen already cropped"))
    print(f"largest SSIM deviation over the rectangle cases {worst:.3e}")


def test_reference_signatures_of_ssim_and_psnr():
    from enarf_gan_amd.libraries import metrics as M
    rng = np.random.default_rng(17)
    img = rng.uniform(-1, 1, (2, 3, 48, 40)).astype(np.float32)
    gen = np.clip(img + rng.normal(0, 0.1, img.shape), -1, 1).astype(np.float32)
    s = M.ssim(_dev(img), _dev(gen))
    assert isinstance(s, float) and abs(s - R.ssim(img[0], gen[0])) <= SSIM_TOL          # image 0 only, as the reference
    p = M.psnr(_dev(img), _dev(gen))
    mse = np.mean((img.astype(np.float64) - gen) ** 2)
    assert isinstance(p, float) and abs(p - (20 * np.log10(2) - 10 * np.log10(mse))) <= 10 / np.log(10) * 2 * ULP
    assert M.image_metrics is not None


def test_two_runs_give_identical_bits():
    from enarf_gan_amd import ops
    inp = _loss_case(6, 128, 4096, seed=21)
    for loss_type in ("mse", "mae"):
        a, b = (_run_loss(inp, loss_type, True, 1.7, 0.6) for _ in range(2))
        for x, y in zip(a, b):
            assert torch.equal(x, y), loss_type
    rng = np.random.default_rng(23)
    img, gen, mask, gen_mask = (_dev(t) for t in _blob_images(3, 200, 160, rng))
    runs = [ops.image_metrics(img, gen, mask, gen_mask, bbox=(3, 5, 150, 190)) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------- loop pieces
def _dso_generator(sc, size, Nc=48, Nf=32, ray_batchsize=512):
    from enarf_gan_amd.models.generator import DSONARFGenerator
    gen = DSONARFGenerator(Cfg(use_triplane=True, ray_batchsize=ray_batchsize, nerf_params=_nerf_cfg(Nc=Nc, Nf=Nf)), size, 24,
                           sc.raw["parents"], 23)
    gen.register_canonical_pose(sc.raw["canonical_pose"])
    gen.nerf.load_state_dict({f"mlp.{k}": v for k, v in sc.raw["mlp"].items()}, strict=False)
    with torch.no_grad():
        gen.nerf.tri_plane.copy_(sc.raw["tri_plane"][:1])
    return gen.cuda().eval()


def _dso_batch(sc, gen, S, frame_time=0.37):
    """one training frame: the generator's own render, brightened inside its mask, as the target"""
    s = sc.raw
    ft = torch.tensor([frame_time]).cuda()
    with torch.no_grad():
        color, mask, _ = gen.render_entire_img(s["pose_to_camera"].cuda(), s["inv_intrinsics"].cuda(), ft, s["bone_length"].cuda(), None, S)
    fg = (mask > 0.05).float()
    img = ((color * 0.5 + 0.3) * fg + -1.0 * (1 - fg))[None].clamp(-1, 1).contiguous()
    return {"img": img, "mask": fg[None].contiguous(), "pose_3d": s["pose_to_camera"].cuda(), "frame_time": ft,
            "bone_length": s["bone_length"].cuda(), "camera_rotation": None, "intrinsics": s["intrinsics"].cuda()}


def _torch_loss(grid, sparse_color, sparse_mask, color, mask, cc, mc):
    """the plain-torch restatement a user would write (mse)"""
    B, _, S, _ = color.shape
    t = torch.gather(color.reshape(B, 3, S * S), 2, grid[:, None].repeat(1, 3, 1))
    tm = torch.gather(mask.reshape(B, S * S), 1, grid)
    return (t - sparse_color).square().mean() * cc, (tm - sparse_mask).square().mean() * mc


def test_train_step_matches_torch_restatement_and_learns():
    """train_step on a small DSONARFGenerator with a replayed ray and sample draw: its losses equal the plain-torch restatement on
    the same rays (fp32 torch sums of 3 * 512 terms: 16 * 2^-24 relative covers the pairwise sum and the three
    roundings per term), the parameter gradients agree to the renderer backward's bound (1e-3 of each gradient
    tensor's largest magnitude: float atomics, tests/test_gpu_backward.py), and five Adam steps on the fixed frame
    and rays lower the loss."""
    from enarf_gan_amd.libraries.NeRF.loss import PhotometricLoss
    from enarf_gan_amd.libraries.NeRF.ray_sampler import mask_based_sampler
    from enarf_gan_amd.models import dso
    S = 64
    sc = Scene(S, 1, "center_fixed", 20)
    gen = _dso_generator(sc, S)
    batch = _dso_batch(sc, gen, S)
    noise = torch.rand(1, S * S, generator=torch.Generator().manual_seed(5)).cuda()
    ray_idx, pixels = mask_based_sampler(batch["mask"], 512, noise=noise)
    assert ray_idx.shape == (1, 512) and int(ray_idx.min()) >= 0 and int(ray_idx.max()) < S * S
    # one draw, replayed in its order: the sampler returns its rays unordered, and the renderer's sample draw follows
    # the ray's position in the batch
    gen.ray_sampler = lambda mask, k: (ray_idx, pixels)
    cfg = types.SimpleNamespace(nerf_loss_type="mse", color_coef=1.0, mask_coef=0.5)
    loss_func = PhotometricLoss(cfg)
    params = [p for p in gen.parameters() if p.requires_grad]
    frozen = torch.optim.SGD(params, lr=0.0)
    torch.manual_seed(3)                               # the renderer seeds its in-kernel sample draw from torch's generator
    lc, lm = dso.train_step(gen, loss_func, batch, frozen, bg_color=-1.0)
    assert gen.training and lc.is_cuda and not lc.requires_grad and lc.dim() == 0
    ours = [None if p.grad is None else p.grad.clone() for p in params]
    # the restatement, on the same rays
    frozen.zero_grad()
    torch.manual_seed(3)
    color, alpha, grid = gen(batch["pose_3d"], None, batch["mask"], batch["frame_time"], batch["bone_length"],
                             torch.inverse(batch["intrinsics"]), background=-1.0)
    tc, tm = _torch_loss(grid, color, alpha, batch["img"], batch["mask"], 1.0, 0.5)
    (tc + tm).backward()
    print(f"train_step loss {lc.item():.8e} / {lm.item():.8e}, torch {tc.item():.8e} / {tm.item():.8e}")
    assert lc.item() > 1e-4 and lm.item() > 1e-6
    assert abs(lc.item() - tc.item()) <= 16 * 2.0 ** -24 * tc.item()
    assert abs(lm.item() - tm.item()) <= 16 * 2.0 ** -24 * tm.item()
    n = 0
    for p, g in zip(params, ours):
        assert (g is None) == (p.grad is None)
        if g is None or not p.grad.any():
            continue
        scale = float(p.grad.abs().max())
        assert float((g - p.grad).abs().max()) <= 1e-3 * scale
        n += 1
    assert n >= 4
    # learning
    adam = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.99))
    first = sum(float(v) for v in (lc, lm))
    for _ in range(5):
        torch.manual_seed(3)
        lc, lm = dso.train_step(gen, loss_func, batch, adam, bg_color=-1.0)
    last = float(lc) + float(lm)
    print(f"loss before {first:.6e}, after five Adam steps {last:.6e}")
    assert last < first


def test_validate_equals_per_image_metric_calls():
    """validate (one synchronisation, results kept on the device) against per-image ssim / psnr calls on the same
    renders; psnr() works from the fp32 MSE and validate from the fp32 PSNR, each within one ulp of the exact value."""
    from enarf_gan_amd.libraries import metrics as M
    from enarf_gan_amd.models import dso
    S = 64
    sc = Scene(S, 1, "center_fixed", 20)
    gen = _dso_generator(sc, S)
    batches = [_dso_batch(sc, gen, S, ft) for ft in (0.1, 0.5, 0.9)]
    for crop in (False, True):
        torch.manual_seed(4)                           # the same sample draws in validate and in the loop below
        got = dso.validate(gen, batches, S, -1.0, crop=crop)
        assert sorted(got) == ["color", "color_PSNR", "color_SSIM", "mask"] and not gen.training
        ssim, psnr, mse, mmse = [], [], [], []
        torch.manual_seed(4)
        for b in batches:
            box = dso._mask_bbox(b["mask"][0]) if crop else None
            with torch.no_grad():
                c, m, _ = gen.render_entire_img(b["pose_3d"], torch.inverse(b["intrinsics"]), b["frame_time"], b["bone_length"],
                                                None, S, bbox=box)
            c = (c + -1.0 * (1 - m))[None]
            img, mask = b["img"], b["mask"]
            if crop:
                x0, y0, x1, y1 = box
                assert x1 - x0 >= 7 and y1 - y0 >= 7
                img, mask = img[:, :, y0:y1, x0:x1].contiguous(), mask[:, y0:y1, x0:x1].contiguous()
            ssim.append(M.ssim(img, c))
            psnr.append(M.psnr(img, c))
            mse.append(float((img.double() - c.double()).square().mean()))
            mmse.append(float((mask.double() - m[None].double()).square().mean()))
        assert abs(got["color_SSIM"] - np.mean(ssim)) <= 2.0 ** -24
        assert abs(got["color_PSNR"] - np.mean(psnr)) <= 2 * ULP * abs(np.mean(psnr))
        assert abs(got["color"] - np.mean(mse)) <= ULP * np.mean(mse)
        assert abs(got["mask"] - np.mean(mmse)) <= ULP * np.mean(mmse)
    assert dso.validate(gen, batches, S, -1.0, num_data=1, metric=("PSNR",)).keys() == {"color", "mask", "color_PSNR"}
