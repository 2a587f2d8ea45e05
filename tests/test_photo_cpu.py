"""CPU checks of the DSO supervision (libenarf_photo.so, include/enarf_photo.h): the float64 restatement
(tests/photo_reference.py) against the reference's recorded losses and gradients and against the properties that pin its
SSIM, the library's ABI and kernel inventory, and the argument checks that need no device."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import libraries as L
import photo_reference as R

ROOT, TESTS = L.ROOT, L.TESTS
SRC = os.path.join(ROOT, "enarf-gan_amd", "csrc", "enarf_photo.hip")
HEADER = L.header("photo")

def golden():
    return np.load(os.path.join(TESTS, "golden", "photometric.npz"))


def golden_cases(g):
    """(key, inputs dict, loss_type, with_mask) of every recorded case"""
    for tag in ("b1", "b3"):
        inp = {k: g[f"{tag}_{k}"] for k in ("color", "mask", "grid", "sparse_color", "sparse_mask")}
        for loss_type in ("mse", "mae"):
            for with_mask in (True, False):
                yield f"{tag}_{loss_type}_{'mask' if with_mask else 'nomask'}", inp, loss_type, with_mask


# ------------------------------------------------------------------------------------------------- the restatement
def test_restatement_reproduces_reference_fixture():
    g = golden()
    cc, mc, gc, gm = float(g["color_coef"]), float(g["mask_coef"]), float(g["g_color"]), float(g["g_mask"])
    n = 0
    for key, inp, loss_type, with_mask in golden_cases(g):
        mask = inp["mask"] if with_mask else None
        args = (inp["grid"], inp["sparse_color"], inp["sparse_mask"], inp["color"], mask, loss_type, cc, mc)
        lc, lm = R.loss(*args)
        # float64 round-off: sums of <= 3 * 3 * 333 terms, evaluated in another order than torch's
        assert abs(lc - float(g[key + "_loss_color"])) <= 1e-14 * abs(lc), key
        assert abs(lm - float(g[key + "_loss_mask"])) <= 1e-14 * abs(lm), key
        assert (lm == 0) == (not with_mask)
        dc, dm = R.loss_grad(*args, g_color=gc, g_mask=gm)
        ref = g[key + "_d_sparse_color"]
        assert np.abs(dc - ref).max() <= 1e-14 * np.abs(ref).max(), key
        if with_mask:
            ref = g[key + "_d_sparse_mask"]
            assert np.abs(dm - ref).max() <= 1e-14 * np.abs(ref).max(), key
        else:
            assert dm is None and key + "_d_sparse_mask" not in g.files
        n += 1
    assert n == 8
    # what the fixture was asked to cover
    for tag, B in (("b1", 1), ("b3", 3)):
        grid = g[f"{tag}_grid"]
        assert grid.shape[0] == B and grid.shape[1] % 64 != 0
        assert all(len(np.unique(row)) < len(row) for row in grid)                     # duplicated ids
        assert R.mae_tie_margin(grid, g[f"{tag}_sparse_color"], g[f"{tag}_color"]) > 1e-3
        d = np.abs(R.gather(g[f"{tag}_color"], None, grid)[0] - g[f"{tag}_sparse_color"])
        assert (d < 0.01).any() and (d > 0.01).any()                                   # both sides of the truncation


def test_restatement_loss_rejects_other_types():
    z = np.zeros((1, 3, 4))
    with pytest.raises(ValueError):
        R.loss(np.zeros((1, 4), np.int64), z, np.zeros((1, 4)), np.zeros((1, 3, 2, 2)), None, "huber", 1, 1)


def test_window_means_match_scipy_and_direct_sums():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 1, (3, 23, 31))
    direct = R.window_means_direct(a)
    assert np.abs(R.window_means(a) - direct).max() < 1e-13
    for mode in ("reflect", "constant", "nearest", "mirror", "wrap"):                 # the interior ignores the border mode
        f = np.stack([ndi.uniform_filter(a[c], size=7, mode=mode) for c in range(3)])
        assert np.abs(f[:, 3:-3, 3:-3] - direct).max() < 1e-14, mode


def test_ssim_properties_pin_the_restatement():
    """scikit-image is not a dependency, so SSIM is pinned by properties instead of recorded values."""
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-1, 1, (3, 20, 27)), rng.uniform(-1, 1, (3, 20, 27))
    assert R.ssim(a, a) == 1.0
    assert R.ssim(a, b) == R.ssim(b, a)
    assert -1.0 < R.ssim(a, b) < 0.2                                                  # independent noise
    for va, vb in ((-1.0, -1.0), (-1.0, 1.0), (0.3, -0.45), (0.0, 0.5)):
        got = R.ssim(np.full((3, 9, 12), va), np.full((3, 9, 12), vb))
        assert abs(got - R.ssim_constant(va, vb)) < 1e-12, (va, vb)
    # both ways of forming the window means give the same maps
    x, y = a * 0.5 + 0.5, b * 0.5 + 0.5
    assert np.abs(R.ssim_map(x, y, R.window_means) - R.ssim_map(x, y)).max() < 1e-10
    # a 7 x 7 image has one window: the plain sample statistics
    p, q = x[0, :7, :7], y[0, :7, :7]
    vx, vy, vxy = p.var(ddof=1), q.var(ddof=1), np.cov(p.ravel(), q.ravel())[0, 1]
    want = (2 * p.mean() * q.mean() + 1e-4) * (2 * vxy + 9e-4) / ((p.mean() ** 2 + q.mean() ** 2 + 1e-4) * (vx + vy + 9e-4))
    assert abs(R.ssim_map(p, q)[0, 0] - want) < 1e-13
    with pytest.raises(ValueError):
        R.ssim(a[:, :6], b[:, :6])
    m = R.image_metrics(a, b, bbox=(2, 1, 21, 19))
    assert m[0] == R.ssim(a[:, 1:19, 2:21], b[:, 1:19, 2:21]) and np.isnan(m[3])
    assert abs(m[2] - (20 * np.log10(2) - 10 * np.log10(m[1]))) < 1e-12


# ------------------------------------------------------------------------------------------------- the library
def test_header_symbols_exported_and_bound():
    """what is specific to this library; tests/test_libraries_cpu.py holds the checks every library gets"""
    from enarf_gan_amd import _photo_lib
    assert L.declared("photo") == ["enarf_photo_abi_version", "enarf_photo_last_error", "enarf_photo_loss_bwd",
                                   "enarf_photo_loss_fwd", "enarf_photo_metrics"]
    assert _photo_lib.ABI_VERSION == 1
    header = open(HEADER).read()
    assert "#define ENARF_PHOTO_LOSS_MAX_BLOCKS 1024" in header and _photo_lib.LOSS_PARTIALS == 2048
    assert f"#define ENARF_PHOTO_TILE     {_photo_lib.TILE}" in header
    assert f"#define ENARF_PHOTO_WINDOW   {_photo_lib.WINDOW}" in header
    assert f"#define ENARF_PHOTO_MAE_THRESHOLD {_photo_lib.MAE_THRESHOLD}" in header and R.MAE_THRESHOLD == 0.01
    assert _photo_lib.metric_partials(17, 512) == 3 * 2 * 32


def test_sources_read_no_environment_and_hold_no_assembly():
    for path in (SRC, HEADER):
        src = open(path).read()
        assert "getenv" not in src and "asm" not in src and "atomic" not in src.replace("no atomics", ""), path
    for path in ("_photo_lib.py", os.path.join("libraries", "NeRF", "loss.py"), os.path.join("libraries", "metrics.py"),
                 os.path.join("models", "dso.py")):
        src = open(os.path.join(ROOT, "enarf-gan_amd", path)).read()
        assert "os.environ" not in src and "getenv" not in src, path


def test_abi_argument_checks_need_no_device():
    from enarf_gan_amd import _photo_lib
    L.library("photo")
    lib = _photo_lib.load()
    err = lib.enarf_photo_last_error

    def fwd(color=1, mask=None, grid=1, sc=1, sm=1, B=2, npix=64, N=10, t=0, partials=1, loss=1):
        return lib.enarf_photo_loss_fwd(color, mask, grid, sc, sm, B, npix, N, t, 1.0, 1.0, partials, loss, None)
    assert fwd(t=2) == -1 and b"loss type 2" in err()
    assert fwd(B=-1) == -1 and fwd(N=-1) == -1 and fwd(B=1 << 20, N=1 << 11) == -1
    assert fwd(grid=None) == -1 and b"null grid" in err()
    assert fwd(color=None) == -1 and fwd(sc=None) == -1 and fwd(mask=1, sm=None) == -1
    assert fwd(partials=None) == -1 and fwd(loss=None) == -1
    assert fwd(npix=0) == -1

    def bwd(B=2, N=10, t=0, d_color=1):
        return lib.enarf_photo_loss_bwd(1, None, 1, 1, 1, B, 64, N, t, 1.0, 1.0, None, None, d_color, None, None)
    assert bwd(t=-1) == -1 and bwd(d_color=None) == -1
    assert bwd(B=0) == 0 and bwd(N=0, d_color=None) == 0                     # nothing to write: no launch

    def metrics(B=1, H=64, W=64, gh=64, gw=64, cropped=0, box=None, mask=None, gen_mask=None, n=1 << 20, img=1):
        arr = None if box is None else (C.c_int * len(box))(*box)
        return lib.enarf_photo_metrics(img, 1, mask, gen_mask, B, H, W, gh, gw, cropped, arr, 1, n, 1, None)
    assert metrics(H=6, gh=6) == -1 and b"shorter than the 7 x 7 window" in err()
    assert metrics(box=[0, 0, 6, 30]) == -1 and b"shorter" in err()
    assert metrics(box=[-1, 0, 20, 30]) == -1 and b"outside" in err()
    assert metrics(box=[0, 0, 20, 65]) == -1 and metrics(box=[10, 0, 10, 30]) == -1
    assert metrics(gh=32) == -1 and b"gen_cropped" in err()
    assert metrics(gh=30, gw=20, cropped=1, box=[0, 0, 20, 31]) == -1
    assert metrics(mask=1) == -1 and b"together" in err()
    assert metrics(n=3 * 16 - 1) == -1 and b"partials" in err()
    assert metrics(img=None) == -1
    assert metrics(B=-1) == -1 and metrics(H=0, gh=0) == -1 and metrics(W=1 << 15, gw=1 << 15) == -1
    assert metrics(B=0) == 0


def test_binding_argument_checks_need_no_device():
    from enarf_gan_amd import ops
    from enarf_gan_amd._lib import EnarfHipError
    from enarf_gan_amd.libraries import metrics as M
    from enarf_gan_amd.libraries.NeRF.loss import PhotometricLoss
    B, S, N = 2, 8, 5
    grid, sc, sm = torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, 3, N), torch.zeros(B, N)
    color, mask = torch.zeros(B, 3, S, S), torch.zeros(B, S, S)
    with pytest.raises(ValueError):
        ops.photometric_loss(grid, sc, sm, color, mask, "huber")
    cfg = types.SimpleNamespace(nerf_loss_type="l1", color_coef=1.0, mask_coef=1.0)
    with pytest.raises(ValueError):
        PhotometricLoss(cfg)(grid, sc, sm, color, mask)
    with pytest.raises(ValueError):
        PhotometricLoss(cfg).img_mask_loss(sc, sc, sm, sm)
    for bad in (dict(grid=grid[:, :4]), dict(sm=sm[:1]), dict(color=color[:, :, :, :7]), dict(color=color[:1]),
                dict(mask=mask[:, :7]), dict(sc=sc[:, :2])):
        a = dict(grid=grid, sc=sc, sm=sm, color=color, mask=mask)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.photometric_loss(a["grid"], a["sc"], a["sm"], a["color"], a["mask"])
    with pytest.raises(ValueError):
        ops.photometric_loss(None, sc, sm, color, None)                      # gathered targets must be (B, 3, N)
    # the real image and mask are targets
    with pytest.raises(NotImplementedError):
        ops.photometric_loss(grid, sc, sm, color.clone().requires_grad_(), mask)
    with pytest.raises(NotImplementedError):
        ops.photometric_loss(grid, sc, sm, color, mask.clone().requires_grad_())
    # no CPU fallback
    with pytest.raises(EnarfHipError):
        ops.photometric_loss(grid, sc, sm, color, mask)
    img = torch.zeros(1, 3, 16, 16)
    with pytest.raises(EnarfHipError):
        ops.image_metrics(img, img)
    # metrics
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        ops.image_metrics(torch.zeros(1, 3, 6, 16), torch.zeros(1, 3, 6, 16))
    with pytest.raises(ValueError):
        M.ssim(torch.zeros(1, 3, 16, 5), torch.zeros(1, 3, 16, 5))
    for bbox in ((0, 0, 6, 16), (0, 0, 17, 16), (-1, 0, 8, 8), (4, 4, 4, 12), [(0, 0, 8, 8), (0, 0, 8, 8)]):
        with pytest.raises(ValueError):
            ops.image_metrics(img, img, bbox=bbox)
    with pytest.raises(ValueError):
        ops.image_metrics(img, torch.zeros(1, 3, 8, 8))                      # neither the frame nor the rectangle
    with pytest.raises(ValueError):
        ops.image_metrics(img, img, mask=torch.zeros(1, 16, 16))             # one mask without the other
    with pytest.raises(ValueError):
        ops.image_metrics(img, torch.zeros(2, 3, 16, 16))
    with pytest.raises(ImportError):
        M.lpips(img, img)
    with pytest.raises(ImportError):
        M.neural_actor_lpips(img, img)


def test_validate_refuses_unknown_metrics_before_rendering():
    from enarf_gan_amd.models import dso
    with pytest.raises(ImportError):
        dso.validate(None, [], 64, -1, metric=("SSIM", "LPIPS"))
    with pytest.raises(ValueError):
        dso.validate(None, [], 64, -1, metric=("FID",))
