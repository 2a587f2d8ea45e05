"""Float64 restatement, in plain numpy, of the two contracts of include/enarf_photo.h: the photometric loss of the
reference's libraries/NeRF/loss.py with its gradients, and the image metrics of its libraries/metrics.py (SSIM as
scikit-image's structural_similarity computes it for that call). It is the referee of the CPU and GPU tests; it never
sees a kernel."""
import numpy as np

MAE_THRESHOLD = 0.01
WINDOW = 7
K1, K2 = 0.01, 0.03


# ------------------------------------------------------------------------------------------------------- loss
def gather(color, mask, grid):
    """targets of the rays: color (B, 3, S, S) -> (B, 3, N), mask (B, S, S) or None -> (B, N) or None"""
    B = color.shape[0]
    flat = np.asarray(color, np.float64).reshape(B, 3, -1)
    t_color = np.take_along_axis(flat, np.repeat(grid[:, None, :], 3, axis=1), axis=2)
    t_mask = None if mask is None else np.take_along_axis(np.asarray(mask, np.float64).reshape(B, -1), grid, axis=1)
    return t_color, t_mask


def loss(grid, sparse_color, sparse_mask, color, mask, loss_type, color_coef, mask_coef):
    """(loss_color, loss_mask) in float64; loss_mask is 0 without a mask"""
    t_color, t_mask = gather(color, mask, grid)
    d = t_color - np.asarray(sparse_color, np.float64)
    if loss_type == "mse":
        loss_color = np.mean(d * d) * color_coef
    elif loss_type == "mae":
        loss_color = np.mean(np.maximum(np.abs(d), MAE_THRESHOLD)) * color_coef
    else:
        raise ValueError(loss_type)
    if t_mask is None:
        return loss_color, 0.0
    dm = t_mask - np.asarray(sparse_mask, np.float64)
    return loss_color, np.mean(dm * dm) * mask_coef


def loss_grad(grid, sparse_color, sparse_mask, color, mask, loss_type, color_coef, mask_coef, g_color=1.0, g_mask=1.0):
    """(d sparse_color, d sparse_mask or None) for the upstream gradients g_color, g_mask; the truncated MAE passes the
    gradient where |t - s| >= the threshold (torch's clamp_min rule)"""
    t_color, t_mask = gather(color, mask, grid)
    d = np.asarray(sparse_color, np.float64) - t_color
    if loss_type == "mse":
        g = 2.0 * d
    elif loss_type == "mae":
        g = np.sign(d) * (np.abs(d) >= MAE_THRESHOLD)
    else:
        raise ValueError(loss_type)
    d_color = g * (g_color * color_coef / d.size)
    if t_mask is None:
        return d_color, None
    dm = np.asarray(sparse_mask, np.float64) - t_mask
    return d_color, 2.0 * dm * (g_mask * mask_coef / dm.size)


def mae_tie_margin(grid, sparse_color, color):
    """smallest distance of |t - s| from the MAE threshold (tests keep away from the tie)"""
    t_color, _ = gather(color, None, grid)
    return np.abs(np.abs(t_color - np.asarray(sparse_color, np.float64)) - MAE_THRESHOLD).min()


# ------------------------------------------------------------------------------------------------------- metrics
def window_means(a, win=WINDOW):
    """mean of every full win x win window of the last two axes, by cumulative sums: (..., H, W) -> (..., H - win + 1,
    W - win + 1); entry (i, j) is the window centred on pixel (i + win // 2, j + win // 2)"""
    a = np.asarray(a, np.float64)
    c = np.cumsum(np.cumsum(a, axis=-2), axis=-1)
    c = np.pad(c, [(0, 0)] * (a.ndim - 2) + [(1, 0), (1, 0)])
    s = c[..., win:, win:] - c[..., :-win, win:] - c[..., win:, :-win] + c[..., :-win, :-win]
    return s / (win * win)


def window_means_direct(a, win=WINDOW):
    """the same by adding the win^2 shifted copies (no cancellation): the check of `window_means`"""
    a = np.asarray(a, np.float64)
    H, W = a.shape[-2:]
    s = np.zeros(a.shape[:-2] + (H - win + 1, W - win + 1))
    for i in range(win):
        for j in range(win):
            s += a[..., i:i + H - win + 1, j:j + W - win + 1]
    return s / (win * win)


def ssim_map(x, y, means=window_means_direct):
    """S of scikit-image's structural_similarity at every pixel whose window lies inside the image, for images already
    in [0, 1] (data_range 1): (..., H, W) -> (..., H - 6, W - 6)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = WINDOW * WINDOW
    cov_norm = n / (n - 1.0)
    ux, uy = means(x), means(y)
    uxx, uyy, uxy = means(x * x), means(y * y), means(x * y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = K1 ** 2, K2 ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))


def ssim(img, gen):
    """SSIM of two (3, h, w) images in [-1, 1]: per channel the mean of S over the interior, then the channels' mean"""
    x, y = np.asarray(img, np.float64) * 0.5 + 0.5, np.asarray(gen, np.float64) * 0.5 + 0.5
    if min(x.shape[-2:]) < WINDOW:
        raise ValueError("win_size exceeds image extent")
    return float(np.mean([ssim_map(x[c], y[c]).mean() for c in range(x.shape[0])]))


def ssim_constant(a, b):
    """closed form for two constant images of values a, b in [-1, 1]: the variances vanish"""
    x, y, C1 = a * 0.5 + 0.5, b * 0.5 + 0.5, K1 ** 2
    return (2 * x * y + C1) / (x * x + y * y + C1)


def image_metrics(img, gen, mask=None, gen_mask=None, bbox=None):
    """[ssim, mse_color, psnr, mse_mask] of one image pair (3, H, W) over bbox = (x0, y0, x1, y1), float64"""
    x0, y0, x1, y1 = bbox if bbox is not None else (0, 0, img.shape[-1], img.shape[-2])
    a = np.asarray(img, np.float64)[:, y0:y1, x0:x1]
    g = np.asarray(gen, np.float64)
    g = g[:, y0:y1, x0:x1] if g.shape == np.shape(img) else g
    mse = np.mean((a - g) ** 2)
    with np.errstate(divide="ignore"):
        psnr = 20 * np.log10(2.0) - 10 * np.log10(mse)
    if mask is None:
        mse_mask = np.nan
    else:
        m, gm = np.asarray(mask, np.float64)[y0:y1, x0:x1], np.asarray(gen_mask, np.float64)
        gm = gm[y0:y1, x0:x1] if gm.shape == np.shape(mask) else gm
        mse_mask = np.mean((m - gm) ** 2)
    return np.array([ssim(a, g), mse, psnr, mse_mask])
