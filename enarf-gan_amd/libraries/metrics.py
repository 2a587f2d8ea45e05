"""Validation metrics of the reference's libraries/metrics.py:8-33 on the device: `ssim` and `psnr` keep its signatures
and return types, `image_metrics` is what a validation loop should call (every figure of every image in one device
tensor, no synchronisation). SSIM is scikit-image's `structural_similarity(x * 0.5 + 0.5, data_range=1)` for 3-channel
images - 7 x 7 uniform window, sample covariance, K1 0.01, K2 0.03, mean over the pixels 3 from every side - computed by
libenarf_photo.so (contract: include/enarf_photo.h). LPIPS needs the `lpips` / `lpips_pytorch` packages and their
network weights, as in the reference; without them `lpips` and `neural_actor_lpips` raise ImportError."""
from .. import ops

image_metrics = ops.image_metrics


def ssim(img1, img2):
    """SSIM of image 0 of the two (B, 3, H, W) batches in [-1, 1], as a Python float (metrics.py:8-11)."""
    return image_metrics(img1[:1], img2[:1])[0, 0].item()


def psnr(img1, img2):
    """20 log10(2) - 10 log10(mse) with the MSE over the whole batch, as a Python float (metrics.py:14-16)."""
    mse = image_metrics(img1, img2)[:, 1].double().mean().item()     # equal-sized images: the mean of their MSEs
    import numpy as np
    return 20 * np.log10(2) - 10 * np.log10(mse)


def lpips(img1, img2):
    import lpips as _lpips  # noqa: F401  (not a dependency of this package: raises ImportError when absent)
    raise ImportError("lpips is installed but its VGG weights are not wired into this package")


def neural_actor_lpips(img1, img2):
    from lpips_pytorch import LPIPS  # noqa: F401  (as above)
    raise ImportError("lpips_pytorch is installed but its AlexNet weights are not wired into this package")


def inv_depth_mse(gen_disparity, gt_disparity):
    """Mean squared error between generated and ground-truth inverse-depth maps of equal shape, as a Python float: what
    the reference's evaluation/compute_depth.py:69-77 computes with MSELoss on the host, summed in fp64 on the device by
    libenarf_geom.so (one host read). For a whole evaluation set keep an ops.DepthError and call result() once."""
    return ops.DepthError().update(gen_disparity, gt_disparity).result()["inv_depth_mse"]
