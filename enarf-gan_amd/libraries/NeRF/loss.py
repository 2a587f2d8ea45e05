"""`PhotometricLoss` of the reference's libraries/NeRF/loss.py:5-48, the only loss of its train_DSO.py: same constructor
(a config with `nerf_loss_type`, `color_coef`, `mask_coef`), same `__call__` and `img_mask_loss`, same return pair.
Gather, difference, reduction and the backward are the HIP kernels of libenarf_photo.so (`ops.photometric_loss`)
instead of a chain of torch ops; the real image and mask are targets and must not require gradients."""
from ... import ops


class PhotometricLoss:
    def __init__(self, config):
        self.config = config

    def __call__(self, grid, sparse_color, sparse_mask, color, mask=None):
        """grid (B, N) int64 ray ids as `mask_based_sampler` returns them, sparse_color (B, 3, N) and sparse_mask (B, N)
        the rendered rays, color (B, 3, S, S) and mask (B, S, S) the real frame -> (loss_color, loss_mask); loss_mask is
        0 without a mask."""
        c = self.config
        return ops.photometric_loss(grid, sparse_color, sparse_mask, color, mask, c.nerf_loss_type, c.color_coef, c.mask_coef)

    def img_mask_loss(self, real_color, nerf_color, real_mask, nerf_mask):
        """The same losses on targets that are already gathered: real_color (B, 3, N), real_mask (B, N) or None."""
        c = self.config
        return ops.photometric_loss(None, nerf_color, nerf_mask, real_color, real_mask, c.nerf_loss_type, c.color_coef,
                                    c.mask_coef)
