/*
 * enarf_photo.h - C ABI of libenarf_photo.so: the supervision of the single-scene (DSO) path on the MI355X (gfx950) -
 * the photometric loss of the reference's libraries/NeRF/loss.py (forward and backward) and the per-image validation
 * metrics of its libraries/metrics.py (SSIM as scikit-image's structural_similarity computes it for that call, MSE,
 * PSNR). A library of its own, next to libenarf_hip.so, libenarf_mesh.so, libenarf_raster.so and libenarf_pose.so; same
 * conventions as enarf_pose.h: raw device pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed
 * as void*, NULL = the null stream) with no host synchronisation, 0 on success, a negative ENARF_ERR_* for an argument
 * it rejects (checked on the host, no device needed) or a positive hipError_t; enarf_photo_last_error() gives the
 * message (thread local).
 *
 * Contract. All tensors are fp32 row-major on the device unless said otherwise; all arithmetic is
 * fp64 and a result is rounded to fp32 once, when it is stored. Sums are reduced in a fixed order (a thread's terms in
 * index order, a fixed tree over the workgroup, per-workgroup fp64 partials in `partials`, finished by a second launch
 * in a fixed order; no atomics), so every output is bit-identical from run to run.
 *
 * Photometric loss. color (B, 3, npix) is the real image, mask (B, npix) the real foreground mask or null, grid (B, N)
 * int64 the flat pixel id of each ray, sparse_color (B, 3, N) and sparse_mask (B, N) the rendered rays. Every id must
 * lie in [0, npix): the kernels clamp nothing (as torch.gather requires). A null grid stands for id = ray index
 * (npix == N: the targets are already gathered). With t = the target gathered through grid and s = the rendered value:
 *   ENARF_PHOTO_MSE   loss[0] = color_coef * mean (t - s)^2           over the B * 3 * N colour values
 *   ENARF_PHOTO_MAE   loss[0] = color_coef * mean max(|t - s|, 0.01)  (the reference's truncated MAE)
 *   loss[1] = mask_coef * mean (t - s)^2 over the B * N mask values, or 0 when mask is null.
 * Backward, from the upstream gradients g[0], g[1] of loss[0], loss[1] (device scalars, read on the device; a null
 * pointer is a zero gradient):
 *   MSE   d sparse_color = g[0] * color_coef * 2 (s - t) / (3 B N)
 *   MAE   d sparse_color = g[0] * color_coef * sign(s - t) / (3 B N) where |t - s| >= 0.01, else 0 (torch's rule for
 *         clamp_min: the gradient passes at the tie; sign(0) = 0)
 *   d sparse_mask = g[1] * mask_coef * 2 (s - t) / (B N); not written when mask or d_sparse_mask is null.
 * The targets get no gradient. 0 <= B, N and B * N < 2^31; B * N == 0 gives NaN losses (the mean of nothing).
 * `partials` is scratch of at least ENARF_PHOTO_LOSS_PARTIALS doubles.
 *
 * Metrics. img (B, 3, H, W) and gen are images in [-1, 1]; mask (B, H, W) and gen_mask are optional (both or
 * neither). Image b is scored over the rectangle rows [y0, y1) x columns [x0, x1) of bbox[b] = (x0, y0, x1, y1), a HOST
 * array of B * 4 ints (null = the whole frame), read in place. gen and gen_mask are either frames of the same H x W
 * (gen_cropped = 0: the same rectangle is read) or already cropped to the rectangle (gen_cropped = 1: gen is
 * (B, 3, gen_h, gen_w) with gen_h == y1 - y0 and gen_w == x1 - x0 for every image). out (B, 4) is, per image,
 *   out[0] SSIM: x -> x * 0.5 + 0.5, data_range 1, 7 x 7 uniform window, sample covariance (49 / 48), K1 0.01, K2 0.03,
 *          S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) per channel, averaged over the
 *          pixels at least 3 from every side of the rectangle and over the 3 channels. The window moments are exact
 *          7-tap sums in fp64, so vx = uxx - ux^2 cancels in fp64.
 *   out[1] mse_color: mean (img - gen)^2 over the 3 channels of the rectangle, on the [-1, 1] values
 *   out[2] psnr = 20 log10(2) - 10 log10(mse_color)            (+inf for identical images)
 *   out[3] mse_mask: mean (mask - gen_mask)^2 over the rectangle, NaN when no masks are given.
 * A rectangle side shorter than 7 (the window) or outside the frame is ENARF_ERR_ARG. `partials` is scratch of at
 * least B * ENARF_PHOTO_METRIC_PARTIALS(max rectangle height, max rectangle width) doubles; its size is passed in
 * n_partials and checked.
 */
#ifndef ENARF_PHOTO_H
#define ENARF_PHOTO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_PHOTO_ABI_VERSION 1

#define ENARF_PHOTO_MSE 0
#define ENARF_PHOTO_MAE 1
#define ENARF_PHOTO_MAE_THRESHOLD 0.01

#define ENARF_PHOTO_LOSS_MAX_BLOCKS 1024
#define ENARF_PHOTO_LOSS_PARTIALS   (2 * ENARF_PHOTO_LOSS_MAX_BLOCKS)

#define ENARF_PHOTO_WINDOW   7      /* SSIM window; a rectangle side must be at least this */
#define ENARF_PHOTO_TILE     16     /* a workgroup owns a 16 x 16 pixel tile of the rectangle */
#define ENARF_PHOTO_MAX_SIDE 16384
#define ENARF_PHOTO_METRIC_PARTIALS(h, w) \
    (3 * (((h) + ENARF_PHOTO_TILE - 1) / ENARF_PHOTO_TILE) * (((w) + ENARF_PHOTO_TILE - 1) / ENARF_PHOTO_TILE))

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

int enarf_photo_abi_version(void);
const char *enarf_photo_last_error(void);

/* loss[0], loss[1]: one gather-and-reduce launch and one finishing launch on `stream` */
int enarf_photo_loss_fwd(const float *color, const float *mask, const int64_t *grid, const float *sparse_color,
                         const float *sparse_mask, int64_t B, int64_t npix, int64_t N, int loss_type,
                         double color_coef, double mask_coef, double *partials, float *loss, void *stream);

/* d_sparse_color (B, 3, N) and d_sparse_mask (B, N) from the device scalars g_color, g_mask: one launch */
int enarf_photo_loss_bwd(const float *color, const float *mask, const int64_t *grid, const float *sparse_color,
                         const float *sparse_mask, int64_t B, int64_t npix, int64_t N, int loss_type,
                         double color_coef, double mask_coef, const float *g_color, const float *g_mask,
                         float *d_sparse_color, float *d_sparse_mask, void *stream);

/* out (B, 4) = [ssim, mse_color, psnr, mse_mask] per image: one tile launch and one finishing launch per 32 images */
int enarf_photo_metrics(const float *img, const float *gen, const float *mask, const float *gen_mask, int64_t B,
                        int H, int W, int gen_h, int gen_w, int gen_cropped, const int *bbox, double *partials,
                        int64_t n_partials, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_PHOTO_H */
