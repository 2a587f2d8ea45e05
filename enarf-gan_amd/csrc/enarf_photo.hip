// enarf_photo.hip - photometric loss and image metrics of the single-scene path (libenarf_photo.so,
// include/enarf_photo.h).
//
// Loss forward: photo_loss_kernel, one thread per ray (grid-stride, at most ENARF_PHOTO_LOSS_MAX_BLOCKS workgroups),
// gathers the ray's three target texels and its target mask value through `grid` and accumulates both sums in fp64;
// each workgroup writes one partial per sum. photo_loss_finish_kernel (one workgroup) adds the partials and writes
// the two fp32 losses. Loss backward: photo_loss_bwd_kernel, one thread per ray, gathers the same texels and writes
// the ray's four gradients from the upstream scalars it reads from device memory.
//
// Metrics: photo_metrics_kernel, one workgroup of 16 x 16 threads per 16 x 16 pixel tile of an image's rectangle. The
// tile and a 3-pixel halo of both images (three channels) are staged in LDS as fp32; per channel the five window
// moments (x, y, xx, yy, xy of the images mapped to [0, 1]) are formed in fp64 as exact 7-tap sums along the rows
// (22 x 16 row sums in LDS), then along the columns by the thread that owns the pixel, which evaluates S there. The
// workgroup reduces S, the squared colour error and the squared mask error of its pixels to three fp64 partials;
// photo_metrics_finish_kernel (one workgroup per image) adds an image's partials and writes its four fp32 results.
//
// Every sum has a fixed order: a thread's own terms in index order, 64 lanes by a shuffle tree, four waves left to
// right, partials by strided lanes in index order and the same tree. Nothing depends on scheduling, so every output
// is a function of the inputs alone.
#include "enarf_photo.h"
#include "enarf_device.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

using enarf::block_sum;

constexpr int kBlock = 256;
constexpr int kTile = ENARF_PHOTO_TILE;
constexpr int kHalo = ENARF_PHOTO_WINDOW / 2;           // 3
constexpr int kWin = ENARF_PHOTO_WINDOW;
constexpr int kStage = kTile + 2 * kHalo;               // 22 rows / columns staged per tile
constexpr int kStagePitch = kStage + 1;
constexpr int kChunk = 32;                              // images per metrics launch (their rectangles ride in the arguments)
static_assert(kTile * kTile == kBlock, "one thread per tile pixel");

// ------------------------------------------------------------------------------------------------------- loss
struct LossArgs {
    const float *color, *mask;
    const long long *grid;
    const float *sparse_color, *sparse_mask;
    long long B, npix, N;
    int mae;
    double color_coef, mask_coef;
};

__global__ __launch_bounds__(kBlock) void photo_loss_kernel(LossArgs a, double *partials) {
    __shared__ double red[4];
    const long long total = a.B * a.N;
    double sum_c = 0.0, sum_m = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const long long b = i / a.N, n = i - b * a.N;
        const long long id = a.grid ? a.grid[i] : n;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = (double)a.color[(b * 3 + c) * a.npix + id] - (double)a.sparse_color[(b * 3 + c) * a.N + n];
            sum_c += a.mae ? fmax(fabs(d), ENARF_PHOTO_MAE_THRESHOLD) : d * d;
        }
        if (a.mask) {
            const double d = (double)a.mask[b * a.npix + id] - (double)a.sparse_mask[i];
            sum_m += d * d;
        }
    }
    sum_c = block_sum(sum_c, red);
    sum_m = block_sum(sum_m, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sum_c;
        partials[ENARF_PHOTO_LOSS_MAX_BLOCKS + blockIdx.x] = sum_m;
    }
}

__global__ __launch_bounds__(kBlock) void photo_loss_finish_kernel(const double *partials, int blocks, double n_color,
                                                                   double n_mask, double color_coef, double mask_coef,
                                                                   int has_mask, float *loss) {
    __shared__ double red[4];
    double sum_c = 0.0, sum_m = 0.0;
    for (int k = threadIdx.x; k < blocks; k += kBlock) {
        sum_c += partials[k];
        sum_m += partials[ENARF_PHOTO_LOSS_MAX_BLOCKS + k];
    }
    sum_c = block_sum(sum_c, red);
    sum_m = block_sum(sum_m, red);
    if (threadIdx.x == 0) {
        loss[0] = (float)(sum_c / n_color * color_coef);
        loss[1] = has_mask ? (float)(sum_m / n_mask * mask_coef) : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void photo_loss_bwd_kernel(LossArgs a, const float *g_color, const float *g_mask,
                                                                float *d_sparse_color, float *d_sparse_mask) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.B * a.N) return;
    const long long b = i / a.N, n = i - b * a.N;
    const long long id = a.grid ? a.grid[i] : n;
    const double gc = (g_color ? (double)*g_color : 0.0) * a.color_coef / (3.0 * (double)a.B * (double)a.N);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // d = s - t: the derivative of (t - s)^2 in s is 2 d, that of |t - s| is sign(d)
        const double d = (double)a.sparse_color[(b * 3 + c) * a.N + n] - (double)a.color[(b * 3 + c) * a.npix + id];
        double g;
        if (a.mae)
            g = fabs(d) >= ENARF_PHOTO_MAE_THRESHOLD ? (d > 0.0 ? gc : (d < 0.0 ? -gc : 0.0)) : 0.0;
        else
            g = gc * (2.0 * d);
        d_sparse_color[(b * 3 + c) * a.N + n] = (float)g;
    }
    if (a.mask && d_sparse_mask) {
        const double gm = (g_mask ? (double)*g_mask : 0.0) * a.mask_coef / ((double)a.B * (double)a.N);
        const double d = (double)a.sparse_mask[i] - (double)a.mask[b * a.npix + id];
        d_sparse_mask[i] = (float)(gm * (2.0 * d));
    }
}

// ------------------------------------------------------------------------------------------------------- metrics
struct MetricArgs {
    const float *img, *gen, *mask, *gen_mask;
    long long image0;                 // first image of this launch
    int H, W, gen_h, gen_w, gen_cropped;
    int tiles_stride;                 // tiles reserved per image in `partials`
    int box[kChunk][4];               // (x0, y0, x1, y1) of the launch's images
};

__device__ __forceinline__ int tiles_of(int n) { return (n + kTile - 1) / kTile; }

__global__ __launch_bounds__(kBlock) void photo_metrics_kernel(MetricArgs a, double *partials) {
    __shared__ float in[2][3][kStage][kStagePitch];
    __shared__ double hs[5][kStage][kTile];
    __shared__ double red[4];
    const int bl = blockIdx.y;
    const int x0 = a.box[bl][0], y0 = a.box[bl][1];
    const int w = a.box[bl][2] - x0, h = a.box[bl][3] - y0;
    const int tiles_x = tiles_of(w);
    const int tile = blockIdx.x;
    if (tile >= tiles_x * tiles_of(h)) return;          // the grid is sized for the launch's largest rectangle
    const long long ib = a.image0 + bl;
    const int oy = (tile / tiles_x) * kTile, ox = (tile % tiles_x) * kTile;   // rectangle-relative origin of the tile
    const int gy0 = a.gen_cropped ? 0 : y0, gx0 = a.gen_cropped ? 0 : x0;
    const int tid = threadIdx.x;

    for (int idx = tid; idx < 6 * kStage * kStage; idx += kBlock) {
        const int plane = idx / (kStage * kStage), rem = idx - plane * (kStage * kStage);
        const int which = plane / 3, c = plane - which * 3;
        const int r = rem / kStage, q = rem - r * kStage;
        const int ry = oy - kHalo + r, rx = ox - kHalo + q;
        float v = 0.0f;                                 // outside the rectangle: never part of an interior window
        if (ry >= 0 && ry < h && rx >= 0 && rx < w) {
            v = which == 0 ? a.img[((size_t)(ib * 3 + c) * a.H + (y0 + ry)) * a.W + (x0 + rx)]
                           : a.gen[((size_t)(ib * 3 + c) * a.gen_h + (gy0 + ry)) * a.gen_w + (gx0 + rx)];
        }
        in[which][c][r][q] = v;
    }
    __syncthreads();

    const int ly = tid / kTile, lx = tid - ly * kTile;
    const int py = oy + ly, px = ox + lx;
    const bool owned = py < h && px < w;
    const bool interior = py >= kHalo && py < h - kHalo && px >= kHalo && px < w - kHalo;
    double sq_c = 0.0, sq_m = 0.0, ssim = 0.0;
    if (owned) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = (double)in[0][c][ly + kHalo][lx + kHalo] - (double)in[1][c][ly + kHalo][lx + kHalo];
            sq_c += d * d;
        }
        if (a.mask) {
            const double d = (double)a.mask[((size_t)ib * a.H + (y0 + py)) * a.W + (x0 + px)] -
                             (double)a.gen_mask[((size_t)ib * a.gen_h + (gy0 + py)) * a.gen_w + (gx0 + px)];
            sq_m = d * d;
        }
    }
    constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03;       // (K data_range)^2, data_range 1
    constexpr double kNP = (double)(kWin * kWin), kCov = kNP / (kNP - 1.0);
    for (int c = 0; c < 3; ++c) {
        for (int idx = tid; idx < kStage * kTile; idx += kBlock) {
            const int r = idx / kTile, q = idx - r * kTile;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const double x = (double)in[0][c][r][q + k] * 0.5 + 0.5, y = (double)in[1][c][r][q + k] * 0.5 + 0.5;
                sx += x, sy += y, sxx += x * x, syy += y * y, sxy += x * y;
            }
            hs[0][r][q] = sx, hs[1][r][q] = sy, hs[2][r][q] = sxx, hs[3][r][q] = syy, hs[4][r][q] = sxy;
        }
        __syncthreads();
        if (interior) {
            double m[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < kWin; ++k) s += hs[j][ly + k][lx];
                m[j] = s / kNP;
            }
            const double ux = m[0], uy = m[1];
            const double vx = kCov * (m[2] - ux * ux), vy = kCov * (m[3] - uy * uy), vxy = kCov * (m[4] - ux * uy);
            ssim += ((2.0 * ux * uy + kC1) * (2.0 * vxy + kC2)) / ((ux * ux + uy * uy + kC1) * (vx + vy + kC2));
        }
        __syncthreads();                                // the next channel overwrites hs
    }
    ssim = block_sum(ssim, red);
    sq_c = block_sum(sq_c, red);
    sq_m = block_sum(sq_m, red);
    if (tid == 0) {
        double *p = partials + ((size_t)ib * a.tiles_stride + tile) * 3;
        p[0] = ssim, p[1] = sq_c, p[2] = sq_m;
    }
}

__global__ __launch_bounds__(kBlock) void photo_metrics_finish_kernel(MetricArgs a, const double *partials, float *out) {
    __shared__ double red[4];
    const int bl = blockIdx.x;
    const long long ib = a.image0 + bl;
    const int w = a.box[bl][2] - a.box[bl][0], h = a.box[bl][3] - a.box[bl][1];
    const int tiles = tiles_of(w) * tiles_of(h);
    const double *p = partials + (size_t)ib * a.tiles_stride * 3;
    double ssim = 0.0, sq_c = 0.0, sq_m = 0.0;
    for (int k = threadIdx.x; k < tiles; k += kBlock) ssim += p[k * 3], sq_c += p[k * 3 + 1], sq_m += p[k * 3 + 2];
    ssim = block_sum(ssim, red);
    sq_c = block_sum(sq_c, red);
    sq_m = block_sum(sq_m, red);
    if (threadIdx.x == 0) {
        const double area = (double)h * (double)w;
        const double mse = sq_c / (3.0 * area);
        float *o = out + ib * 4;
        o[0] = (float)(ssim / (3.0 * (double)(h - 2 * kHalo) * (double)(w - 2 * kHalo)));
        o[1] = (float)mse;
        o[2] = (float)(20.0 * log10(2.0) - 10.0 * log10(mse));
        o[3] = a.mask ? (float)(sq_m / area) : nanf("");
    }
}

int check_loss_args(const char *who, const float *color, const int64_t *grid, const float *sparse_color,
                    const float *sparse_mask, const float *mask, int64_t B, int64_t npix, int64_t N, int loss_type) {
    if (loss_type != ENARF_PHOTO_MSE && loss_type != ENARF_PHOTO_MAE)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: loss type %d is neither ENARF_PHOTO_MSE nor ENARF_PHOTO_MAE", who,
                                 loss_type);
    if (B < 0 || N < 0 || npix < 0 || B >= (1LL << 31) || N >= (1LL << 31) || B * N >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: B %lld, N %lld outside 0 <= B, N and B * N < 2^31", who,
                                 (long long)B, (long long)N);
    if (npix >= (1LL << 40)) return enarf::host::fail(ENARF_ERR_ARG, "%s: npix %lld too large", who, (long long)npix);
    if (B * N > 0 && npix == 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: rays but an empty image", who);
    if (!grid && npix != N)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: a null grid needs npix == N, got %lld and %lld", who,
                                 (long long)npix, (long long)N);
    if (B * N > 0 && (!color || !sparse_color || (mask && !sparse_mask)))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null color, sparse_color, or sparse_mask beside a mask", who);
    return 0;
}

}  // namespace

extern "C" {

int enarf_photo_abi_version(void) { return ENARF_PHOTO_ABI_VERSION; }

const char *enarf_photo_last_error(void) { return enarf::host::last_error(); }

int enarf_photo_loss_fwd(const float *color, const float *mask, const int64_t *grid, const float *sparse_color,
                         const float *sparse_mask, int64_t B, int64_t npix, int64_t N, int loss_type,
                         double color_coef, double mask_coef, double *partials, float *loss, void *stream) {
    const char *who = "enarf_photo_loss_fwd";
    if (const int rc = check_loss_args(who, color, grid, sparse_color, sparse_mask, mask, B, npix, N, loss_type)) return rc;
    if (!partials || !loss) return enarf::host::fail(ENARF_ERR_ARG, "%s: null partials or loss", who);
    const LossArgs a{color, mask, reinterpret_cast<const long long *>(grid), sparse_color, sparse_mask,
                     (long long)B, (long long)npix, (long long)N, loss_type == ENARF_PHOTO_MAE, color_coef, mask_coef};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long total = (long long)B * N;
    long long blocks = (total + kBlock - 1) / kBlock;
    if (blocks > ENARF_PHOTO_LOSS_MAX_BLOCKS) blocks = ENARF_PHOTO_LOSS_MAX_BLOCKS;
    if (blocks > 0) {
        hipLaunchKernelGGL(photo_loss_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, a, partials);
        if (const int rc = enarf::host::check_launch("enarf_photo_loss_fwd: photo_loss_kernel")) return rc;
    }
    hipLaunchKernelGGL(photo_loss_finish_kernel, dim3(1), dim3(kBlock), 0, st, partials, (int)blocks,
                       3.0 * (double)total, (double)total, color_coef, mask_coef, mask != nullptr, loss);
    return enarf::host::check_launch("enarf_photo_loss_fwd: photo_loss_finish_kernel");
}

int enarf_photo_loss_bwd(const float *color, const float *mask, const int64_t *grid, const float *sparse_color,
                         const float *sparse_mask, int64_t B, int64_t npix, int64_t N, int loss_type,
                         double color_coef, double mask_coef, const float *g_color, const float *g_mask,
                         float *d_sparse_color, float *d_sparse_mask, void *stream) {
    const char *who = "enarf_photo_loss_bwd";
    if (const int rc = check_loss_args(who, color, grid, sparse_color, sparse_mask, mask, B, npix, N, loss_type)) return rc;
    const long long total = (long long)B * N;
    if (total == 0) return 0;
    if (!d_sparse_color) return enarf::host::fail(ENARF_ERR_ARG, "%s: null d_sparse_color", who);
    const LossArgs a{color, mask, reinterpret_cast<const long long *>(grid), sparse_color, sparse_mask,
                     (long long)B, (long long)npix, (long long)N, loss_type == ENARF_PHOTO_MAE, color_coef, mask_coef};
    hipLaunchKernelGGL(photo_loss_bwd_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a, g_color, g_mask, d_sparse_color, d_sparse_mask);
    return enarf::host::check_launch("enarf_photo_loss_bwd: photo_loss_bwd_kernel");
}

int enarf_photo_metrics(const float *img, const float *gen, const float *mask, const float *gen_mask, int64_t B,
                        int H, int W, int gen_h, int gen_w, int gen_cropped, const int *bbox, double *partials,
                        int64_t n_partials, float *out, void *stream) {
    const char *who = "enarf_photo_metrics";
    if (B < 0 || B >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: batch %lld outside [0, 2^31)", who, (long long)B);
    if (H < 1 || W < 1 || H > ENARF_PHOTO_MAX_SIDE || W > ENARF_PHOTO_MAX_SIDE)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: frame %d x %d outside [1, %d]", who, H, W, ENARF_PHOTO_MAX_SIDE);
    if (!gen_cropped && (gen_h != H || gen_w != W))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: gen is %d x %d, img %d x %d, and gen_cropped is not set", who,
                                 gen_h, gen_w, H, W);
    if ((mask == nullptr) != (gen_mask == nullptr))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: mask and gen_mask come together or not at all", who);
    int max_tiles = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int x0 = bbox ? bbox[b * 4] : 0, y0 = bbox ? bbox[b * 4 + 1] : 0;
        const int x1 = bbox ? bbox[b * 4 + 2] : W, y1 = bbox ? bbox[b * 4 + 3] : H;
        if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x1 <= x0 || y1 <= y0)
            return enarf::host::fail(ENARF_ERR_ARG, "%s: image %lld: rectangle (%d, %d, %d, %d) outside the %d x %d frame",
                                     who, (long long)b, x0, y0, x1, y1, H, W);
        if (x1 - x0 < ENARF_PHOTO_WINDOW || y1 - y0 < ENARF_PHOTO_WINDOW)
            return enarf::host::fail(ENARF_ERR_ARG, "%s: image %lld: rectangle %d x %d has a side shorter than the "
                                     "%d x %d window", who, (long long)b, y1 - y0, x1 - x0, ENARF_PHOTO_WINDOW,
                                     ENARF_PHOTO_WINDOW);
        if (gen_cropped && (gen_h != y1 - y0 || gen_w != x1 - x0))
            return enarf::host::fail(ENARF_ERR_ARG, "%s: image %lld: gen is %d x %d but its rectangle %d x %d", who,
                                     (long long)b, gen_h, gen_w, y1 - y0, x1 - x0);
        const int tiles = ENARF_PHOTO_METRIC_PARTIALS(y1 - y0, x1 - x0) / 3;
        if (tiles > max_tiles) max_tiles = tiles;
    }
    if (B == 0) return 0;
    if (!img || !gen || !partials || !out)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null img, gen, partials or out", who);
    if (n_partials < (int64_t)B * 3 * max_tiles)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: partials holds %lld doubles, %lld are needed", who,
                                 (long long)n_partials, (long long)B * 3 * max_tiles);
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t b0 = 0; b0 < B; b0 += kChunk) {
        const int n = (int)(B - b0 < kChunk ? B - b0 : kChunk);
        MetricArgs a{img, gen, mask, gen_mask, (long long)b0, H, W, gen_h, gen_w, gen_cropped, max_tiles, {}};
        for (int i = 0; i < n; ++i) {
            const int *bx = bbox ? bbox + (b0 + i) * 4 : nullptr;
            a.box[i][0] = bx ? bx[0] : 0, a.box[i][1] = bx ? bx[1] : 0;
            a.box[i][2] = bx ? bx[2] : W, a.box[i][3] = bx ? bx[3] : H;
        }
        hipLaunchKernelGGL(photo_metrics_kernel, dim3((unsigned)max_tiles, (unsigned)n), dim3(kBlock), 0, st, a, partials);
        if (const int rc = enarf::host::check_launch("enarf_photo_metrics: photo_metrics_kernel")) return rc;
        hipLaunchKernelGGL(photo_metrics_finish_kernel, dim3((unsigned)n), dim3(kBlock), 0, st, a, partials, out);
        if (const int rc = enarf::host::check_launch("enarf_photo_metrics: photo_metrics_finish_kernel")) return rc;
    }
    return 0;
}

}  // extern "C"
