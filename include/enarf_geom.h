/*
 * enarf_geom.h - C ABI of libenarf_geom.so: the geometry the march already carries, on the MI355X (gfx950). The march
 * returns a disparity and a mask per ray; this library turns them into a depth map, a camera-space point map, a
 * screen-space normal map and a shape image (enarf_geom_buffers), and keeps the running inverse-depth error of an
 * evaluation set on the device (enarf_geom_err_update). A library of its own; same conventions as enarf_paint.h: raw
 * device pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null stream)
 * with no host synchronisation, no allocation and no environment variable read, 0 on success, a negative ENARF_ERR_*
 * for an argument it rejects (checked on the host before any launch, no device needed) or a positive hipError_t;
 * enarf_geom_last_error() gives the message (thread local).
 *
 * Every value is computed in fp64 from the stored fp32 (the scalars of the argument structure are fp32 too), each
 * operation rounded on its own (no FMA contraction), sums taken in the written order, and rounded to fp32 once when it
 * is stored. Only +, -, *, / and sqrt are used.
 *
 * enarf_geom_buffers. One lane per pixel, one launch per batch, 16 x 16 pixel tiles, no LDS, no
 * atomics. Inputs: disparity q and mask m, (B, H, W) fp32; inv_intrinsics (KB, 3, 3) fp32 with KB = 1 (shared) or B.
 * Pixel (r, c) has x = x0 + (c + 0.5) step, y = y0 + (r + 0.5) step. Per pixel:
 *   valid        q and m finite, m >= mask_threshold and q > 0, compared as fp32;
 *   depth        z = depth_scale (m / q) with `normalise` (the march's disparity is sum w / d, not divided by sum w, so
 *                m / q is the weighted harmonic-mean depth), z = depth_scale / q without (a buffer that holds a
 *                surface's own inverse depth); z = 0 on an invalid pixel;
 *   ray          ray_i = (K[i][0] x + K[i][1] y) + K[i][2], K = inv_intrinsics; point p = z ray (the depth is along the
 *                camera axis, the ray is not normalised);
 *   neighbour    a 4-neighbour is usable when it is inside the image, valid, and |z_n - z| <= edge z (the last test is
 *                skipped when edge < 0);
 *   differences  dx = p(c+1) - p(c-1) when both are usable, else p(c+1) - p(c), else p(c) - p(c-1), else none; dy the
 *                same along r, r + 1 being below;
 *   normal       n = dy x dx (n0 = dy1 dx2 - dy2 dx1, ...), l = sqrt((n0 n0 + n1 n1) + n2 n2), N = n / l, negated when
 *                (N0 p0 + N1 p1) + N2 p2 > 0, so that it faces the camera as the rasteriser's normals do; the normal is
 *                valid when the pixel is valid, both differences exist and 0 < l < inf;
 *   shade 0      normal: rgb = 0.5 + 0.5 (N0, -N1, -N2), needs a valid normal;
 *   shade 1      lit: grey = (0.5 + 0.3 max(c, 0)) + 0.2 s with c = -((N0 p0 + N1 p1) + N2 p2) / max(|p|, 1e-6) and
 *                s = max(2 c c - 1, 0)^64 (six squarings) when c > 0, else 0 - the hard-Phong terms of enarf_raster.h with a
 *                white texel; needs a valid normal;
 *   shade 2      depth: grey = (1 / z - 1 / far) / (1 / near - 1 / far), needs a valid pixel;
 *                a pixel without what the mode needs takes `background`.
 * Outputs, each optional (NULL = not written), at least one required: depth (B, H, W) fp32; points (B, H, W, 3) fp32;
 * normals (B, H, W, 3) fp32, zeros without a valid normal; flags (B, H, W) uint8, bit 0 = valid, bit 1 = normal valid;
 * image (B, H, W, 3) uint8 = floor(255 clamp(v, 0, 1)), a NaN giving 0.
 * 1 <= H, W <= 4096, 1 <= B, B H W < 2^31; shade 2 takes near > 0, far > 0, near != far. No address is formed from a
 * neighbour outside the image. Every output is a function of the inputs alone: two runs give identical bits.
 *
 * enarf_geom_err_update. Adds n = B H W pixels of generated disparity q, optional generated mask m and target inverse
 * depth g (0 = background) to `state`, 8 x 8 bytes on the device:
 *   state[0] int64 n          state[1] fp64 sse_all = sum (q - g)^2      state[2] int64 n_fg = #(g > 0)
 *   state[3] fp64 sse_fg = the same sum over g > 0                       state[4] int64 inter, state[5] int64 union of
 *   the silhouettes (m >= mask_threshold, or q > 0 without a mask) and (g > 0)     state[6] int64 updates   state[7] 0.
 * Two launches: geom_err_partial_kernel writes one record of 8 x 8 bytes per workgroup into `workspace` (lane t of
 * workgroup w takes the pixels w 256 + t + k 256 G in order of k, the 256 lane sums are added by the fixed tree
 * a[t] += a[t + s], s = 128 ... 1); geom_err_finish_kernel, one workgroup, adds the records in index order and adds the
 * totals to `state`. No atomics: identical bits from run to run. G = enarf_geom_err_records(n); `workspace_records` must
 * be at least that. Non-finite values propagate into the sums. 1 <= n < 2^31. A state of zeros is an empty set.
 */
#ifndef ENARF_GEOM_H
#define ENARF_GEOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_GEOM_ABI_VERSION 1

#define ENARF_GEOM_MAX_SIZE      4096   /* H, W */
#define ENARF_GEOM_SHADE_NORMAL  0
#define ENARF_GEOM_SHADE_LIT     1
#define ENARF_GEOM_SHADE_DEPTH   2
#define ENARF_GEOM_FLAG_VALID    1
#define ENARF_GEOM_FLAG_NORMAL   2
#define ENARF_GEOM_STATE_WORDS   8      /* 8-byte words of the error state and of a workspace record */
#define ENARF_GEOM_MAX_RECORDS   1024

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_geom_buffers_args {
    int32_t B, H, W, KB;                        /* KB: matrices in inv_intrinsics, 1 or B */
    int32_t normalise, shade;
    float x0, y0, step;
    float depth_scale, mask_threshold, edge;
    float near_depth, far_depth;                /* shade 2 */
    float background[3];
    int32_t reserved;
    const float *disparity, *mask, *inv_intrinsics;
    float *depth, *points, *normals;            /* optional */
    uint8_t *flags, *image;                     /* optional */
} enarf_geom_buffers_args;

int enarf_geom_abi_version(void);
const char *enarf_geom_last_error(void);

/* depth, points, normals, flags and shape image of a batch of (disparity, mask) maps, one launch on `stream` */
int enarf_geom_buffers(const enarf_geom_buffers_args *args, void *stream);

/* records of 64 bytes the workspace of an update of n pixels must hold; 0 for an n outside [1, 2^31) */
int64_t enarf_geom_err_records(int64_t n);

/* adds n pixels to the running error in `state`, two launches on `stream`; mask may be NULL */
int enarf_geom_err_update(const float *disparity, const float *mask, const float *target, int64_t n, float mask_threshold,
                          void *workspace, int64_t workspace_records, void *state, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_GEOM_H */
