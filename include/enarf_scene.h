/*
 * enarf_scene.h - C ABI of libenarf_scene.so: several avatars in one image, on the MI355X (gfx950). K avatars are marched
 * on the same n rays of one camera (the march's own fine samples: depth, density and colour taps and the ray validity);
 * enarf_scene_composite turns the K sample lists of every ray into one colour, mask and disparity, the share of the mask
 * each avatar carries and the avatar that owns the pixel. A library of its own; same conventions as enarf_geom.h: raw
 * device pointers and sizes, the call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null stream)
 * with no host synchronisation, no allocation and no environment variable read, 0 on success, a negative ENARF_ERR_*
 * for an argument it rejects (checked on the host before any launch, no device needed) or a positive hipError_t;
 * enarf_scene_last_error() gives the message (thread local).
 *
 * enarf_scene_composite. One wavefront per (frame, ray), one launch for all F frames, no atomics.
 * Inputs, fp32, in the layouts the march's outputs have for a batch of F K images: depth d and density s (F, K, n, Nf),
 * colour c (F, K, 3, n, Nf), valid (F, K, n) uint8 or NULL (= every byte 1).
 *
 * Avatar k as a medium on a ray (the quadrature of the march's own compositing): D[i] = max(D[i - 1], d[i]) is the
 * running maximum of its depths; its density is s[i] and its colour c[i] on [D[i], D[i + 1]) for i < Nf - 1, and the
 * density is zero before D[0] and from D[Nf - 1] on (the last sample only closes an interval).
 *
 * An avatar takes no part on a ray where its validity byte is 0. Where the byte is not 0 it is screened: when any of its
 * Nf depths, densities or 3 Nf colours on the ray is not finite, a depth is <= 0 or a density is < 0, it takes no part
 * either and bit k of skipped[ray] is set (a ray the march dropped holds zeros and a validity byte of 0: it is not
 * screened and sets no bit).
 *
 * The scene is the sum of the media of the avatars that take part. Their M = (avatars taking part) Nf breakpoints are
 * ordered by the key (D, avatar index, sample index): t_0 <= ... <= t_{M-1}. On segment [t_j, t_{j+1}) the active interval
 * of avatar k is (the number of its breakpoints at positions <= j) - 1; it has none when that is -1 or Nf - 1. With
 * s_k, c_k the density and colour of avatar k's active interval (0 without one), per segment j < M - 1
 *   sigma_j = sum_k s_k (k ascending)       tau_j = (sigma_j (t_{j+1} - t_j)) render_scale
 *   T_j = exp(-sum_{i<j} tau_i)             w_j = T_j (-expm1(-tau_j)),          and w_{M-1} = 0;
 * per ray
 *   colour = sum_j w_j ((sum_k s_k c_k) / sigma_j)   (segments with sigma_j = 0 add nothing)
 *   mask = sum_j w_j        disparity = sum_j w_j / t_j        instance_mass[k] = sum_j w_j (s_k / sigma_j)
 *   instance = the k of the largest instance_mass (the lowest k among equals, compared in fp64) where mask, rounded to
 *   fp32, is >= threshold and some avatar takes part, else -1.
 * A ray on which no avatar takes part gets colour 0, mask 0, disparity 0, instance_mass 0 and instance -1.
 *
 * All arithmetic is fp64 from the stored fp32 (render_scale and threshold are fp32 too), each operation rounded on its
 * own (no FMA contraction), every sum in a fixed order, each result rounded to fp32 once when stored: two runs give
 * identical bits.
 *
 * Outputs, each optional (NULL = not wanted, nothing is written for it), at least one required: color (F, 3, n), mask and
 * disparity (F, n), instance_mass (F, K, n) fp32; instance and skipped (F, n) int32; and the merged samples, (F, n, K Nf):
 * t fp32, the ordered breakpoints, +inf from M on; source int32, k Nf + i of the breakpoint at each position, -1 from M
 * on; weight fp32, w_j, 0 from M on.
 *
 * Limits: 1 <= K <= 8, 2 <= Nf <= 128, K Nf <= 512 (ENARF_ERR_UNSUPPORTED otherwise); F >= 0, n >= 0, F n < 2^31. F n = 0
 * launches nothing.
 */
#ifndef ENARF_SCENE_H
#define ENARF_SCENE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_SCENE_ABI_VERSION 1

#define ENARF_SCENE_MAX_AVATARS  8      /* K */
#define ENARF_SCENE_MAX_SAMPLES  128    /* Nf */
#define ENARF_SCENE_MAX_MERGED   512    /* K Nf */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_scene_composite_args {
    int32_t F, K, n, Nf;
    float render_scale, threshold;
    const float *depth, *density, *color;
    const uint8_t *valid;                                 /* optional */
    float *out_color, *out_mask, *out_disparity;          /* optional, as every output */
    float *out_instance_mass;
    int32_t *out_instance, *out_skipped;
    float *out_t;
    int32_t *out_source;
    float *out_weight;
} enarf_scene_composite_args;

int enarf_scene_abi_version(void);
const char *enarf_scene_last_error(void);

/* the K sample lists of every ray of F frames to one image per frame, one launch on `stream` */
int enarf_scene_composite(const enarf_scene_composite_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_SCENE_H */
