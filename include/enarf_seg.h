/*
 * enarf_seg.h - C ABI of libenarf_seg.so: part segmentation on the MI355X (gfx950). Two calls: the owner of a sample
 * point among the P articulated parts of the radiance field (the part with the largest tri-plane part probability among
 * the parts whose cube contains the point, models/narf.py:176-240), and the composition of such labels along a ray into
 * the semantic map the reference's render() carries a flag for (libraries/NeRF/rendering.py:298-305). A library of its
 * own next to libenarf_hip.so; same conventions as enarf_anim.h: raw device pointers and sizes, every call asynchronous
 * on `stream` (a hipStream_t passed as void*, NULL = the null stream) with no host synchronisation and no allocation,
 * 0 on success, a negative ENARF_ERR_* for an argument it rejects (checked on the host, no device needed) or a positive
 * hipError_t; enarf_seg_last_error() gives the message (thread local).
 *
 * enarf_seg_labels. One lane per point; B images of M points each. The point comes from one of
 *   explicit mode  points != NULL: component c of point i of image b is
 *                  points[b * point_batch_stride + i * point_stride + c * comp_stride] (strides in floats), so (B, 3, M) is
 *                  (3 M, 1, M) and (M, 3) is (0 or 3 M, 3, 1); coordinates in the scaled camera space of enarf_prepare;
 *   ray mode       points == NULL: M = n * Nf, point i is sample i % Nf of ray i / Nf, formed exactly as the fine pass of
 *                  the march forms it: d = K^-1 [u v w] with image_coord (B, 3, n) and inv_intrinsics (B, 3, 3),
 *                  each row ((k0 u + k1 v) + k2 w); start = depth_min d, end = depth_max d; p = start (1 - t) + end t
 *                  with t = bins[b, ray, sample], every operation rounded on its own. depth_min, depth_max (B, n) and
 *                  bins (B, n, Nf) are the march's taps.
 * parts (B, P, 16) are the frames enarf_prepare writes, canonical_pose (P, 4, 4) row-major; mask_planes points at the
 * part-probability planes where they lie in the NCHW tri-plane (channel 96 of image 0: plane p of part k is channel
 * 3 k + p from there), mask_batch_stride floats from one image's planes to the next (0 = shared). For every part k in
 * ascending order: local = R^T (p - t), canonical = Rc (local s) + tc in the fixed operation order of the query and the
 * march; the pair is valid iff every |local| <= 1 and every |canonical| < 1. The weight of a valid pair is
 * (s0 s1) s2, s_p = sigmoid(bilinear sample of plane p at (xy, yz, zx), zeros padding, align_corners false), the sample
 * clamped to [-2, 5] first under clamp_mask; under uniform_part_weight every valid pair weighs 1 / P. Outputs, (B, M):
 *   label      int32   the valid part of the largest weight, the lowest index among equals; -1 when no part is valid
 *   top        fp32    that weight; 0 when label is -1
 *   second     fp32    the largest weight among the other valid parts; -1 when there is none
 *   valid_bits uint32  optional (NULL = not written): bit k set iff part k is valid
 * 1 <= P <= 32 (the bit mask), H, W >= 2, 3 P H W floats < 2^30, 0 <= M, M / 256 + 1 < 2^31, 1 <= B <= 65535. M = 0 or
 * B = 0 launches nothing.
 *
 * enarf_seg_composite. labels (B, n, Nf) int32, fine_weights (B, n, Nf - 1) fp32 (the march's compositing weights),
 * palette (P, 3) fp32. One wavefront per ray, lanes as samples (2 <= Nf <= 128: a lane takes at most two). Only the first
 * Nf - 1 samples carry weight: the last closes the last interval. A label outside [0, P) counts as -1.
 *   color     (B, 3, n) fp32   sum over i < Nf - 1 with label_i >= 0 of w_i palette[label_i]
 *   part_mass (B, n)    fp32   max over k of m_k, m_k = sum of w_i over the samples with label_i = k; 0 when part_map is -1
 *   part_map  (B, n)    int32  the k of that maximum, the lowest among equals; -1 when no part has a positive mass (no
 *                              labelled sample of the ray has w > 0)
 * The distinct labels of a ray are peeled one at a time with a ballot and each sum is the fixed-order reduction of the
 * wave, so every output is a function of the inputs alone: two runs give identical bits. 0 <= B n < 2^31 - 4.
 */
#ifndef ENARF_SEG_H
#define ENARF_SEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_SEG_ABI_VERSION 1

#define ENARF_SEG_MAX_PARTS    32     /* one bit of valid_bits per part */
#define ENARF_SEG_MAX_SAMPLES  128    /* one wavefront per ray, two samples a lane */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_seg_label_args {
    int32_t B, P, H, W;
    int64_t M;                                  /* points per image; n * Nf in ray mode */
    int32_t clamp_mask, uniform_part_weight;
    const float *points;                        /* explicit mode, or NULL */
    int64_t point_batch_stride, point_stride, comp_stride;
    const float *image_coord, *inv_intrinsics, *depth_min, *depth_max, *bins;    /* ray mode */
    int32_t n, Nf;
    const float *parts, *canonical_pose, *mask_planes;
    int64_t mask_batch_stride;
    int32_t *label;
    float *top, *second;
    uint32_t *valid_bits;                       /* optional */
} enarf_seg_label_args;

typedef struct enarf_seg_composite_args {
    int32_t B, n, Nf, P;
    const int32_t *labels;
    const float *fine_weights, *palette;
    float *color, *part_mass;
    int32_t *part_map;
} enarf_seg_composite_args;

int enarf_seg_abi_version(void);
const char *enarf_seg_last_error(void);

/* the owner of every point, one launch on `stream` */
int enarf_seg_labels(const enarf_seg_label_args *args, void *stream);

/* labels along each ray to the semantic colour, the dominant part and its mass, one launch on `stream` */
int enarf_seg_composite(const enarf_seg_composite_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_SEG_H */
