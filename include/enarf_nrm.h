/*
 * enarf_nrm.h - C ABI of libenarf_nrm.so: surface normals from the field itself, on the MI355X (gfx950). The density of
 * the articulated query has an exact spatial gradient; enarf_nrm_field_gradient returns the density and that gradient at
 * sample points in one launch, enarf_nrm_ray_normals composites the gradients of a march's fine samples into one normal
 * per ray, with validity, a fallback and an 8-bit shade. A library of its own next to libenarf_hip.so; same conventions
 * as enarf_pgrad.h and enarf_geom.h: raw device pointers and sizes, every call asynchronous on `stream` (a hipStream_t
 * passed as void*, NULL = the null stream) with no host synchronisation, no allocation and no environment variable read,
 * 0 on success, a negative ENARF_ERR_* for an argument it rejects (checked on the host before any launch, no device
 * needed) or a positive hipError_t; enarf_nrm_last_error() gives the message (thread local).
 *
 * enarf_nrm_field_gradient. Inputs as enarf_pgrad_query takes them, without upstream gradients: points
 * (B, 3, N) in the scaled camera space; parts (B, P, 16) records; canonical_pose (P, 4, 4); mask_planes at the
 * part-probability planes inside the NCHW tri-plane and feat_cl at the channel-last feature planes, each with its batch
 * stride in floats (0 = shared); mlp_pack the per-image pack of enarf_prepare (its fp32 section is read). Outputs:
 *   density  (B, N) fp32     the density of enarf_query_fwd in mode f32 (same walk, same fp32 MLP, to rounding);
 *   gradient (B, 3, N) fp32  d density / d point in the space the points are given in.
 * The gradient is what the reference's autograd returns for sum(density), i.e. g_points of enarf_pgrad_query with
 * g_density = 1 and g_color = NULL: the plain derivative of the density head where it is on (its activation >= 0), zero
 * where it is off; validity bits and bilinear cells are constants; under clamp_mask the clamped part-probability sample
 * passes its gradient straight through; under multiply_density_with_weight the factor max w carries its gradient to the
 * first valid part that attains it (nowhere when an invalid part's 0.125 wins). A point in no cube gets density 0 and an
 * exact zero gradient. One lane per point, a workgroup per 256 points of one image, one launch, no workspace, no atomics,
 * no fp64: walk 1 (csrc/enarf_parts.h) gives validity, the weighted feature and the arg-max weight; the layers 32 -> 64
 * -> 64 run forward in fp32 FMAs on dense weights in LDS and only the density row of the last layer is formed; the
 * backward runs from that one output; walk 2 chains each valid part's gradient at the canonical point through Rc, the
 * scale and R to the point. Every output is a function of the inputs alone: two runs give identical bits.
 * 1 <= P <= 32, H, W >= 2, 3 P H W floats < 2^30 and 96 H W floats < 2^31; 1 <= B <= 65535 and N / 256 + 1 < 2^31, else
 * ENARF_ERR_UNSUPPORTED. N = 0 launches nothing.
 *
 * enarf_nrm_ray_normals. One lane per ray, one launch per batch, no atomics. Every value is computed in fp64 from the
 * stored fp32, each operation rounded on its own (no FMA contraction), sums in the written order, rounded to fp32 once
 * when stored; only +, -, *, / and sqrt are used. Inputs: gradient (B, 3, n Nf) fp32, ray-major and sample-minor as the
 * march's fine points; weights (B, n, Nf - 1) fp32, the march's fine weights (weight i belongs to sample i); mask (B, n)
 * fp32; optionally fallback (B, n, 3) fp32 with flags_in (B, n) uint8 as enarf_geom_buffers returns its normals and
 * flags; optionally points (B, n, 3) fp32 (required by the lit shade). Per ray:
 *   G       G_c = sum_{i = 0}^{Nf - 2} w_i g_c[i] in ascending i, m = sqrt((G0 G0 + G1 G1) + G2 G2);
 *   field   the ray has a field normal when mask >= mask_threshold (compared as fp32) and min_gradient < m < inf; then
 *           N = -G / m (the density grows into the body, so the normal points out of it; no flip);
 *   else    N = fallback where bit 1 (ENARF_NRM_FLAG_NORMAL) of flags_in is set, else zeros;
 *   flags   flags_in (0 without one) with bit 2 (ENARF_NRM_FLAG_FIELD) cleared, then set on a field normal;
 *   shade 0 normal: rgb = 0.5 + 0.5 (N0, -N1, -N2);   shade 1 lit: grey = (0.5 + 0.3 max(c, 0)) + 0.2 s with
 *           c = -((N0 p0 + N1 p1) + N2 p2) / max(|p|, 1e-6) and s = max(2 c c - 1, 0)^64 when c > 0, else 0 - the formulas
 *           and constants of enarf_geom.h; a ray without a normal (neither field nor fallback) takes `background`.
 * Outputs: normals (B, n, 3) fp32; flags (B, n) uint8; optionally magnitude (B, n) fp32 = m and image (B, n, 3) uint8 =
 * floor(255 clamp(v, 0, 1)), a NaN giving 0. 2 <= Nf <= 128, 1 <= B <= 65535 (else ENARF_ERR_UNSUPPORTED), n >= 0 with
 * n Nf < 2^31; n = 0 launches nothing. Two runs give identical bits.
 */
#ifndef ENARF_NRM_H
#define ENARF_NRM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_NRM_ABI_VERSION 1

#define ENARF_NRM_MAX_PARTS     32    /* one bit of the validity mask per part */
#define ENARF_NRM_BLOCK         256   /* points (rays) a workgroup takes */
#define ENARF_NRM_MAX_SAMPLES   128   /* Nf */
#define ENARF_NRM_SHADE_NONE    (-1)  /* no image */
#define ENARF_NRM_SHADE_NORMAL  0
#define ENARF_NRM_SHADE_LIT     1
#define ENARF_NRM_FLAG_VALID    1     /* as ENARF_GEOM_FLAG_VALID */
#define ENARF_NRM_FLAG_NORMAL   2     /* as ENARF_GEOM_FLAG_NORMAL: the fallback normal is usable */
#define ENARF_NRM_FLAG_FIELD    4     /* the normal written is the field's */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_nrm_gradient_args {
    int32_t B, P, H, W;
    int64_t N;
    int32_t clamp_mask, uniform_part_weight, multiply_density_with_weight, reserved;
    const float *points, *parts, *canonical_pose;
    const float *feat_cl;
    int64_t feat_batch_stride;
    const float *mask_planes;
    int64_t mask_batch_stride;
    const void *mlp_pack;
    float *density, *gradient;
} enarf_nrm_gradient_args;

typedef struct enarf_nrm_ray_args {
    int32_t B, Nf;
    int64_t n;
    int32_t shade, reserved;
    float mask_threshold, min_gradient;
    float background[3];
    int32_t reserved2;
    const float *gradient, *weights, *mask;
    const float *fallback;                      /* optional, with flags_in */
    const uint8_t *flags_in;                    /* optional */
    const float *points;                        /* optional; required by ENARF_NRM_SHADE_LIT */
    float *normals;
    uint8_t *flags;
    float *magnitude;                           /* optional */
    uint8_t *image;                             /* optional; required unless shade is ENARF_NRM_SHADE_NONE */
} enarf_nrm_ray_args;

int enarf_nrm_abi_version(void);
const char *enarf_nrm_last_error(void);

/* density and its spatial gradient at the points, one launch on `stream` */
int enarf_nrm_field_gradient(const enarf_nrm_gradient_args *args, void *stream);

/* the composited normal of every ray with flags, magnitude and shade, one launch on `stream` */
int enarf_nrm_ray_normals(const enarf_nrm_ray_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_NRM_H */
