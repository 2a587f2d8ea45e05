/*
 * enarf_paint.h - C ABI of libenarf_paint.so: deferred shading of a rasterised mesh on the MI355X (gfx950) with a colour
 * or a part label per vertex. enarf_raster_mesh (enarf_raster.h) leaves the fragment buffers of an image - the covering
 * face, its perspective-correct barycentrics and the interpolated normal of every pixel -; this library turns them into
 * a coloured image. A library of its own next to libenarf_raster.so; same conventions as enarf_seg.h: raw device
 * pointers and sizes, the call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null stream) with no
 * host synchronisation and no allocation, 0 on success, a negative ENARF_ERR_* for an argument it rejects (checked on
 * the host before any launch, no device needed) or a positive hipError_t; enarf_paint_last_error() gives the message
 * (thread local).
 *
 * enarf_paint_shade. One lane per pixel, one launch per image, no atomics. Inputs: pix_to_face (R, R)
 * int64, bary (R, R, 3) and normals (R, R, 3) fp32 as enarf_raster_mesh wrote them, vertices (V, 3) fp32 in camera
 * space, triangles (T, 3) int64, and exactly one of
 *   colour mode  vertex_colors (V, 3) fp32 in [0, 1];
 *   label mode   vertex_labels (V) int32 with palette (P, 3) fp32 in [0, 1], P >= 1.
 * Every value is computed in fp64 from the fp32 inputs, each operation rounded on its own (no FMA contraction), and
 * rounded to fp32 once when it is stored. Per pixel, with f = pix_to_face and (i0, i1, i2) = triangles[f]:
 *   background   f outside [0, T), or any of i0, i1, i2 outside [0, V): albedo = shaded = background; nothing is read
 *                through f or the indices;
 *   texel        colour mode: (b'0 colour[i0] + b'1 colour[i1]) + b'2 colour[i2] per channel, b' = bary as stored;
 *                label mode: the corner k with the largest b'k, compared as fp32, the lowest k among equals (a NaN never
 *                wins over corner 0); l = vertex_labels[ik]; palette[l] when 0 <= l < P, else neutral;
 *   point        p = (b'0 v[i0] + b'1 v[i1]) + b'2 v[i2] per component;
 *   normal       N = normals / max(|normals|, 1e-6), |n| = sqrt((n0 n0 + n1 n1) + n2 n2);
 *   light        c = -((N0 p0 + N1 p1) + N2 p2) / max(|p|, 1e-6): the light is at the camera; a NaN counts as 0 below;
 *   shaded       lit: texel (0.5 + 0.3 max(c, 0)) + 0.2 s, s = max(2 c c - 1, 0)^64 (six squarings) when c > 0, else 0 -
 *                pytorch3d's (ambient + diffuse) texel + specular with its default material and light, the formula of
 *                enarf_raster.h when the texel is white; not lit: shaded = texel.
 * Outputs: albedo (R, R, 3) fp32 = the texel, shaded (R, R, 3) fp32, image (R, R, 3) uint8 = floor(255 clamp(shaded, 0,
 * 1)), a NaN giving 0. albedo and shaded are optional (NULL = not written); image is required.
 * 1 <= R <= 4096, 0 <= V, T < 2^31; T = 0 gives the background everywhere. Every output is a function of the inputs
 * alone: two runs give identical bits.
 */
#ifndef ENARF_PAINT_H
#define ENARF_PAINT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_PAINT_ABI_VERSION 1

#define ENARF_PAINT_MAX_SIZE   4096   /* R */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_paint_shade_args {
    int32_t R, P;                               /* P: palette entries, label mode only */
    int64_t V, T;
    int32_t lit, reserved;
    float neutral[3], background[3];
    const int64_t *pix_to_face;
    const float *bary, *normals;
    const float *vertices;
    const int64_t *triangles;
    const float *vertex_colors;                 /* colour mode, or NULL */
    const int32_t *vertex_labels;               /* label mode, or NULL */
    const float *palette;                       /* label mode */
    float *albedo, *shaded;                     /* optional */
    uint8_t *image;
} enarf_paint_shade_args;

int enarf_paint_abi_version(void);
const char *enarf_paint_last_error(void);

/* the coloured image of one set of fragment buffers, one launch on `stream` */
int enarf_paint_shade(const enarf_paint_shade_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_PAINT_H */
