/*
 * enarf_bake.h - C ABI of libenarf_bake.so: a texture atlas for an extracted mesh on the MI355X (gfx950) - the surface
 * point of every texel, the RGBA8 texture from the colours or labels found at those points, and the deferred textured
 * shading of a rasterised mesh. A library of its own next to libenarf_paint.so; same conventions as enarf_paint.h: raw
 * device pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null stream)
 * with no host synchronisation and no allocation, 0 on success, a negative ENARF_ERR_* for an argument it rejects (checked
 * on the host before any launch, no device needed) or a positive hipError_t; enarf_bake_last_error() gives the message
 * (thread local). Every kernel is one lane per element, without atomics or LDS; every value is computed in fp64 from the
 * stored fp32 / integer inputs, each operation rounded on its own (no FMA contraction), and rounded once when it is
 * stored. Every output is a function of the inputs alone: two runs give identical bits.
 *
 * The atlas is a pure function of the triangle count T and the atlas size A, 6 <= A <= 8192; no UV
 * buffer is stored anywhere.
 *   cells      triangles are packed in pairs into square cells of c texels a side, n = A / c (integer) cells a row; c is
 *              the largest integer >= 6 with 2 n n >= T, that is c = A / max(1, ceil(sqrt(T / 2))). No such c:
 *              ENARF_ERR_UNSUPPORTED (the message names the smallest A that holds T triangles).
 *   origin     triangle t lies in cell q = t / 2, half h = t & 1; the cell's origin in texels is (q % n c, q / n c): x is
 *              the column, y the row, row 0 the top row of the image (glTF's UV origin).
 *   corners    local to the cell, in continuous texel coordinates, texel (i, j) centred at (i + 1/2, j + 1/2):
 *              h = 0: corners (i0, i1, i2) at (1, 1), (c - 3, 1), (1, c - 3);
 *              h = 1: at (c - 1, c - 1), (3, c - 1), (c - 1, 3) (the half turn of h = 0: the winding is kept).
 *   ownership  texel (i, j) of a cell belongs to the lower triangle (h = 0) when i + j + 1 <= c, else to the upper one.
 *              A texel is empty when it lies outside every cell (column or row >= n c), its owner is >= T, or its owner
 *              names a vertex outside [0, V).
 * A bilinear tap (clamp to edge, no mip-maps) at any point of a triangle, edges included, reads only texels that triangle
 * owns; owned texels outside the triangle's outline take the affine continuation of its map.
 *
 * enarf_bake_points. One lane per texel of the rows [row0, row0 + rows) of the atlas. For an owned texel (x, y) of cell
 * origin (ox, oy), with i = x - ox, j = y - oy, L = c - 4 and (i0, i1, i2) = triangles[t]:
 *   h = 0: a1 = (i + 0.5 - 1) / L, a2 = (j + 0.5 - 1) / L;   h = 1: a1 = (c - 1 - (i + 0.5)) / L, a2 = (c - 1 - (j + 0.5)) / L;
 *   a0 = (1 - a1) - a2;   p = (a0 v[i0] + a1 v[i1]) + a2 v[i2] per component.
 * Outputs: points (3, rows A) fp32, three planes (the layout the query takes), (0, 0, 0) for an empty texel; texel_face
 * (rows, A) int32, the owner, -1 for an empty texel. Nothing is read through an index out of range.
 *
 * enarf_bake_resolve. One lane per texel of `count` texels. Inputs: texel_face (count) and exactly one of
 *   colour mode  colors (3, count) fp32, three planes; v = (x + 1) / 2, or v = x when `unit` is set;
 *   label mode   labels (count) int32 with palette (P, 3) fp32 in [0, 1], P >= 1: v = palette[l] when 0 <= l < P, else
 *                neutral.
 * Outputs: texture (count, 4) uint8, one 32-bit store a texel: rgb = floor(255 clamp(v, 0, 1)), a NaN giving 0, alpha
 * 255; an empty texel (texel_face < 0) takes floor(255 clamp(fill, 0, 1)) and alpha 0 and reads neither colour nor label.
 * texture_f32 (count, 3) fp32, optional: v unquantised and unclamped, `fill` for an empty texel.
 *
 * enarf_bake_shade. One lane per pixel, one launch per image. Inputs: pix_to_face (R, R) int64, bary (R, R, 3) and normals
 * (R, R, 3) fp32 as enarf_raster_mesh wrote them, vertices (V, 3) fp32, triangles (T, 3) int64 and exactly one of texture
 * (A, A, 4) uint8 (a channel is byte / 255, alpha is ignored) or texture_f32 (A, A, 3) fp32. Per pixel, with f =
 * pix_to_face and (i0, i1, i2) = triangles[f]:
 *   background   as enarf_paint.h: f outside [0, T), or any index outside [0, V): albedo = shaded = background;
 *   uv           (b'0 U0 + b'1 U1) + b'2 U2 per component, U the corners of face f in atlas texels (cell origin + the
 *                local corner: exact integers), b' = bary as stored;
 *   tap          s = u - 0.5, fx = floor(s), wx1 = s - fx, wx0 = 1 - wx1; x0 = clamp(fx, 0, A - 1), x1 = clamp(fx + 1, 0,
 *                A - 1) (a NaN clamps to 0); the same for v (fy, wy0, wy1, y0, y1);
 *                albedo = (((wx0 wy0) t[y0][x0] + (wx1 wy0) t[y0][x1]) + (wx0 wy1) t[y1][x0]) + (wx1 wy1) t[y1][x1];
 *   point, normal, light, shaded   the formulas of enarf_paint.h with the albedo as the texel.
 * Outputs as there: albedo and shaded (R, R, 3) fp32, optional; image (R, R, 3) uint8 = floor(255 clamp(shaded, 0, 1)).
 * 1 <= R <= 4096, 0 <= V, T < 2^31; T = 0 gives the background everywhere.
 */
#ifndef ENARF_BAKE_H
#define ENARF_BAKE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_BAKE_ABI_VERSION 1

#define ENARF_BAKE_MIN_CELL    6      /* c */
#define ENARF_BAKE_MIN_ATLAS   6      /* A */
#define ENARF_BAKE_MAX_ATLAS   8192
#define ENARF_BAKE_MAX_SIZE    4096   /* R */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_bake_points_args {
    int32_t A, row0, rows, reserved;
    int64_t V, T;
    const float *vertices;
    const int64_t *triangles;
    float *points;                              /* (3, rows A) */
    int32_t *texel_face;                        /* (rows, A) */
} enarf_bake_points_args;

typedef struct enarf_bake_resolve_args {
    int64_t count;
    int32_t P, unit;                            /* P: palette entries, label mode only; unit: colours already in [0, 1] */
    float neutral[3], fill[3];
    const int32_t *texel_face;
    const float *colors;                        /* colour mode, or NULL */
    const int32_t *labels;                      /* label mode, or NULL */
    const float *palette;                       /* label mode */
    uint8_t *texture;                           /* (count, 4), 4-byte aligned */
    float *texture_f32;                         /* optional */
} enarf_bake_resolve_args;

typedef struct enarf_bake_shade_args {
    int32_t R, A;
    int64_t V, T;
    int32_t lit, reserved;
    float background[3], reserved2;
    const int64_t *pix_to_face;
    const float *bary, *normals;
    const float *vertices;
    const int64_t *triangles;
    const uint8_t *texture;                     /* (A, A, 4), 4-byte aligned, or NULL */
    const float *texture_f32;                   /* (A, A, 3), or NULL */
    float *albedo, *shaded;                     /* optional */
    uint8_t *image;
} enarf_bake_shade_args;

int enarf_bake_abi_version(void);
const char *enarf_bake_last_error(void);

/* the layout of T triangles in an atlas of A texels a side: the cell size and the cells a row; no device needed */
int enarf_bake_layout(int64_t T, int32_t A, int32_t *cell, int32_t *cells_per_row);

/* surface points and owners of a band of atlas rows, one launch on `stream` */
int enarf_bake_points(const enarf_bake_points_args *args, void *stream);

/* colours or labels of `count` texels to the RGBA8 (and fp32) texture, one launch on `stream` */
int enarf_bake_resolve(const enarf_bake_resolve_args *args, void *stream);

/* the textured image of one set of fragment buffers, one launch on `stream` */
int enarf_bake_shade(const enarf_bake_shade_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_BAKE_H */
