/*
 * enarf_nmap.h - C ABI of libenarf_nmap.so: tangent-space normal maps in the texture atlas of an extracted mesh on the
 * MI355X (gfx950) - the encoding of a vector field found at the texel points into the atlas, and the deferred shading of a
 * rasterised mesh with the map. A library of its own next to libenarf_bake.so; the conventions of enarf_bake.h: raw device
 * pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null stream) with no
 * host synchronisation and no allocation, 0 on success, a negative ENARF_ERR_* for an argument it rejects (checked on the
 * host before any launch, no device needed) or a positive hipError_t; enarf_nmap_last_error() gives the message (thread
 * local). Every kernel is one lane per element, without atomics or LDS; every value is computed in fp64 from the stored
 * fp32 / integer inputs, each operation rounded on its own (no FMA contraction), and rounded once when it is stored. Every
 * output is a function of the inputs alone: two runs give identical bits.
 *
 * The atlas is that of enarf_bake.h (cells, origin, corners, ownership: a pure function of the triangle count T and the
 * atlas size A). The tangent frame is a pure function of that layout and the vertices; no tangent buffer
 * is stored anywhere. For triangle t with corners (v0, v1, v2) = vertices[triangles[t]], per component k:
 *   e1 = v1 - v0, e2 = v2 - v0;   s = +1 for even t, -1 for odd t (the half-turned upper triangle of a cell);
 *   c  = e1 x e2: (e1[1] e2[2] - e1[2] e2[1], e1[2] e2[0] - e1[0] e2[2], e1[0] e2[1] - e1[1] e2[0]);
 *   |a| = sqrt((a0 a0 + a1 a1) + a2 a2);   n^ = c / |c| (the rasteriser's face normal);   t^ = (s e1) / |e1| (the direction
 *   of increasing u);   b^ = t^ x n^ (the direction of decreasing v, orthogonalised). This is glTF's bitangent
 *   cross(n^, t^) w with w = -1 for every triangle.
 * A triangle has no frame unless 0 < |e1| < inf and 0 < |c| < inf (a NaN fails both).
 *
 * enarf_nmap_encode. One lane per texel of `count` texels. Inputs: texel_face (count) int32 as enarf_bake_points wrote it,
 * vectors (3, count) fp32 as three planes, vertices (V, 3) fp32, triangles (T, 3) int64, negate, min_length. Per texel with
 * owner t = texel_face:
 *   empty   t < 0: the texel is (128, 128, 255, 0) and (0, 0, 1); nothing else is read;
 *   flat    t >= T, a vertex of t outside [0, V), no frame, or a length that fails the test below: (x, y, z) = (0, 0, 1);
 *   else    g = -vector when `negate` is set, else vector; m = |g|; when min_length < m < inf:
 *           x = ((g0 t^0 + g1 t^1) + g2 t^2) / m, y the same with b^, z with n^.
 * Outputs: texture (count, 4) uint8, one 32-bit store a texel: channel = floor(255 clamp((c + 1) / 2, 0, 1) + 0.5) for
 * c = x, y, z, alpha 255 (a flat texel is (128, 128, 255, 255)); texture_f32 (count, 3) fp32, optional: (x, y, z)
 * unquantised. 0 <= count <= 8192^2 (count = 0 launches nothing), 0 <= V, T < 2^31.
 *
 * enarf_nmap_shade. One lane per pixel, one launch per image. Inputs: pix_to_face, bary, normals, vertices, triangles as
 * enarf_bake_shade takes them; a normal texture, exactly one of normal_texture (A, A, 4) uint8 or normal_texture_f32
 * (A, A, 3) fp32; an albedo, at most one of texture (A, A, 4) uint8 and texture_f32 (A, A, 3) fp32 of the same A, and
 * base_color when neither is given. Per pixel, with f = pix_to_face:
 *   background   as enarf_paint.h: albedo = shaded = background, normal = the stored normal;
 *   uv, tap      those of enarf_bake.h - the same indices, clamps, weights and sum order - for both textures; a byte of
 *                the albedo is byte / 255, a byte of the normal texture decodes as (2 byte) / 255 - 1, an fp32 texel is
 *                taken as it is;
 *   q            the tapped (x, y, z), replaced by (0, 0, 1) when |q| is 0 or not finite;
 *   Ns           the frame of face f from the vertices given to this call (the posed mesh): w = (x t^ + y b^) + z n^ per
 *                component, Ns = w / |w|; a face without a frame keeps N = normals / max(|normals|, 1e-6) of enarf_paint.h
 *                and its normal output is the stored normal;
 *   point, light, shaded   the formulas of enarf_paint.h with Ns in place of N.
 * Outputs: albedo, normal and shaded (R, R, 3) fp32, optional (NULL = not written); image (R, R, 3) uint8 = floor(255
 * clamp(shaded, 0, 1)), a NaN giving 0. 1 <= R <= 4096, 6 <= A <= 8192, 0 <= V, T < 2^31; T = 0 gives the background
 * everywhere.
 */
#ifndef ENARF_NMAP_H
#define ENARF_NMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_NMAP_ABI_VERSION 1

#define ENARF_NMAP_MIN_CELL    6      /* c, as ENARF_BAKE_MIN_CELL */
#define ENARF_NMAP_MIN_ATLAS   6      /* A */
#define ENARF_NMAP_MAX_ATLAS   8192
#define ENARF_NMAP_MAX_SIZE    4096   /* R */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_nmap_encode_args {
    int64_t count, V, T;
    int32_t negate;                             /* 1: the normal is -vector (a density gradient) */
    float min_length;
    const int32_t *texel_face;                  /* (count) */
    const float *vectors;                       /* (3, count), three planes */
    const float *vertices;
    const int64_t *triangles;
    uint8_t *texture;                           /* (count, 4), 4-byte aligned */
    float *texture_f32;                         /* (count, 3), optional */
} enarf_nmap_encode_args;

typedef struct enarf_nmap_shade_args {
    int32_t R, A;
    int64_t V, T;
    int32_t lit, reserved;
    float background[3], base_color[3];
    const int64_t *pix_to_face;
    const float *bary, *normals;
    const float *vertices;
    const int64_t *triangles;
    const uint8_t *normal_texture;              /* (A, A, 4), 4-byte aligned, or NULL */
    const float *normal_texture_f32;            /* (A, A, 3), or NULL */
    const uint8_t *texture;                     /* the albedo: (A, A, 4), 4-byte aligned, or NULL */
    const float *texture_f32;                   /* (A, A, 3), or NULL */
    float *albedo, *normal, *shaded;            /* optional */
    uint8_t *image;
} enarf_nmap_shade_args;

int enarf_nmap_abi_version(void);
const char *enarf_nmap_last_error(void);

/* a vector per texel to the tangent-space RGBA8 (and fp32) normal map, one launch on `stream` */
int enarf_nmap_encode(const enarf_nmap_encode_args *args, void *stream);

/* the normal-mapped image of one set of fragment buffers, one launch on `stream` */
int enarf_nmap_shade(const enarf_nmap_shade_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_NMAP_H */
