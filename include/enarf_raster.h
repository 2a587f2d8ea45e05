/*
 * enarf_raster.h - C ABI of libenarf_raster.so: hard-Phong rasterisation of one device-resident triangle mesh on the
 * MI355X (gfx950), the image half of the reference's render_mesh_ (libraries/NARF/mesh_rendering.py:17-47, a pytorch3d
 * MeshRenderer with a HardPhongShader). A library of its own, next to libenarf_hip.so and libenarf_mesh.so; same
 * conventions as enarf_mesh.h: raw device pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed
 * as void*, NULL = the null stream) with no host synchronisation, 0 on success, a negative ENARF_ERR_* for an argument
 * it rejects (checked on the host, no device needed) or a positive hipError_t; enarf_raster_last_error() gives the
 * message (thread local).
 *
 * Contract. Inputs: vertices (V, 3) fp32 in camera space, triangles (T, 3) int64, K (3, 3) fp32
 * row-major on the device (only fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2] are read), img_size = the width
 * and height of the image K describes, R = the output resolution; 0 <= V, T < 2^31 and 1 <= R <= 4096.
 *   pixel <-> ray   output pixel (r, c) is the point ((c + 1/2) s, (r + 1/2) s) of K's image, s = img_size / R; a vertex
 *                   projects to (fx x / z + cx, fy y / z + cy). Row 0 is the top of K's image (small v): the reference's
 *                   flip of both axes cancels pytorch3d's +X-left / +Y-up screen.
 *   coverage        a triangle covers a pixel when its three 2-D barycentrics at the pixel centre are all > 0 (either
 *                   winding, no culling). A triangle is not drawn when a vertex has z <= 0 (or is not finite), an index
 *                   lies outside [0, V), or its screen area is 0.
 *   depth           b'_i = (b_i / z_i) / S, S = sum_j b_j / z_j (perspective-correct); zbuf = 1 / S. A pixel takes the
 *                   covering triangle with the smallest fp32 zbuf, on a tie the smallest triangle id.
 *   normals         n_f = (v1 - v0) x (v2 - v0); a vertex normal is the sum of n_f over the faces (all faces with valid
 *                   indices, drawn or not) that use the vertex, in increasing face id, divided by max(|.|, 1e-6); the
 *                   pixel normal N is sum_i b'_i n_{v_i} divided by max(|.|, 1e-6).
 *   shading         p = sum_i b'_i v_i, L = -p / max(|p|, 1e-6) (light and camera at the origin), c = N . L:
 *                   colour = 0.5 + 0.3 max(c, 0) + 0.2 (c > 0 ? max(2c^2 - 1, 0)^64 : 0) on all three channels,
 *                   1 on the background; image = floor(255 colour).
 * Geometry and shading are evaluated in fp64 from the fp32 inputs, and rounded to fp32 at the outputs.
 *
 * Outputs, in the final orientation, bit-identical from run to run: image (R, R, 3) uint8 (required); pix_to_face
 * (R, R) int64, -1 on the background; zbuf (R, R) fp32, -1 on the background; bary (R, R, 3) fp32 = b', -1 on the
 * background; normals (R, R, 3) fp32 = N, 0 on the background. A null optional output is not written.
 */
#ifndef ENARF_RASTER_H
#define ENARF_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_RASTER_ABI_VERSION 1

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

int enarf_raster_abi_version(void);
const char *enarf_raster_last_error(void);

/* bytes of device workspace for V vertices, T triangles at R x R (256-byte aligned base expected); 0 for sizes
 * rejected */
size_t enarf_raster_workspace_bytes(int64_t V, int64_t T, int R);

/* the whole rasterisation (project, depth, vertex normals of the visible vertices, shade) on `stream` */
int enarf_raster_mesh(const float *vertices, int64_t V, const int64_t *triangles, int64_t T, const float *K_device,
                      int img_size, int R, void *workspace, uint8_t *image, int64_t *pix_to_face, float *zbuf,
                      float *bary, float *normals, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_RASTER_H */
