/*
 * enarf_simp.h - C ABI of libenarf_simp.so: simplification of a triangle mesh on the MI355X (gfx950) by uniform-grid vertex
 * clustering (Rossignac-Borrel) with quadric placement of the new vertices (after Lindstrom). A library of its own next to
 * libenarf_mesh.so; same conventions as enarf_bake.h: raw device pointers and sizes, every call asynchronous on `stream` (a
 * hipStream_t passed as void*, NULL = the null stream) with no host synchronisation and no allocation, 0 on success, a
 * negative ENARF_ERR_* for an argument it rejects (checked on the host before any launch, no device needed) or a positive
 * hipError_t; enarf_simp_last_error() gives the message (thread local). No atomics, no LDS, no workspace; every value is
 * computed in fp64 from the stored fp32 / integer inputs, each operation rounded on its own (no FMA contraction), every
 * sum runs in a fixed order, and a result is rounded once when it is stored: two runs give identical bits.
 *
 * The library holds the three kernels of the method; the sorts, the segment offsets and the compaction between them are
 * the caller's (enarf_gan_amd/_simp_lib.py does them with torch). The whole contract, for vertices (V, 3)
 * fp32, triangles (T, 3) int64, a cell size h > 0 (fp32) and an origin (3 fp32, at or below the vertices' minimum):
 *   cells      the cell of vertex v is c = floor((double(v) - double(origin)) / double(h)) per axis, 0 <= c < 2^21; its key
 *              is cx << 42 | cy << 21 | cz. A cluster is a non-empty cell; clusters are numbered 0 .. C - 1 by ascending
 *              key. lo = double(origin) + c double(h) is the cell's lower corner.
 *   validity   a triangle naming a vertex outside [0, V) is ignored everywhere.
 *   mean       m = (sum over the cluster's vertices, in vertex order, of double(v) - lo) / count.
 *   quadric    every valid triangle adds n n^T to A and n d to b of every DISTINCT cluster among its three corners, with
 *              p_k = double(v_k) - lo of THAT cluster, n = (p1 - p0) x (p2 - p0), d = n . p0 (planes weighed by their squared
 *              area). lambda = reg trace(A). trace(A) == 0 (no triangle of non-zero area): x = m. Otherwise x solves
 *              (A + lambda I) x = b + lambda m (symmetric positive definite, condition number <= 1 + 1 / reg; Cholesky).
 *   vertex     clamp(x, 0, h) + lo per axis, rounded to fp32. The mean placement takes x = m.
 *   triangles  each corner mapped to its cluster; a triangle with two equal corners is dropped; the others are rotated so
 *              that the smallest cluster comes first (the orientation is kept). The caller keeps one copy of each
 *              distinct triple, in lexicographic order; a triple and its reverse are two triangles.
 * Clustering does not preserve topology: thin gaps can close and edges can become non-manifold.
 *
 * enarf_simp_keys. One lane per vertex: 12 bytes in, the 64-bit key out. Each c is clamped to [0, 2^21) (the caller has
 * checked the extent; a NaN gives 0).
 *
 * enarf_simp_corners. One lane per triangle. Inputs: triangles and vertex_cluster (V) int32, values in [0, C). Outputs:
 * triples (T, 3) int32, the rotated cluster triple, or (-1, -1, -1) for a dropped or an invalid triangle; incidence (T, 3)
 * int32, slot 3 t + k: the cluster of corner k, or ENARF_SIMP_NO_CLUSTER when the triangle is invalid or an earlier corner
 * of it has the same cluster. A stable sort of the slots by that value lists, cluster by cluster, the triangles that add to
 * its quadric, in the order (triangle, corner).
 *
 * enarf_simp_place. One wavefront per cluster. Inputs: keys (C) int64 ascending (the clusters' keys); vertex_order (V)
 * int64, the vertices sorted by cluster (stable) and vertex_start (C + 1) int64, cluster i owning vertex_order[
 * vertex_start[i] .. vertex_start[i + 1]); for the quadric placement slot_order (3 T) int64, the incidence slots sorted by
 * their value (stable), and slot_start (C + 1) int64 in the same way (slots past slot_start[C] are the NO_CLUSTER ones and
 * are not read). Lane l adds the segment's entries l, l + 64, l + 128, ... in that order; the 64 partial sums are then
 * folded pairwise, lane l += lane l + 32, then + 16, 8, 4, 2, 1; lane 0 solves, clamps and stores. Output: out (C, 3) fp32.
 * Entries of the orders and starts outside their ranges are skipped, nothing is read through an index out of range.
 * 0 <= V < 2^31, 0 <= 3 T < 2^31, 0 <= C <= V; C = 0 launches nothing.
 */
#ifndef ENARF_SIMP_H
#define ENARF_SIMP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_SIMP_ABI_VERSION 1

#define ENARF_SIMP_AXIS_BITS   21             /* cells an axis: < 2^21 */
#define ENARF_SIMP_NO_CLUSTER  0x7FFFFFFF     /* incidence slot that adds to no cluster */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_simp_keys_args {
    int64_t V;
    float origin[3], cell;
    const float *vertices;
    int64_t *keys;                              /* (V) */
} enarf_simp_keys_args;

typedef struct enarf_simp_corners_args {
    int64_t V, T;
    int32_t C, reserved;
    const int64_t *triangles;
    const int32_t *vertex_cluster;              /* (V) */
    int32_t *triples;                           /* (T, 3) */
    int32_t *incidence;                         /* (T, 3) */
} enarf_simp_corners_args;

typedef struct enarf_simp_place_args {
    int64_t V, T;
    int32_t C, quadric;                         /* quadric: 0 = the mean placement */
    float origin[3], cell;
    double reg;
    const float *vertices;
    const int64_t *triangles;                   /* quadric only */
    const int64_t *keys;                        /* (C) */
    const int64_t *vertex_order, *vertex_start; /* (V), (C + 1) */
    const int64_t *slot_order, *slot_start;     /* (3 T), (C + 1); quadric only */
    float *out;                                 /* (C, 3) */
} enarf_simp_place_args;

int enarf_simp_abi_version(void);
const char *enarf_simp_last_error(void);

/* the cell key of every vertex, one launch on `stream` */
int enarf_simp_keys(const enarf_simp_keys_args *args, void *stream);

/* the cluster triple and the three incidence slots of every triangle, one launch on `stream` */
int enarf_simp_corners(const enarf_simp_corners_args *args, void *stream);

/* the new vertex of every cluster, one launch on `stream` */
int enarf_simp_place(const enarf_simp_place_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_SIMP_H */
