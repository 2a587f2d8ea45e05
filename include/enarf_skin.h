/*
 * enarf_skin.h - C ABI of libenarf_skin.so: rigged meshes on the MI355X (gfx950). Two calls: the skin weights of mesh
 * vertices (which of the P articulated parts of the radiance field own a vertex, and how much: the normalised tri-plane
 * part probabilities of the parts whose cube contains it), computed once for a mesh extracted in a rest pose, and
 * linear-blend posing of that mesh in F target poses in one launch. A library of its own next to libenarf_hip.so; same
 * conventions as enarf_seg.h: raw device pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed
 * as void*, NULL = the null stream) with no host synchronisation and no allocation, 0 on success, a negative
 * ENARF_ERR_* for an argument it rejects (checked on the host, no device needed) or a positive hipError_t;
 * enarf_skin_last_error() gives the message (thread local). No environment variable is read.
 *
 * enarf_skin_weights. One lane per vertex, one identity. Component c of vertex i is
 * vertices[i * vert_stride + c * comp_stride] (strides in floats), so (V, 3) is (3, 1) and (3, V) is (1, V); vertices are
 * in camera units and are multiplied by coordinate_scale (one fp32 product a component) on the way in. parts (P, 16) are
 * the rest pose's frames as enarf_prepare writes them, canonical_pose (P, 4, 4) row-major; mask_planes points at the
 * part-probability planes where they lie in the NCHW tri-plane (plane p of part k is channel 3 k + p from there).
 * For every part k in ascending order: local = R^T (p - t), canonical = Rc (local s) + tc in the fixed operation order of
 * the query and the march; the pair is valid iff every |local| <= 1 and every |canonical| < 1. The raw weight of a valid
 * pair is enarf_seg_labels': (s0 s1) s2, s_p = sigmoid(bilinear sample of plane p at (xy, yz, zx)), the sample clamped
 * to [-2, 5] first under clamp_mask; under uniform_part_weight every valid pair weighs 1 / P. The K = max_influences
 * (4 or 8) largest raw weights are kept, by descending weight; a weight must be strictly larger to move ahead, so among
 * equals the lower part index comes first. Outputs:
 *   joints     (V, K) int32   the kept parts by descending weight; unused slots hold -1
 *   weights    (V, K) fp32    the kept raw weights over their sum (sum and division in fp64, slot order); unused slots 0
 *   kept_mass  (V)    fp32    the sum of the kept raw weights over the sum of all valid raw weights (fp64, the latter in
 *                             ascending part order); exactly 1 when at most K parts are valid
 *   valid_bits (V)    uint32  optional (NULL = not written): bit k set iff part k is valid
 * Where every kept raw weight is 0 (the sigmoids underflowed) the kept slots share the vertex equally and kept_mass is 1.
 * A vertex no part contains (valid_bits == 0) follows the part with the smallest max(|local_x|, |local_y|, |local_z|),
 * the lowest index on a tie: joints[i, 0] is that part, weights[i, 0] = 1, kept_mass[i] = 0.
 * 1 <= P <= 32, H, W >= 2, 3 P H W floats < 2^30, 0 <= V, V / 256 + 1 < 2^31; joints and weights 16-byte aligned.
 * V = 0 launches nothing.
 *
 * enarf_skin_pose. vertices as above (camera units, not scaled), joints and weights (V, K) as enarf_skin_weights writes
 * them, parts_rest (P, 16) and parts (F, P, 16) records whose translations are in the scaled space (divided by
 * coordinate_scale here). The transform of part k from the rest pose A to frame B, in fp64 from the stored fp32:
 *   rho_k = s_k^A / s_k^B     (record entry 12: the bone-length ratio B over A)
 *   L_k   = rho_k (R_k^B R_k^A^T),  entry (r, c) = rho_k ((RB[r][0] RA[c][0] + RB[r][1] RA[c][1]) + RB[r][2] RA[c][2])
 *   M_k v = L_k v + (t_k^B - L_k t_k^A),  t = record translation / coordinate_scale
 * out[f * out_frame_stride + 3 i + c] = sum over the slots j with joints[i, j] >= 0, in slot order, of
 * w_j (M_{joints[i, j]} v)_c, accumulated in fp64 and rounded once to fp32; a joint outside [0, P) counts as -1. A
 * workgroup of 256 lanes takes 256 vertices and up to ENARF_SKIN_FRAMES_PER_GROUP frames, whose transforms it stages
 * in LDS; no atomics, so two runs give identical bits. 1 <= P <= 32, 0 <= F <= 65535 * ENARF_SKIN_FRAMES_PER_GROUP,
 * out_frame_stride >= 3 V floats. V = 0 or F = 0 launches nothing.
 */
#ifndef ENARF_SKIN_H
#define ENARF_SKIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_SKIN_ABI_VERSION 1

#define ENARF_SKIN_MAX_PARTS         32    /* one bit of valid_bits per part */
#define ENARF_SKIN_FRAMES_PER_GROUP  8     /* frames a workgroup of enarf_skin_pose stages in LDS */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_skin_weights_args {
    int32_t P, H, W, max_influences;            /* max_influences: 4 or 8 */
    int64_t V;
    int32_t clamp_mask, uniform_part_weight;
    float coordinate_scale;
    const float *vertices;
    int64_t vert_stride, comp_stride;
    const float *parts, *canonical_pose, *mask_planes;
    int32_t *joints;
    float *weights, *kept_mass;
    uint32_t *valid_bits;                       /* optional */
} enarf_skin_weights_args;

typedef struct enarf_skin_pose_args {
    int32_t P, F, max_influences;
    float coordinate_scale;
    int64_t V;
    const float *vertices;
    int64_t vert_stride, comp_stride;
    const int32_t *joints;
    const float *weights, *parts_rest, *parts;
    float *out;
    int64_t out_frame_stride;                   /* floats from one frame of out to the next */
} enarf_skin_pose_args;

int enarf_skin_abi_version(void);
const char *enarf_skin_last_error(void);

/* joints, weights and kept mass of every vertex, one launch on `stream` */
int enarf_skin_weights(const enarf_skin_weights_args *args, void *stream);

/* the mesh in F poses, one launch on `stream` */
int enarf_skin_pose(const enarf_skin_pose_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_SKIN_H */
