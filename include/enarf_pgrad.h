/*
 * enarf_pgrad.h - C ABI of libenarf_pgrad.so: the gradient of the articulated query with respect to its articulation, on
 * the MI355X (gfx950). One call: the backward of enarf_query_fwd (mode f32) with respect to the sample points and the part
 * records, the two inputs enarf_query_bwd leaves out. A library of its own next to libenarf_hip.so; same conventions as
 * enarf_skin.h: raw device pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed as void*, NULL =
 * the null stream) with no host synchronisation and no allocation, 0 on success, a negative ENARF_ERR_* for an argument
 * it rejects (checked on the host, no device needed) or a positive hipError_t; enarf_pgrad_last_error() gives the message
 * (thread local). No environment variable is read.
 *
 * enarf_pgrad_query. Inputs as enarf_query_fwd / enarf_query_bwd take them: points (B, 3, N); parts
 * (B, P, 16) records (R row-major in 0..8, the scaled translation t in 9..11, the canonical scale s in 12);
 * canonical_pose (P, 4, 4) row-major; mask_planes points at the part-probability planes where they lie in the NCHW
 * tri-plane (plane p of part k is channel 3 k + p from there), feat_cl at the channel-last feature planes
 * [b][plane][y][x][32], each with its batch stride in floats (0 = one tri-plane shared by every image); mlp_pack the
 * per-image pack enarf_prepare writes (its fp32 section is read); g_density (B, N) and g_color (B, 3, N), the upstream
 * gradients, either of which may be NULL (= zero).
 *
 * The function differentiated is what the reference's autograd returns for its query (oracle/enarf_oracle.py `query`), not
 * the derivative where the two differ: the density's activation passes a negative gradient through its negative region
 * with slope 0.1; under clamp_mask the part-probability sample is clamped in value and its gradient goes straight
 * through; the bilinear taps' floor and the cube tests are constants. One lane per point:
 *   - the membership walk of the query (csrc/enarf_parts.h), so validity is the query's bit for bit; the weighted feature
 *     sum over the valid parts in ascending order, w_k = (s0 s1) s2 of the three plane sigmoids, 1 / P under
 *     uniform_part_weight;
 *   - the three layers 32 -> 64 -> 64 -> 4 forward and backward in fp32 FMAs on the image's demodulated weights;
 *     under multiply_density_with_weight the density carries the factor max w over ALL parts (an invalid part weighs
 *     0.125), whose gradient goes to the first valid part that attains it, or nowhere when 0.125 wins;
 *   - a second walk over the valid parts: with d = p - t, l = R^T d, q = s l, c = Rc q + tc and G_c the gradient at the
 *     canonical point (feature planes and, unless uniform_part_weight, the part-probability planes: dw_k / dm_p =
 *     w_k (1 - s_p); d ix / d x = W / 2, zeros padding):
 *         dq = Rc^T G_c,  dl = s dq,  g_s += l . dq,  dd = R dl,  g_p += dd,  g_t -= dd,  g_R[j][i] += d_j dl_i.
 * Outputs:
 *   g_points (B, 3, N) fp32   every entry written exactly once; a point in no cube gets zeros
 *   g_parts  (B, P, 16) fp32  the gradient of every record entry, laid out as the record; slots 13..15 are zero
 * Each workgroup of 256 lanes writes the sums of its points' record gradients (fp64) to `workspace`
 * (enarf_pgrad_workspace_bytes(B, P, N) bytes, 256-byte aligned, contents need not be initialised); a second kernel adds the
 * workgroups' sums in a fixed order in fp64 and rounds once. No atomics anywhere: two runs on the same inputs give
 * identical bits in both outputs.
 * 1 <= P <= 32, H, W >= 2, 3 P H W floats < 2^30 and 96 H W floats < 2^31; 1 <= B <= 65535 and N / 256 + 1 < 2^31, else
 * ENARF_ERR_UNSUPPORTED. N = 0 launches no kernel and fills g_parts with zeros.
 */
#ifndef ENARF_PGRAD_H
#define ENARF_PGRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_PGRAD_ABI_VERSION 1

#define ENARF_PGRAD_MAX_PARTS   32    /* one bit of the validity mask per part */
#define ENARF_PGRAD_BLOCK       256   /* points a workgroup takes: one partial sum of the record gradients each */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_pgrad_query_args {
    int32_t B, P, H, W;
    int64_t N;
    int32_t clamp_mask, uniform_part_weight, multiply_density_with_weight, reserved;
    const float *points, *parts, *canonical_pose;
    const float *feat_cl;
    int64_t feat_batch_stride;
    const float *mask_planes;
    int64_t mask_batch_stride;
    const void *mlp_pack;
    const float *g_density, *g_color;           /* optional, NULL = zero */
    float *g_points, *g_parts;
    void *workspace;
} enarf_pgrad_query_args;

int enarf_pgrad_abi_version(void);
const char *enarf_pgrad_last_error(void);

/* bytes of workspace enarf_pgrad_query needs for these sizes (0 for sizes it rejects or N = 0) */
size_t enarf_pgrad_workspace_bytes(int32_t B, int32_t P, int64_t N);

/* g_points and g_parts, two launches on `stream` */
int enarf_pgrad_query(const enarf_pgrad_query_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_PGRAD_H */
