/*
 * enarf_sgrad.h - C ABI of libenarf_sgrad.so: the gradient of the multi-avatar composite (enarf_scene.h) with respect to
 * the K avatars' densities and colours, on the MI355X (gfx950). A library of its own; same conventions as enarf_scene.h:
 * raw device pointers and sizes, the call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null stream)
 * with no host synchronisation, no allocation and no environment variable read, 0 on success, a negative ENARF_ERR_*
 * for an argument it rejects (checked on the host before any launch, no device needed) or a positive hipError_t;
 * enarf_sgrad_last_error() gives the message (thread local).
 *
 * enarf_sgrad_composite_bwd. One wavefront per (frame, ray), one launch for all F frames, no atomics.
 * Inputs, fp32, exactly as enarf_scene_composite takes them: depth d and density s (F, K, n, Nf), colour c
 * (F, K, 3, n, Nf), valid (F, K, n) uint8 or NULL (= every byte 1), render_scale; and the upstream gradients of the
 * forward's ray outputs, fp32, each optional (NULL = zeros), at least one required: g_color g_C (F, 3, n), g_mask g_M and
 * g_disparity g_D (F, n), g_instance_mass g_I (F, K, n). The loss they stand for is
 *   L = g_C . colour + g_M mask + g_D disparity + sum_k g_I[k] instance_mass[k].
 *
 * Which avatars take part on a ray (validity byte, screening), the running maximum D of an avatar's depths, the merged
 * breakpoints t_0 <= ... <= t_{M-1} in the order of the key (D, avatar index, sample index) and the active interval of
 * avatar k on segment [t_j, t_{j+1}) are enarf_scene.h's. With s_k, c_k the density and colour of avatar k's active
 * interval on segment j (0 without one), per segment j < M - 1
 *   a_j = (t_{j+1} - t_j) render_scale
 *   sigma_j = sum_k s_k (k ascending)    tau_j = (sigma_j (t_{j+1} - t_j)) render_scale    T_j = exp(-sum_{i<j} tau_i)
 *   u_j = T_j (-expm1(-tau_j)) / sigma_j   (= w_j / sigma_j; where sigma_j = 0 its limit T_j a_j)
 *   h_j = g_M + g_D / t_j
 *   r_j = g_C . (sum_k s_k c_k) + sigma_j h_j + sum_k g_I[k] s_k        (so that L = sum_j u_j r_j)
 *   S_j = sum_{i>j} u_i r_i
 *   v_j = r_j / sigma_j
 *   E_j = a_j (T_j exp(-tau_j) v_j - S_j) - u_j v_j   where sigma_j > 0,      E_j = -a_j S_j   where sigma_j = 0.
 * For sample i < Nf - 1 of an avatar k that takes part, R(k, i) is the contiguous run of segments on which interval i is
 * k's active one: from the position of breakpoint (k, i) up to, but excluding, that of (k, i + 1); it may be empty.
 *   g_density[k, i]          = sum_{j in R} (E_j + u_j h_j) + (g_C . c_{k,i} + g_I[k]) sum_{j in R} u_j
 *   g_sample_color[k, ch, i] = g_C[ch] s_{k,i} sum_{j in R} u_j
 * At a sample whose density is exactly 0 this is the derivative from inside s >= 0 (the integrand u_j sum_k s_k c_k is
 * smooth there), so segments with sigma_j = 0 are not skipped as the forward skips them. Depths are constants: there is
 * no depth gradient.
 *
 * Outputs, each optional (NULL = not wanted, nothing is written for it), at least one required: g_density (F, K, n, Nf)
 * and g_sample_color (F, K, 3, n, Nf) fp32. Every entry of a wanted output is written (the caller may pass uninitialised
 * memory); exact zeros go to an avatar's last sample (it only closes an interval), to an avatar that takes no part on
 * the ray (validity byte 0, or screened out) and to a ray on which nobody takes part.
 *
 * All arithmetic is fp64 from the stored fp32 (render_scale is fp32 too), each operation rounded on its own (no FMA
 * contraction), every sum in a fixed order (a run R is summed directly, in ascending j, not as a difference of prefix
 * sums), each result rounded to fp32 once when stored: two runs give identical bits.
 *
 * Limits: 1 <= K <= 8, 2 <= Nf <= 128, K Nf <= 512 (ENARF_ERR_UNSUPPORTED otherwise); F >= 0, n >= 0, F n < 2^31. F n = 0
 * launches nothing.
 */
#ifndef ENARF_SGRAD_H
#define ENARF_SGRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_SGRAD_ABI_VERSION 1

#define ENARF_SGRAD_MAX_AVATARS  8      /* K */
#define ENARF_SGRAD_MAX_SAMPLES  128    /* Nf */
#define ENARF_SGRAD_MAX_MERGED   512    /* K Nf */

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

typedef struct enarf_sgrad_composite_bwd_args {
    int32_t F, K, n, Nf;
    float render_scale;
    const float *depth, *density, *color;
    const uint8_t *valid;                                             /* optional */
    const float *g_color, *g_mask, *g_disparity, *g_instance_mass;    /* each optional, at least one */
    float *g_density, *g_sample_color;                                /* each optional, at least one */
} enarf_sgrad_composite_bwd_args;

int enarf_sgrad_abi_version(void);
const char *enarf_sgrad_last_error(void);

/* the gradients of every ray of F frames back onto the K avatars' own samples, one launch on `stream` */
int enarf_sgrad_composite_bwd(const enarf_sgrad_composite_bwd_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_SGRAD_H */
