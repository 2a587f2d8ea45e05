/*
 * enarf_guide.h - C ABI of libenarf_guide.so: the generator's own supervision term of the GAN path on the MI355X
 * (gfx950) - the mask-guidance loss `nerf_patch_loss` of the reference's models/loss.py (forward and backward). A
 * library of its own, next to libenarf_hip.so, libenarf_mesh.so, libenarf_raster.so, libenarf_pose.so and
 * libenarf_photo.so; same conventions as enarf_photo.h: raw device pointers and sizes, every call asynchronous on
 * `stream` (a hipStream_t passed as void*, NULL = the null stream) with no host synchronisation and no device-to-host
 * copy, 0 on success, a negative ENARF_ERR_* for an argument it rejects (checked on the host, no device needed) or a
 * positive hipError_t; enarf_guide_last_error() gives the message (thread local).
 *
 * Contract. fake_mask is the rendered foreground mask, fp32, (B, s, s) row-major, N = B * s * s
 * values m_i (i the flat index). bone_mask is the projected skeleton, fp32, (B, S, S) with rate = S / s >= 1 (integer
 * division) and S / rate == s. All arithmetic is fp64 and a result is rounded to fp32 once, when it is stored.
 *
 *   on-bone   pixel (b, y, x) is on the bone when the maximum of bone_mask[b, y*rate .. y*rate + rate - 1,
 *             x*rate .. x*rate + rate - 1] is > 0.5 (a max-pool of kernel and stride `rate`, no padding, the S % rate
 *             remainder rows and columns dropped; a NaN in the window makes the maximum NaN, which is not > 0.5).
 *             Pooled and thresholded inside the kernels: there is no pooled temporary. n_bone = their number.
 *   bone      = sum over on-bone pixels of (1 - m_i)^2 / n_bone                       (0 / 0 = NaN when n_bone == 0)
 *   selection with_push != 0: the k smallest values, 0 <= k <= N (the host computes k = int(N * background_ratio) and
 *             passes the integer). Values are ordered by their order-preserving integer image
 *                 key(m) = NaN ? 0xFFFFFFFF : (bits(m) ^ (sign(m) ? 0xFFFFFFFF : 0x80000000))
 *             so NaN is the largest value (as in torch.topk) and -0 orders below +0 (their squares and gradients are
 *             the same zeros). T = the k-th smallest key, found EXACTLY by a radix select (four passes over 8 key bits,
 *             integer histogram counters, no sort). Every value with key < T is selected, and of the values with
 *             key == T the Q = k - #{key < T} with the LOWEST FLAT INDEX: the selection, and with it the gradient,
 *             is a function of the input alone.
 *   push      = (sum of m_i^2 over key_i < T  +  Q * value(T)^2) / k    (0 / 0 = NaN when k == 0); 0 without with_push
 *   out[0]    = (push + bone) * coef,   out[1] = push,   out[2] = bone                 (fp32)
 *
 * Sums are reduced in a fixed order (a thread's terms in index order, a shuffle tree over the wave, the four waves left
 * to right, one fp64 partial per workgroup, the partials by strided lanes in index order and the same tree, in a
 * finishing launch). The only atomics are integer adds on the histogram counters, whose result does not depend on
 * their order; there is no float atomic. Every output is bit-identical from run to run.
 *
 * Backward, one elementwise launch, from the upstream gradient `up` of out[0] (a device scalar, read on the device):
 *   d m_i = up * coef * ( 2 m_i / k  [i selected]  -  2 (1 - m_i) / n_bone  [i on the bone] )
 * The bone term is formed as (up * coef * 2 / n_bone) * -(1 - m_i) * (on-bone ? 1 : 0), so n_bone == 0 gives NaN in
 * every element, as autograd does for the reference; k == 0 selects nothing. The selection is re-derived from `state`,
 * which the forward wrote: T, Q, n_bone and, per chunk of ENARF_GUIDE chunk geometry (below), how many of the chunk's
 * values with key == T are selected. There is no index tensor.
 *
 * Geometry: the N values are cut into `chunks` consecutive chunks of `chunk_len` values, one workgroup each:
 *   blocks0 = min(ceil(N / 256), ENARF_GUIDE_MAX_BLOCKS), chunk_len = 256 * ceil(ceil(N / blocks0) / 256),
 *   chunks = ceil(N / chunk_len).
 * Forward with_push: one 4 KB memset of the histograms and six kernel launches (four histogram passes, one sum pass,
 * one finishing workgroup); without: the sum pass and the finish. The count depends on nothing but with_push.
 *
 * Refused with ENARF_ERR_ARG, not computed: N == 0, N >= 2^31, s < 1, S < s (a rate of 0), S / rate != s, k outside
 * [0, N], null pointers.
 */
#ifndef ENARF_GUIDE_H
#define ENARF_GUIDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_GUIDE_ABI_VERSION 1

#define ENARF_GUIDE_MAX_BLOCKS 512
#define ENARF_GUIDE_RADIX_BITS 8
#define ENARF_GUIDE_PASSES     4
/* scratch of the forward: 2 * MAX_BLOCKS fp64 partials, PASSES * 256 histogram counters, 2 * MAX_BLOCKS int counts */
#define ENARF_GUIDE_WORK_BYTES (2 * ENARF_GUIDE_MAX_BLOCKS * 8 + (ENARF_GUIDE_PASSES * 256 + 2 * ENARF_GUIDE_MAX_BLOCKS) * 4)
/* what the backward needs of the forward: [T, Q, n_bone, 0, selected ties of chunk 0, 1, ...] (-1 = all of them) */
#define ENARF_GUIDE_STATE_INTS (4 + ENARF_GUIDE_MAX_BLOCKS)

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

int enarf_guide_abi_version(void);
const char *enarf_guide_last_error(void);

/* out[0..2] = loss, push, bone; `work` is scratch of ENARF_GUIDE_WORK_BYTES (8-byte aligned), `state`
 * ENARF_GUIDE_STATE_INTS ints kept for the backward */
int enarf_guide_loss_fwd(const float *fake_mask, const float *bone_mask, int64_t B, int s, int S, int64_t k,
                         int with_push, double coef, void *work, int32_t *state, float *out, void *stream);

/* d_fake_mask (B, s, s) from the device scalar `up` and the forward's `state`: one launch */
int enarf_guide_loss_bwd(const float *fake_mask, const float *bone_mask, int64_t B, int s, int S, int64_t k,
                         int with_push, double coef, const int32_t *state, const float *up, float *d_fake_mask,
                         void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_GUIDE_H */
