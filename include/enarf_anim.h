/*
 * enarf_anim.h - C ABI of libenarf_anim.so: pose sequences and 8-bit frames on the MI355X (gfx950). Two calls: the
 * reference's interpolate_pose (libraries/NARF/pose_utils.py:48-115) with an optional per-frame turntable angle
 * (rotate_pose, :39-45), and the image conversion of its demo (ENARF_GAN_demo.py:70-79) fused with the background
 * composition of the generator. A library of its own next to libenarf_hip.so; same conventions as enarf_pose.h: raw
 * device pointers and sizes, every call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null
 * stream) with no host synchronisation, 0 on success, a negative ENARF_ERR_* for an argument it rejects (checked on the
 * host, no device needed) or a positive hipError_t; enarf_anim_last_error() gives the message (thread local).
 *
 * enarf_anim_interpolate_pose. key_poses (K, J, 4, 4) fp64 row-major on the device: rigid transforms
 * [R t; 0 0 0 1] of the J joints of K key poses. parents: J ints ON THE HOST (as enarf_prepare_args.parents),
 * parents[0] = -1 and 0 <= parents[j] < j. 1 <= J <= 64, K >= 1, num >= 1; with loop, num % K == 0; without, K >= 2,
 * num >= 2 and num % (K - 1) == 0 (where the reference's concatenate of equal blocks fails). One wavefront per output
 * frame i, lane j = joint j; everything is fp64, evaluated in the order written with FMA contraction off:
 *   clocks        S = K segments with loop, else K - 1; per = num / S. Rotations: t = i K / num with loop, else
 *                 i (K - 1) / (num - 1); s = min(floor(t), S - 1), alpha = t - s. Translations (the reference's
 *                 concatenated linspace blocks): u = i / per (integer), beta = (i % per) / per with loop, else
 *                 (i % per) / (per - 1), and 0 when per = 1. Without loop the two clocks differ slightly; kept.
 *   locals        local_j(k) = inverse(P_k[parents[j]]) P_k[j], the inverse being [R^T, -(R^T t)]; the root's local is
 *                 its own matrix. Rotations from keys s and (s + 1) % K, translations from keys u and (u + 1) % K.
 *   rotation      each rotation block -> unit quaternion by Shepperd's choice of the largest of (m00, m11, m22, trace),
 *                 normalised; d = conj(q0) q1, negated when d.w < 0 (the short arc); |v| = sqrt(d.x^2 + d.y^2 + d.z^2),
 *                 angle = 2 atan2(|v|, d.w); q = q0 (sin(h) v / |v|, cos(h)) with h = alpha angle / 2, q = q0 when
 *                 |v| = 0; back to a matrix. At a relative angle of pi the short arc is not unique.
 *   translation   t0 + (t1 - t0) beta.
 *   kinematics    the locals are staged in LDS; joint j's matrix is the product of the locals of its chain from the root
 *                 down, left-associated: G_j = G_parents[j] local_j.
 *   orbit         optional, (num,) fp64 on the device: frame i becomes R (G - C) + C on the 4 x 4s, with R the reference's
 *                 rotation_matrix(orbit[i]) ([c 0 -s 0; 0 1 0 0; s 0 c 0; 0 0 0 1]) and C zero but for its translation
 *                 column, the mean of the J joint translations (summed in joint order, divided by J).
 * Outputs, bit-identical from run to run: poses (num, J, 4, 4) fp64 (required); poses_f32, the same values rounded once
 * to fp32 (optional); bone_length (num, J - 1, 1) fp32 (optional), sqrt(dx^2 + dy^2 + dz^2) of joint j's translation
 * minus its parent's in the frame as written, computed in fp64 and rounded once. A null optional pointer is not written.
 *
 * enarf_anim_compose_frames. color (F, 3, n) and mask (F, n) fp32 on the device, n = S * S pixels; the background is
 * the scalar bg_value when background is null, else fp32 images (F, 3, n) with bg_frame_stride = 3 n, or one shared
 * image (1, 3, n) with bg_frame_stride = 0. Per pixel and channel, in fp32 with contraction off and in this order:
 * v = c + (1 - m) bg; w = v 127.5 + 127.5; clamp to [0, 255]; truncate. masks: m 255, clamped and truncated. A NaN
 * gives 0. frames (F, S, S, 3) uint8 (required, 4-byte aligned), masks (F, S, S) uint8 (optional, 4-byte aligned).
 * Each thread takes four consecutive pixels of the flat (F n) pixel range, so its 12 output bytes leave as three aligned
 * dwords; the last (F n) % 4 pixels are written byte by byte. 0 <= F, 1 <= S <= 4096, F n < 2^40.
 */
#ifndef ENARF_ANIM_H
#define ENARF_ANIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_ANIM_ABI_VERSION 1

#define ENARF_ANIM_MAX_JOINTS  64     /* one wavefront per frame, one lane per joint */
#define ENARF_ANIM_MAX_SIZE    4096

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

int enarf_anim_abi_version(void);
const char *enarf_anim_last_error(void);

/* num interpolated poses from K key poses, one launch on `stream` */
int enarf_anim_interpolate_pose(const double *key_poses, const int32_t *parents_host, int K, int J, int num, int loop,
                                const double *orbit, double *poses, float *poses_f32, float *bone_length,
                                void *stream);

/* F rendered frames to 8-bit images, one launch on `stream` */
int enarf_anim_compose_frames(const float *color, const float *mask, const float *background,
                              int64_t bg_frame_stride, float bg_value, int64_t F, int size, uint8_t *frames,
                              uint8_t *masks, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_ANIM_H */
