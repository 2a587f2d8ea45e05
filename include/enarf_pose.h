/*
 * enarf_pose.h - C ABI of libenarf_pose.so: the bone masks of the pose prior on the MI355X (gfx950), the
 * create_mask / pose_to_image_coord pair of the reference's HumanPoseDataset (dataset/utils_3d.py,
 * dataset/dataset.py) for the SMPL property set, after add_blank_part. A library of its own, next to libenarf_hip.so,
 * libenarf_mesh.so and libenarf_raster.so; same conventions as enarf_raster.h: raw device pointers and sizes, every
 * call asynchronous on `stream` (a hipStream_t passed as void*, NULL = the null stream) with no host synchronisation, 0
 * on success, a negative ENARF_ERR_* for an argument it rejects (checked on the host, no device needed) or a positive
 * hipError_t; enarf_pose_last_error() gives the message (thread local).
 *
 * Contract. Inputs: pose_to_camera (B, 24, 4, 4) and intrinsics K (B, 3, 3), fp64 row-major on the
 * device; 0 <= B < 2^31, 1 <= S = size <= 4096, t = thickness finite. joint_pos_image (B, 24, 2) fp64 is optional:
 * when it is given it replaces the projection below (create_mask's own input) and K may be null. Everything below is
 * fp64, evaluated in the order written with FMA contraction off, and rounded to fp32 once at an fp32 output.
 *   projection    joint j's translation (x, y, z) = pose[j][0..2][3]; u = x / z, v = y / z, w = z / z (each divided
 *                 by its own z: z = 0 gives inf or NaN, as in numpy); p_r = (K[r][0] u + K[r][1] v) + K[r][2] w.
 *                 pose_2d[j] = (p_0, p_1), or joint_pos_image[j] when that is given.
 *   joints        add_blank_part's idx = [0, 0, 0..9, 9, 9, 10..23] gives 28 joints; bone k = 1..27 runs from
 *                 a = joint k to b = joint prev_seq[k] (SMPLProperty.prev_seq), z_a and z_b being the translations' z.
 *                 Blank parts give zero-length bones.
 *   pixels        pixel (row y, column x) is the integer point c = (x, y). Per bone: ac = c - a, ab = b - a,
 *                 acab = ac.x ab.x + ac.y ab.y, abab = ab.x^2 + ab.y^2, acac = ac.x^2 + ac.y^2;
 *                 in = 0 <= acab && acab <= abab && acab^2 >= abab (acac - t^2) && abab > 1e-8;
 *                 s = acab / (abab + 1e-10), tt = s z_a / (s z_a + (1 - s) z_b), zc = z_a (1 - tt) + z_b tt,
 *                 d = 1 / (zc + 1e-8) * in (so inf * 0 and NaN give NaN, also outside the bone).
 *   mask          1 where some bone has in, else 0 (clip(sum in, 0, 1)).
 *   disparity     the maximum of d over the 27 bones in bone order; part_disparity[g] the maximum over the bones of
 *                 part group g (a bone's group is its part's parent, or the parent's parent when the parent is blank;
 *                 the 19 groups are the sorted distinct ids). A NaN term makes the maximum NaN (np.max), and a term
 *                 replaces the running maximum only when it is greater (so of +0 and -0 the first one stays).
 *   keypoint_mask for each of the 24 valid keypoints (x, y) = (p_0, p_1): left = ceil(x - t), right = ceil(x + t),
 *                 top = ceil(y - t), bottom = ceil(y + t) as integers; rows [top:bottom], columns [left:right] with
 *                 numpy's slice rules (a negative bound wraps to S + bound, then clips to [0, S]) are set to
 *                 (bottom >= 0 && right >= 0). So a box that crosses the top or left border disappears and one that
 *                 crosses the bottom or right border is clipped. A bound that is not finite or lies outside the int32
 *                 range draws nothing: the reference's astype(int) is undefined there.
 *
 * Outputs, bit-identical from run to run: mask (B, S, S) fp32 (required); disparity (B, S, S) fp32, part_disparity
 * (B, 19, S, S) fp32, keypoint_mask (B, 24, S, S) fp32 and pose_2d (B, 24, 2) fp64 (optional: a null pointer is not
 * written).
 */
#ifndef ENARF_POSE_H
#define ENARF_POSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENARF_POSE_ABI_VERSION 1

#define ENARF_POSE_NUM_JOINTS     24   /* SMPL joints of pose_to_camera */
#define ENARF_POSE_NUM_BONES      27   /* bones of the 28 joints after add_blank_part */
#define ENARF_POSE_NUM_PARTS      19   /* part groups of part_disparity */
#define ENARF_POSE_NUM_KEYPOINTS  24   /* valid keypoints of keypoint_mask */
#define ENARF_POSE_MAX_SIZE       4096

#ifndef ENARF_ERR_ARG
#define ENARF_ERR_ARG          (-1)   /* null pointer / size out of range */
#endif
#ifndef ENARF_ERR_UNSUPPORTED
#define ENARF_ERR_UNSUPPORTED  (-2)   /* valid input this implementation does not take (message says what) */
#endif

int enarf_pose_abi_version(void);
const char *enarf_pose_last_error(void);

/* the masks of B poses at S x S, one launch on `stream` */
int enarf_pose_bone_masks(const double *pose_to_camera, const double *intrinsics, const double *joint_pos_image,
                          int64_t B, int size, double thickness, float *mask, float *disparity,
                          float *part_disparity, float *keypoint_mask, double *pose_2d, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ENARF_POSE_H */
