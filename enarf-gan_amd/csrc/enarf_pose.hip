// enarf_pose.hip - bone masks of the pose prior (libenarf_pose.so, include/enarf_pose.h).
//
// One launch per batch: pose_mask_kernel, grid (pixel blocks, frames), one thread per pixel. Each workgroup first runs
// a per-frame preamble: 24 lanes project the joints (and write pose_2d from the frame's first workgroup), then 27 lanes
// stage the bones' a, ab, |ab|^2, z_a, z_b and 24 lanes the keypoints' row / column slices in LDS. Each pixel then
// walks the 27 bones in bone order and writes its mask, disparity, part disparities and keypoint values with plain
// vector stores. The template flags drop the disparity arithmetic (three fp64 divisions a bone) and the keypoint stores
// when those outputs are not asked for. All arithmetic is fp64 with FMA contraction off, in the operation order of the
// reference's numpy expressions; nothing depends on scheduling, so every output is a function of the inputs alone.
#include "enarf_pose.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kBlock = 256;
constexpr int kJoints = ENARF_POSE_NUM_JOINTS;
constexpr int kBones = ENARF_POSE_NUM_BONES;
constexpr int kParts = ENARF_POSE_NUM_PARTS;
constexpr int kKeys = ENARF_POSE_NUM_KEYPOINTS;
constexpr int kMaxFramesPerGrid = 65535;

// SMPLProperty after add_blank_part (idx = [0, 0, 0..9, 9, 9, 10..23]), in terms of the 24 original joints.
// Bone k + 1 runs from joint kBoneA[k] (= idx[k + 1]) to joint kBoneB[k] (= idx[prev_seq[k + 1]]).
__constant__ int kBoneA[kBones] = {0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20,
                                   21, 22, 23};
__constant__ int kBoneB[kBones] = {0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 9, 9, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19,
                                   20, 21};
// part group of bone k + 1: the sorted position of (prev_seq[p] if is_blank[p] else p), p = prev_seq[k + 1]
constexpr int kBoneGroup[kBones] = {0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 9, 9, 7, 8, 9, 9, 9, 10, 11, 12, 13, 14, 15, 16,
                                    17, 18};
// valid keypoint i is joint idx[valid_keypoints[i]] of the original 24
__constant__ int kKeyJoint[kKeys] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22,
                                     23};

constexpr bool first_of_group(int k) {
    for (int i = 0; i < k; ++i)
        if (kBoneGroup[i] == kBoneGroup[k]) return false;
    return true;
}

// np.max's rule: NaN wins for good; otherwise a term replaces the running maximum only when it is greater
__device__ __forceinline__ double max_nan(double m, double v) { return (v > m || v != v) ? v : m; }

// numpy's slice bound for an axis of length S
__device__ __forceinline__ int slice_bound(long long v, int S) {
    if (v < 0) v += S;
    return v < 0 ? 0 : (v > S ? S : (int)v);
}

// ceil(v) as an integer when it is finite and within int32, else false (astype(int) is undefined there)
__device__ __forceinline__ bool ceil_int(double v, long long &out) {
    const double c = ceil(v);
    if (!(c >= -2147483648.0 && c <= 2147483647.0)) return false;
    out = (long long)c;
    return true;
}

// the call's pointers and sizes, passed by value to every instantiation
struct Args {
    const double *pose, *K, *jpos;           // jpos: the caller's image coordinates, or null to project with K
    long long B;
    int S;
    double t;
    float *mask, *disparity, *part_disparity, *keypoint_mask;
    double *pose_2d;
};

template <bool kDisp, bool kKeyMask>
__global__ void __launch_bounds__(kBlock) pose_mask_kernel(const Args a) {
#pragma clang fp contract(off)
    __shared__ double jx[kJoints], jy[kJoints], jz[kJoints];
    __shared__ double ax[kBones], ay[kBones], abx[kBones], aby[kBones], abab_s[kBones], za_s[kBones], zb_s[kBones];
    __shared__ int box[kKeys][4];            // row begin, row end, column begin, column end (numpy slice bounds)
    const double *__restrict__ pose = a.pose, *__restrict__ K = a.K, *__restrict__ jpos = a.jpos;
    float *__restrict__ mask = a.mask, *__restrict__ disparity = a.disparity;
    float *__restrict__ part_disparity = a.part_disparity, *__restrict__ keypoint_mask = a.keypoint_mask;
    double *__restrict__ pose_2d = a.pose_2d;
    const long long B = a.B;
    const int S = a.S;
    const double t = a.t;
    const int tid = threadIdx.x;
    const long long npx = (long long)S * S;
    const long long p = (long long)blockIdx.x * kBlock + tid;
    const double t2 = t * t;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        if (tid < kJoints) {
            const double *P = pose + (b * kJoints + tid) * 16;
            const double x = P[3], y = P[7], z = P[11];
            double p0, p1;
            if (jpos) {
                p0 = jpos[(b * kJoints + tid) * 2];
                p1 = jpos[(b * kJoints + tid) * 2 + 1];
            } else {
                const double *Kb = K + b * 9;
                const double u = x / z, v = y / z, w = z / z;
                p0 = Kb[0] * u + Kb[1] * v + Kb[2] * w;
                p1 = Kb[3] * u + Kb[4] * v + Kb[5] * w;
            }
            jx[tid] = p0;
            jy[tid] = p1;
            jz[tid] = z;
            if (pose_2d && blockIdx.x == 0) {
                pose_2d[(b * kJoints + tid) * 2] = p0;
                pose_2d[(b * kJoints + tid) * 2 + 1] = p1;
            }
        }
        __syncthreads();
        if (tid < kBones) {
            const int ja = kBoneA[tid], jb = kBoneB[tid];
            const double bx = jx[jb] - jx[ja], by = jy[jb] - jy[ja];
            ax[tid] = jx[ja];
            ay[tid] = jy[ja];
            abx[tid] = bx;
            aby[tid] = by;
            abab_s[tid] = bx * bx + by * by;
            za_s[tid] = jz[ja];
            zb_s[tid] = jz[jb];
        } else if (kKeyMask && tid >= 64 && tid < 64 + kKeys) {
            const int i = tid - 64, j = kKeyJoint[i];
            long long left = 0, right = 0, top = 0, bottom = 0;
            const bool ok = ceil_int(jx[j] - t, left) && ceil_int(jx[j] + t, right) && ceil_int(jy[j] - t, top) &&
                            ceil_int(jy[j] + t, bottom);
            // a fill with value 0 leaves the zeros as they are: only a box with bottom >= 0 and right >= 0 draws
            const bool draw = ok && bottom >= 0 && right >= 0;
            box[i][0] = draw ? slice_bound(top, S) : 0;
            box[i][1] = draw ? slice_bound(bottom, S) : 0;
            box[i][2] = draw ? slice_bound(left, S) : 0;
            box[i][3] = draw ? slice_bound(right, S) : 0;
        }
        __syncthreads();
        if (p < npx) {
            const int yi = (int)(p / S), xi = (int)(p - (long long)yi * S);
            const double cx = (double)xi, cy = (double)yi;
            bool any = false;
            double dmax = 0.0, pmax[kParts];
#pragma unroll
            for (int k = 0; k < kBones; ++k) {
                const double acx = cx - ax[k], acy = cy - ay[k];
                const double bx = abx[k], by = aby[k], abab = abab_s[k];
                const double acab = acx * bx + acy * by;
                const double acac = acx * acx + acy * acy;
                const bool in = (0.0 <= acab) & (acab <= abab) & (acab * acab >= abab * (acac - t2)) & (abab > 1e-8);
                any |= in;
                if (kDisp) {
                    const double za = za_s[k], zb = zb_s[k];
                    const double s = acab / (abab + 1e-10);
                    const double sza = s * za;
                    const double tt = sza / (sza + (1.0 - s) * zb);
                    const double zc = za * (1.0 - tt) + zb * tt;
                    const double d = 1.0 / (zc + 1e-8) * (in ? 1.0 : 0.0);
                    dmax = k == 0 ? d : max_nan(dmax, d);
                    const int g = kBoneGroup[k];
                    pmax[g] = first_of_group(k) ? d : max_nan(pmax[g], d);
                }
            }
            mask[b * npx + p] = any ? 1.0f : 0.0f;
            if (kDisp) {
                if (disparity) disparity[b * npx + p] = (float)dmax;
                if (part_disparity) {
#pragma unroll
                    for (int g = 0; g < kParts; ++g) part_disparity[(b * kParts + g) * npx + p] = (float)pmax[g];
                }
            }
            if (kKeyMask) {
                for (int i = 0; i < kKeys; ++i) {
                    const bool inside = yi >= box[i][0] && yi < box[i][1] && xi >= box[i][2] && xi < box[i][3];
                    keypoint_mask[(b * kKeys + i) * npx + p] = inside ? 1.0f : 0.0f;
                }
            }
        }
        __syncthreads();                     // the next frame's preamble overwrites the LDS tables
    }
}

template <bool kDisp, bool kKeyMask>
int launch(const Args &a, hipStream_t st) {
    const long long npx = (long long)a.S * a.S;
    const long long frames = a.B < kMaxFramesPerGrid ? a.B : kMaxFramesPerGrid;   // the kernel strides over the rest
    const dim3 grid((unsigned)((npx + kBlock - 1) / kBlock), (unsigned)frames);
    hipLaunchKernelGGL((pose_mask_kernel<kDisp, kKeyMask>), grid, dim3(kBlock), 0, st, a);
    return enarf::host::check_launch("enarf_pose_bone_masks: pose_mask_kernel");
}

}  // namespace

extern "C" {

int enarf_pose_abi_version(void) { return ENARF_POSE_ABI_VERSION; }

const char *enarf_pose_last_error(void) { return enarf::host::last_error(); }

int enarf_pose_bone_masks(const double *pose_to_camera, const double *intrinsics, const double *joint_pos_image,
                          int64_t B, int size, double thickness, float *mask, float *disparity,
                          float *part_disparity, float *keypoint_mask, double *pose_2d, void *stream) {
    const char *who = "enarf_pose_bone_masks";
    if (B < 0 || B >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: batch %lld outside [0, 2^31)", who, (long long)B);
    if (size < 1 || size > ENARF_POSE_MAX_SIZE)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: size %d outside [1, %d]", who, size, ENARF_POSE_MAX_SIZE);
    if (!isfinite(thickness)) return enarf::host::fail(ENARF_ERR_ARG, "%s: thickness %g is not finite", who, thickness);
    if (B > 0 && (!pose_to_camera || (!intrinsics && !joint_pos_image) || !mask))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null pose_to_camera, mask, or both intrinsics and joint_pos_image",
                                 who);
    if (B == 0) return 0;
    const Args a{pose_to_camera, intrinsics, joint_pos_image, (long long)B, size, thickness,
                 mask, disparity, part_disparity, keypoint_mask, pose_2d};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (disparity || part_disparity) return keypoint_mask ? launch<true, true>(a, st) : launch<true, false>(a, st);
    return keypoint_mask ? launch<false, true>(a, st) : launch<false, false>(a, st);
}

}  // extern "C"
