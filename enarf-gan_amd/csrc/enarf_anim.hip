// enarf_anim.hip - pose sequences and 8-bit frames (libenarf_anim.so, include/enarf_anim.h).
//
// anim_pose_kernel: one wavefront per output frame, lane j = joint j. Each lane forms its joint's parent-relative
// transform in the key poses of its segment, slerps the rotation and lerps the offset, stages the local in LDS and then
// multiplies its chain of locals from the root down; the optional turntable needs the mean joint translation and the
// bone lengths the parent's translation, both read back from LDS. All fp64 with FMA contraction off, in the operation
// order of the header; nothing depends on scheduling, so every output is a function of the inputs alone.
//
// anim_compose_kernel: one thread per four consecutive pixels of the flat (frame, pixel) range; their 12 bytes leave as
// three aligned dwords, the last (F n) % 4 pixels byte by byte. One division per thread finds the group's frame; when
// n % 4 == 0 (and the inputs are 16-byte aligned) the group is four floats of one frame and each plane is one load,
// otherwise the thread steps pixel by pixel, across a frame boundary if need be.
#include "enarf_anim.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kMaxJoints = ENARF_ANIM_MAX_JOINTS;
constexpr int kBlock = 256;
static_assert(kMaxJoints == kWave, "one lane per joint");

struct PoseArgs {
    const double *key, *orbit;
    double *out;
    float *out32, *bone_length;
    int K, J, num, loop;
    signed char parents[kMaxJoints];         // validated on the host: parents[0] = -1, 0 <= parents[j] < j
};

struct Rigid {
    double r[9], t[3];                       // rotation row-major, translation
};

__device__ __forceinline__ void load_rigid(const double *__restrict__ P, Rigid &m) {
    m.r[0] = P[0]; m.r[1] = P[1]; m.r[2] = P[2];  m.t[0] = P[3];
    m.r[3] = P[4]; m.r[4] = P[5]; m.r[5] = P[6];  m.t[1] = P[7];
    m.r[6] = P[8]; m.r[7] = P[9]; m.r[8] = P[10]; m.t[2] = P[11];
}

// inverse(parent) child, the inverse being [R^T, -(R^T t)]
__device__ __forceinline__ void local_of(const Rigid &p, const Rigid &c, Rigid &l) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) l.r[3 * a + b] = (p.r[a] * c.r[b] + p.r[3 + a] * c.r[3 + b]) + p.r[6 + a] * c.r[6 + b];
        const double tinv = -((p.r[a] * p.t[0] + p.r[3 + a] * p.t[1]) + p.r[6 + a] * p.t[2]);
        l.t[a] = ((p.r[a] * c.t[0] + p.r[3 + a] * c.t[1]) + p.r[6 + a] * c.t[2]) + tinv;
    }
}

// joint j's parent-relative transform in one key pose (the root's is its own matrix)
__device__ __forceinline__ void key_local(const double *__restrict__ pose, int j, int parent, Rigid &l) {
    Rigid c;
    load_rigid(pose + (long long)j * 16, c);
    if (parent < 0) {
        l = c;
    } else {
        Rigid p;
        load_rigid(pose + (long long)parent * 16, p);
        local_of(p, c, l);
    }
}

// unit quaternion (x, y, z, w) of a rotation matrix: Shepperd's choice of the largest of (m00, m11, m22, trace)
__device__ __forceinline__ void quat_of(const double *m, double *q) {
    const double tr = (m[0] + m[4]) + m[8];
    int c = 0;
    double best = m[0];
    if (m[4] > best) { c = 1; best = m[4]; }
    if (m[8] > best) { c = 2; best = m[8]; }
    if (tr > best) c = 3;
    if (c == 3) {
        q[0] = m[7] - m[5]; q[1] = m[2] - m[6]; q[2] = m[3] - m[1]; q[3] = 1.0 + tr;
    } else if (c == 0) {
        q[0] = (1.0 - tr) + 2.0 * m[0]; q[1] = m[3] + m[1]; q[2] = m[6] + m[2]; q[3] = m[7] - m[5];
    } else if (c == 1) {
        q[1] = (1.0 - tr) + 2.0 * m[4]; q[2] = m[7] + m[5]; q[0] = m[1] + m[3]; q[3] = m[2] - m[6];
    } else {
        q[2] = (1.0 - tr) + 2.0 * m[8]; q[0] = m[2] + m[6]; q[1] = m[5] + m[7]; q[3] = m[3] - m[1];
    }
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

__device__ __forceinline__ void quat_mul(const double *a, const double *b, double *o) {
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    o[1] = ((a[3] * b[1] - a[0] * b[2]) + a[1] * b[3]) + a[2] * b[0];
    o[2] = ((a[3] * b[2] + a[0] * b[1]) - a[1] * b[0]) + a[2] * b[3];
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
}

__device__ __forceinline__ void matrix_of(const double *q, double *m) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    m[0] = 1.0 - 2.0 * (y * y + z * z); m[1] = 2.0 * (x * y - z * w);       m[2] = 2.0 * (x * z + y * w);
    m[3] = 2.0 * (x * y + z * w);       m[4] = 1.0 - 2.0 * (x * x + z * z); m[5] = 2.0 * (y * z - x * w);
    m[6] = 2.0 * (x * z - y * w);       m[7] = 2.0 * (y * z + x * w);       m[8] = 1.0 - 2.0 * (x * x + y * y);
}

// q0 exp(alpha log(conj(q0) q1)) along the short arc
__device__ __forceinline__ void slerp(const double *q0, const double *q1, double alpha, double *q) {
    const double conj[4] = {-q0[0], -q0[1], -q0[2], q0[3]};
    double d[4];
    quat_mul(conj, q1, d);
    if (d[3] < 0.0) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; d[3] = -d[3]; }
    const double s = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (s == 0.0) {
        q[0] = q0[0]; q[1] = q0[1]; q[2] = q0[2]; q[3] = q0[3];
        return;
    }
    const double angle = 2.0 * atan2(s, d[3]);
    const double h = alpha * angle / 2.0;
    const double sh = sin(h), ch = cos(h);
    const double e[4] = {d[0] / s * sh, d[1] / s * sh, d[2] / s * sh, ch};
    quat_mul(q0, e, q);
}

__global__ void __launch_bounds__(kWave) anim_pose_kernel(const PoseArgs a) {
    __shared__ double loc[kMaxJoints][12];                 // the locals: r00 r01 r02 t0 | r10 .. | r20 ..
    __shared__ double gt[kMaxJoints][3], ft[kMaxJoints][3];  // translations after the kinematics / as written
    __shared__ unsigned char chain[kMaxJoints][kMaxJoints];  // joint, parent, .., root
    __shared__ signed char par[kMaxJoints];
    const int j = threadIdx.x, J = a.J, K = a.K, num = a.num;
    const int i = blockIdx.x;
    const bool live = j < J;
    int parent = -1;
    if (live) {
        parent = a.parents[j];
        if (parent >= j) parent = -1;                      // never taken after the host's check; keeps the walk in bounds
        par[j] = (signed char)parent;
        // the two clocks
        const int S = a.loop ? K : K - 1;
        const int per = num / S;
        const double t = a.loop ? (double)i * (double)K / (double)num : (double)i * (double)(K - 1) / (double)(num - 1);
        int s = (int)floor(t);
        if (s > S - 1) s = S - 1;
        const double alpha = t - (double)s;
        const int u = i / per, r = i % per;
        const double beta = a.loop ? (double)r / (double)per : (per > 1 ? (double)r / (double)(per - 1) : 0.0);
        const long long stride = (long long)J * 16;
        Rigid l0, l1;
        double q0[4], q1[4], q[4], m[9];
        key_local(a.key + s * stride, j, parent, l0);
        key_local(a.key + ((s + 1) % K) * stride, j, parent, l1);
        quat_of(l0.r, q0);
        quat_of(l1.r, q1);
        slerp(q0, q1, alpha, q);
        matrix_of(q, m);
        if (u != s) {                                      // the translation's own segment (only without loop)
            key_local(a.key + u * stride, j, parent, l0);
            key_local(a.key + ((u + 1) % K) * stride, j, parent, l1);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            loc[j][4 * c] = m[3 * c];
            loc[j][4 * c + 1] = m[3 * c + 1];
            loc[j][4 * c + 2] = m[3 * c + 2];
            loc[j][4 * c + 3] = l0.t[c] + (l1.t[c] - l0.t[c]) * beta;
        }
    }
    __syncthreads();
    Rigid g;
    if (live) {
        int n = 0;
        for (int c = j; c >= 0 && n < kMaxJoints; c = par[c]) chain[j][n++] = (unsigned char)c;
        const double *L = loc[chain[j][n - 1]];            // identity times the root's local
        g.r[0] = L[0]; g.r[1] = L[1]; g.r[2] = L[2];  g.t[0] = L[3];
        g.r[3] = L[4]; g.r[4] = L[5]; g.r[5] = L[6];  g.t[1] = L[7];
        g.r[6] = L[8]; g.r[7] = L[9]; g.r[8] = L[10]; g.t[2] = L[11];
        for (int k = n - 2; k >= 0; --k) {
            L = loc[chain[j][k]];
            Rigid o;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double g0 = g.r[3 * r], g1 = g.r[3 * r + 1], g2 = g.r[3 * r + 2];
#pragma unroll
                for (int c = 0; c < 3; ++c) o.r[3 * r + c] = (g0 * L[c] + g1 * L[4 + c]) + g2 * L[8 + c];
                o.t[r] = ((g0 * L[3] + g1 * L[7]) + g2 * L[11]) + g.t[r];
            }
            g = o;
        }
        gt[j][0] = g.t[0]; gt[j][1] = g.t[1]; gt[j][2] = g.t[2];
    }
    __syncthreads();
    if (live) {
        if (a.orbit) {
            double cx = 0.0, cy = 0.0, cz = 0.0;
            for (int k = 0; k < J; ++k) { cx += gt[k][0]; cy += gt[k][1]; cz += gt[k][2]; }
            cx /= (double)J; cy /= (double)J; cz /= (double)J;
            const double th = a.orbit[i];
            const double c = cos(th), s = sin(th);
            Rigid o;
#pragma unroll
            for (int k = 0; k < 3; ++k) {                  // the rotation columns: R G
                o.r[k] = c * g.r[k] + (-s) * g.r[6 + k];
                o.r[3 + k] = g.r[3 + k];
                o.r[6 + k] = s * g.r[k] + c * g.r[6 + k];
            }
            const double x = g.t[0] - cx, y = g.t[1] - cy, z = g.t[2] - cz;
            o.t[0] = (c * x + (-s) * z) + cx;
            o.t[1] = y + cy;
            o.t[2] = (s * x + c * z) + cz;
            g = o;
        }
        ft[j][0] = g.t[0]; ft[j][1] = g.t[1]; ft[j][2] = g.t[2];
        const long long at = ((long long)i * J + j) * 16;
        const double row[16] = {g.r[0], g.r[1], g.r[2], g.t[0], g.r[3], g.r[4], g.r[5], g.t[1],
                                g.r[6], g.r[7], g.r[8], g.t[2], 0.0, 0.0, 0.0, 1.0};
#pragma unroll
        for (int k = 0; k < 16; ++k) a.out[at + k] = row[k];
        if (a.out32) {
#pragma unroll
            for (int k = 0; k < 16; ++k) a.out32[at + k] = (float)row[k];
        }
    }
    __syncthreads();
    if (live && a.bone_length && j >= 1) {
        const int p = parent < 0 ? j : parent;
        const double dx = ft[j][0] - ft[p][0], dy = ft[j][1] - ft[p][1], dz = ft[j][2] - ft[p][2];
        a.bone_length[(long long)i * (J - 1) + (j - 1)] = (float)sqrt((dx * dx + dy * dy) + dz * dz);
    }
}

struct ComposeArgs {
    const float *color, *mask, *bg;
    long long bg_stride, n, total;           // pixels a frame, pixels in all
    float bg_value;
    int vec;                                 // n % 4 == 0 and 16-byte aligned inputs: a group is four floats of one frame
    uint8_t *frames, *masks;
};

__device__ __forceinline__ unsigned byte_of(float w) {
    w = w > 0.0f ? w : 0.0f;                 // a NaN fails the comparison and gives 0
    w = w < 255.0f ? w : 255.0f;
    return (unsigned)w;
}

__device__ __forceinline__ unsigned channel_byte(float c, float m, float bg) {
    const float v = c + (1.0f - m) * bg;
    return byte_of(v * 127.5f + 127.5f);
}

__device__ __forceinline__ void unpack4(const float *__restrict__ at, float *v) {
    const float4 q = *reinterpret_cast<const float4 *>(at);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

__global__ void __launch_bounds__(kBlock) anim_compose_kernel(const ComposeArgs a) {
    const long long g0 = ((long long)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (g0 >= a.total) return;
    const long long left = a.total - g0;
    const int cnt = left < 4 ? (int)left : 4;
    const long long n = a.n;
    long long f = g0 / n, p = g0 - f * n;     // the one division of the thread; the group steps on from here
    float c[3][4], m[4], bg[3][4];
    if (a.vec) {                             // the four pixels lie in one frame, at a multiple of four: one load a plane
        unpack4(a.mask + g0, m);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            unpack4(a.color + (f * 3 + ch) * n + p, c[ch]);
            if (a.bg) unpack4(a.bg + f * a.bg_stride + ch * n + p, bg[ch]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool live = k < cnt;
            m[k] = live ? a.mask[g0 + k] : 0.0f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                c[ch][k] = live ? a.color[(f * 3 + ch) * n + p] : 0.0f;
                if (a.bg) bg[ch][k] = live ? a.bg[f * a.bg_stride + ch * n + p] : 0.0f;
            }
            if (++p == n) { p = 0; ++f; }    // into the next frame
        }
    }
    unsigned px[4], mb[4];                   // the three channel bytes of a pixel in bits 0..23; its mask byte
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        mb[k] = byte_of(m[k] * 255.0f);
        px[k] = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) px[k] |= channel_byte(c[ch][k], m[k], a.bg ? bg[ch][k] : a.bg_value) << (8 * ch);
    }
    if (cnt == 4) {
        unsigned *__restrict__ out = reinterpret_cast<unsigned *>(a.frames + g0 * 3);    // 12 q bytes in: dword aligned
        out[0] = px[0] | (px[1] << 24);
        out[1] = (px[1] >> 8) | (px[2] << 16);
        out[2] = (px[2] >> 16) | (px[3] << 8);
        if (a.masks) *reinterpret_cast<unsigned *>(a.masks + g0) = mb[0] | (mb[1] << 8) | (mb[2] << 16) | (mb[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < cnt) {
                a.frames[(g0 + k) * 3] = (uint8_t)(px[k] & 0xFFu);
                a.frames[(g0 + k) * 3 + 1] = (uint8_t)((px[k] >> 8) & 0xFFu);
                a.frames[(g0 + k) * 3 + 2] = (uint8_t)(px[k] >> 16);
                if (a.masks) a.masks[g0 + k] = (uint8_t)mb[k];
            }
        }
    }
}

}  // namespace

extern "C" {

int enarf_anim_abi_version(void) { return ENARF_ANIM_ABI_VERSION; }

const char *enarf_anim_last_error(void) { return enarf::host::last_error(); }

int enarf_anim_interpolate_pose(const double *key_poses, const int32_t *parents_host, int K, int J, int num, int loop,
                                const double *orbit, double *poses, float *poses_f32, float *bone_length,
                                void *stream) {
    const char *who = "enarf_anim_interpolate_pose";
    if (J < 1 || J > kMaxJoints) return enarf::host::fail(ENARF_ERR_ARG, "%s: %d joints outside [1, %d]", who, J, kMaxJoints);
    if (K < 1) return enarf::host::fail(ENARF_ERR_ARG, "%s: %d key poses, at least 1 is needed", who, K);
    if (num < 1) return enarf::host::fail(ENARF_ERR_ARG, "%s: num %d < 1", who, num);
    if (!loop && (K < 2 || num < 2))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: without loop at least 2 key poses and 2 frames are needed, got %d and %d",
                                 who, K, num);
    const int S = loop ? K : K - 1;
    if (num % S != 0)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: num %d is not a multiple of the %d segments", who, num, S);
    if (!key_poses || !parents_host || !poses) return enarf::host::fail(ENARF_ERR_ARG, "%s: null key_poses, parents or poses", who);
    PoseArgs a{key_poses, orbit, poses, poses_f32, bone_length, K, J, num, loop ? 1 : 0, {}};
    for (int j = 0; j < J; ++j) {
        const int p = parents_host[j];
        if (j == 0 ? p != -1 : (p < 0 || p >= j))
            return enarf::host::fail(ENARF_ERR_ARG, "%s: parents[%d] = %d: the root comes first and a parent before its joint",
                                     who, j, p);
        a.parents[j] = (signed char)p;
    }
    hipLaunchKernelGGL(anim_pose_kernel, dim3((unsigned)num), dim3(kWave), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_anim_interpolate_pose: anim_pose_kernel");
}

int enarf_anim_compose_frames(const float *color, const float *mask, const float *background,
                              int64_t bg_frame_stride, float bg_value, int64_t F, int size, uint8_t *frames,
                              uint8_t *masks, void *stream) {
    const char *who = "enarf_anim_compose_frames";
    if (size < 1 || size > ENARF_ANIM_MAX_SIZE)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: size %d outside [1, %d]", who, size, ENARF_ANIM_MAX_SIZE);
    const long long n = (long long)size * size;
    if (F < 0 || F > (1LL << 40) / n) return enarf::host::fail(ENARF_ERR_ARG, "%s: %lld frames outside [0, 2^40 / n]", who, (long long)F);
    if (background && bg_frame_stride != 0 && bg_frame_stride != 3 * n)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: background frame stride %lld is neither 0 nor 3 n", who,
                                 (long long)bg_frame_stride);
    if (F == 0) return 0;
    if (!color || !mask || !frames) return enarf::host::fail(ENARF_ERR_ARG, "%s: null color, mask or frames", who);
    if ((reinterpret_cast<uintptr_t>(frames) & 3u) || (reinterpret_cast<uintptr_t>(masks) & 3u))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: frames and masks must be 4-byte aligned", who);
    const uintptr_t inputs = reinterpret_cast<uintptr_t>(color) | reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(background);
    const int vec = n % 4 == 0 && (inputs & 15u) == 0;
    const ComposeArgs a{color, mask, background, (long long)bg_frame_stride, n, (long long)F * n, bg_value, vec, frames, masks};
    const long long groups = (a.total + 3) / 4, blocks = (groups + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFFLL) return enarf::host::fail(ENARF_ERR_ARG, "%s: %lld pixels are too many for one launch", who, a.total);
    hipLaunchKernelGGL(anim_compose_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_anim_compose_frames: anim_compose_kernel");
}

}  // extern "C"
