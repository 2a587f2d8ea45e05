// enarf_skin.hip - libenarf_skin.so: rigged meshes (gfx950 / CDNA4 only, wave64). The contract is in include/enarf_skin.h.
//
//   skin_weights_kernel<K>  one lane per vertex: the bone transforms and cube tests of the query and the march (the
//                           walk of enarf_parts.h, so the validity bits are theirs bit for bit), the part probability
//                           of every valid pair as seg_label_kernel forms it, and the K largest kept by
//                           sorted insertion into K registers - no feature gather, no MLP, no per-part array.
//   skin_pose_kernel<K>     one lane per vertex, a workgroup per (256 vertices, 8 frames): the frames' part transforms
//                           staged in LDS in fp64, the vertex, its joints and weights read once, one fp64 blend a frame.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "enarf_skin.h"
#include "enarf_parts.h"
#include "enarf_host.h"

namespace {

using namespace enarf;

constexpr int kBlock = 256;
constexpr int kMaxParts = ENARF_SKIN_MAX_PARTS;
constexpr int kFrames = ENARF_SKIN_FRAMES_PER_GROUP;
constexpr int kXf = 12;                 // doubles a transform: L row-major 9, then the translation 3
static_assert(kMaxParts == ENARF_MAX_PARTS, "the bit mask of the march");
static_assert(kFrames * kMaxParts <= kBlock, "one lane stages one transform");

template <int K>
__global__ void __launch_bounds__(kBlock) skin_weights_kernel(const enarf_skin_weights_args a) {
    __shared__ __attribute__((aligned(16))) float l_parts[kMaxParts * kLdsPartStride];
    __shared__ __attribute__((aligned(16))) float l_canon[kMaxParts * kLdsCanonStride];
    const int tid = threadIdx.x, P = a.P;
    stage_frames(l_parts, l_canon, a.parts, a.canonical_pose, P, tid, kBlock);
    __syncthreads();
    const long long i = (long long)blockIdx.x * kBlock + tid;
    if (i >= a.V) return;

    const float *p = a.vertices + i * a.vert_stride;
    const float px = exact_mul(p[0], a.coordinate_scale), py = exact_mul(p[a.comp_stride], a.coordinate_scale),
                pz = exact_mul(p[2 * a.comp_stride], a.coordinate_scale);

    const char *maskb = reinterpret_cast<const char *>(a.mask_planes);
    const unsigned plane_bytes = (unsigned)(a.H * a.W) << 2;       // 3 P planes stay below 2^32 bytes (checked on the host)
    const float uniform_w = a.uniform_part_weight ? 1.0f / (float)P : 0.0f;
    uint32_t bits = 0;
    int jk[K], n_valid = 0, near_k = 0;
    float wk[K], near_d = __builtin_inff();
    double total = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) { jk[j] = -1; wk[j] = -1.0f; }
    for (int k = 0; k < P; ++k) {
        float F[13], Cn[12], lx, ly, lz, cx, cy, cz;
        load_frames(l_parts, l_canon, k, F, Cn);
        part_point(F, Cn, px, py, pz, lx, ly, lz, cx, cy, cz);
        const float d = fmaxf(fmaxf(fabsf(lx), fabsf(ly)), fabsf(lz));
        if (d < near_d) { near_d = d; near_k = k; }          // strictly: the lowest index wins a tie
        if (!ENARF_POINT_IN_PART(lx, ly, lz, cx, cy, cz)) continue;
        bits |= 1u << k;
        ++n_valid;
        float w = uniform_w;
        if (!a.uniform_part_weight) w = part_probability(maskb, k, plane_bytes, cx, cy, cz, a.H, a.W, a.clamp_mask);
        total += (double)w;
        // sorted insertion: the newcomer passes every slot it does not strictly beat, then pushes the rest down one
        float cw = w;
        int ck = k;
        bool moving = false;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (moving || cw > wk[j]) {
                const float tw = wk[j];
                const int tk = jk[j];
                wk[j] = cw; jk[j] = ck;
                cw = tw; ck = tk;
                moving = true;
            }
        }
    }
    double kept = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) kept += jk[j] >= 0 ? (double)wk[j] : 0.0;
    float wn[K];
#pragma unroll
    for (int j = 0; j < K; ++j)          // kept == 0: every kept weight underflowed to 0, the slots then share the vertex
        wn[j] = jk[j] < 0 ? 0.0f : kept > 0.0 ? (float)((double)wk[j] / kept) : 1.0f / (float)min(n_valid, K);
    float mass = (n_valid <= K || !(total > 0.0)) ? 1.0f : (float)(kept / total);
    if (bits == 0) {                       // no part contains the vertex: it follows the nearest cube
        jk[0] = near_k;
        wn[0] = 1.0f;
        mass = 0.0f;
    }
    int4 *jo = reinterpret_cast<int4 *>(a.joints + i * K);
    float4 *wo = reinterpret_cast<float4 *>(a.weights + i * K);
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        jo[q] = make_int4(jk[4 * q], jk[4 * q + 1], jk[4 * q + 2], jk[4 * q + 3]);
        wo[q] = make_float4(wn[4 * q], wn[4 * q + 1], wn[4 * q + 2], wn[4 * q + 3]);
    }
    a.kept_mass[i] = mass;
    if (a.valid_bits) a.valid_bits[i] = bits;
}

template <int K>
__global__ void __launch_bounds__(kBlock) skin_pose_kernel(const enarf_skin_pose_args a) {
    extern __shared__ __attribute__((aligned(16))) double l_xf[];      // [frame of the group][part][12]
    const int tid = threadIdx.x, P = a.P;
    const int f0 = blockIdx.y * kFrames;
    const int nf = min(kFrames, a.F - f0);
    if (tid < nf * P) {                    // one lane a transform
#pragma clang fp contract(off)
        const int f = tid / P, k = tid - f * P;
        const float *A = a.parts_rest + k * kPartStride;
        const float *B = a.parts + ((size_t)(f0 + f) * P + k) * kPartStride;
        const double cs = (double)a.coordinate_scale;
        const double rho = (double)A[12] / (double)B[12];
        const double ta[3] = {(double)A[9] / cs, (double)A[10] / cs, (double)A[11] / cs};
        double *X = l_xf + (size_t)tid * kXf;
#pragma unroll 1
        for (int r = 0; r < 3; ++r) {
            double L[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                L[c] = rho * (((double)B[3 * r] * (double)A[3 * c] + (double)B[3 * r + 1] * (double)A[3 * c + 1]) +
                              (double)B[3 * r + 2] * (double)A[3 * c + 2]);
                X[3 * r + c] = L[c];
            }
            X[9 + r] = (double)B[9 + r] / cs - ((L[0] * ta[0] + L[1] * ta[1]) + L[2] * ta[2]);
        }
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * kBlock + tid;
    if (i >= a.V) return;
    const float *p = a.vertices + i * a.vert_stride;
    const double vx = (double)p[0], vy = (double)p[a.comp_stride], vz = (double)p[2 * a.comp_stride];
    int jk[K];
    float wk[K];
    const int4 *ji = reinterpret_cast<const int4 *>(a.joints + i * K);
    const float4 *wi = reinterpret_cast<const float4 *>(a.weights + i * K);
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        const int4 j4 = ji[q];
        const float4 w4 = wi[q];
        jk[4 * q] = j4.x; jk[4 * q + 1] = j4.y; jk[4 * q + 2] = j4.z; jk[4 * q + 3] = j4.w;
        wk[4 * q] = w4.x; wk[4 * q + 1] = w4.y; wk[4 * q + 2] = w4.z; wk[4 * q + 3] = w4.w;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        jk[j] = (jk[j] < 0 || jk[j] >= P) ? -1 : jk[j] * kXf;      // the slot's offset into a frame's table
    float *o = a.out + (long long)f0 * a.out_frame_stride + i * 3;
    for (int f = 0; f < nf; ++f, o += a.out_frame_stride) {
        const double *Xf = l_xf + (size_t)f * P * kXf;
        double ax = 0.0, ay = 0.0, az = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (jk[j] < 0) continue;
            const double2 *X = reinterpret_cast<const double2 *>(Xf + jk[j]);
            const double2 x0 = X[0], x1 = X[1], x2 = X[2], x3 = X[3], x4 = X[4], x5 = X[5];
            const double w = (double)wk[j];
            // rows (x0.x x0.y x1.x), (x1.y x2.x x2.y), (x3.x x3.y x4.x); translation (x4.y x5.x x5.y)
            ax += w * (((x0.x * vx + x0.y * vy) + x1.x * vz) + x4.y);
            ay += w * (((x1.y * vx + x2.x * vy) + x2.y * vz) + x5.x);
            az += w * (((x3.x * vx + x3.y * vy) + x4.x * vz) + x5.y);
        }
        o[0] = (float)ax; o[1] = (float)ay; o[2] = (float)az;
    }
}

template <int K>
int launch_weights(const enarf_skin_weights_args &a, hipStream_t stream) {
    hipLaunchKernelGGL(skin_weights_kernel<K>, dim3((unsigned)((a.V + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a);
    return enarf::host::check_launch("enarf_skin_weights: skin_weights_kernel");
}

template <int K>
int launch_pose(const enarf_skin_pose_args &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.V + kBlock - 1) / kBlock), (unsigned)((a.F + kFrames - 1) / kFrames));
    const size_t lds = (size_t)kFrames * a.P * kXf * sizeof(double);
    hipLaunchKernelGGL(skin_pose_kernel<K>, grid, dim3(kBlock), lds, stream, a);
    return enarf::host::check_launch("enarf_skin_pose: skin_pose_kernel");
}

}  // namespace

extern "C" {

int enarf_skin_abi_version(void) { return ENARF_SKIN_ABI_VERSION; }

const char *enarf_skin_last_error(void) { return enarf::host::last_error(); }

int enarf_skin_weights(const enarf_skin_weights_args *args, void *stream) {
    const char *who = "enarf_skin_weights";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_skin_weights_args &a = *args;
    if (a.max_influences != 4 && a.max_influences != 8)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: max_influences %d, takes 4 or 8", who, a.max_influences);
    if (const int e = enarf::host::check_part_planes(who, a.P, kMaxParts, a.H, a.W)) return e;
    if (a.V < 0 || a.V / kBlock + 1 >= (1LL << 31)) return enarf::host::fail(ENARF_ERR_ARG, "%s: %lld vertices", who, (long long)a.V);
    if (a.vert_stride < 0 || a.comp_stride < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: negative vertex strides", who);
    if (a.V == 0) return 0;
    if (!a.vertices || !a.parts || !a.canonical_pose || (!a.mask_planes && !a.uniform_part_weight) || !a.joints || !a.weights ||
        !a.kept_mass)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null vertices, parts, canonical_pose, mask_planes, joints, weights or kept_mass", who);
    if (((uintptr_t)a.joints | (uintptr_t)a.weights) & 15)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: joints and weights must be 16-byte aligned", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return a.max_influences == 4 ? launch_weights<4>(a, s) : launch_weights<8>(a, s);
}

int enarf_skin_pose(const enarf_skin_pose_args *args, void *stream) {
    const char *who = "enarf_skin_pose";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_skin_pose_args &a = *args;
    if (a.max_influences != 4 && a.max_influences != 8)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: max_influences %d, takes 4 or 8", who, a.max_influences);
    if (a.P < 1 || a.P > kMaxParts) return enarf::host::fail(ENARF_ERR_ARG, "%s: %d parts outside [1, %d]", who, a.P, kMaxParts);
    if (a.F < 0 || a.F > 65535 * kFrames) return enarf::host::fail(ENARF_ERR_ARG, "%s: %d frames outside [0, %d]", who, a.F, 65535 * kFrames);
    if (a.V < 0 || a.V / kBlock + 1 >= (1LL << 31)) return enarf::host::fail(ENARF_ERR_ARG, "%s: %lld vertices", who, (long long)a.V);
    if (a.vert_stride < 0 || a.comp_stride < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: negative vertex strides", who);
    if (a.out_frame_stride < 3 * a.V)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: out_frame_stride %lld below 3 V = %lld", who, (long long)a.out_frame_stride,
                                 (long long)(3 * a.V));
    if (!(a.coordinate_scale > 0.0f)) return enarf::host::fail(ENARF_ERR_ARG, "%s: coordinate_scale %g not positive", who, (double)a.coordinate_scale);
    if (a.V == 0 || a.F == 0) return 0;
    if (!a.vertices || !a.joints || !a.weights || !a.parts_rest || !a.parts || !a.out)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null vertices, joints, weights, parts_rest, parts or out", who);
    if (((uintptr_t)a.joints | (uintptr_t)a.weights) & 15)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: joints and weights must be 16-byte aligned", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return a.max_influences == 4 ? launch_pose<4>(a, s) : launch_pose<8>(a, s);
}

}  // extern "C"
