// enarf_seg.hip - libenarf_seg.so: part segmentation (gfx950 / CDNA4 only, wave64). The contract is in include/enarf_seg.h.
//
//   seg_label_kernel      one lane per point: the bone transforms and cube tests of the query and the march (the walk of
//                         enarf_parts.h, so the validity bits are theirs bit for bit), the part probability
//                         of every valid pair, and a running best / runner-up - no feature gather, no MLP, no per-part
//                         array. Consecutive lanes take consecutive samples of a ray, so validity is coherent in a wave.
//   seg_composite_kernel  one wavefront per ray, lanes as samples: the semantic colour, and the per-part masses by
//                         peeling the distinct labels of the wave with a ballot - no atomics, no per-lane array.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "enarf_seg.h"
#include "enarf_parts.h"
#include "enarf_host.h"

namespace {

using namespace enarf;

constexpr int kBlock = 256;
constexpr int kMaxParts = ENARF_SEG_MAX_PARTS;
static_assert(kMaxParts == ENARF_MAX_PARTS, "the bit mask of the march");

__global__ void __launch_bounds__(kBlock) seg_label_kernel(const enarf_seg_label_args a) {
    __shared__ __attribute__((aligned(16))) float l_parts[kMaxParts * kLdsPartStride];
    __shared__ __attribute__((aligned(16))) float l_canon[kMaxParts * kLdsCanonStride];
    const int tid = threadIdx.x, b = blockIdx.y, P = a.P;
    const float *parts_b = a.parts + (size_t)b * P * kPartStride;
    stage_frames(l_parts, l_canon, parts_b, a.canonical_pose, P, tid, kBlock);
    __syncthreads();
    const long long i = (long long)blockIdx.x * kBlock + tid;
    if (i >= a.M) return;

    float px, py, pz;
    if (a.points) {
        const float *p = a.points + (long long)b * a.point_batch_stride + i * a.point_stride;
        px = p[0]; py = p[a.comp_stride]; pz = p[2 * a.comp_stride];
    } else {   // the fine pass of the march: enarf_render.hip (ray set-up), enarf_tasks.h ray_segment / ray_tile
        const int n = a.n, Nf = a.Nf;
        const long long ray = i / Nf;
        const float *coord = a.image_coord + (size_t)b * 3 * n;
        const float *Ki = a.inv_intrinsics + (size_t)b * 9;
        const float u = coord[ray], v = coord[n + ray], w = coord[2 * (long long)n + ray];
        const float dx = exact_dot3(Ki[0], u, Ki[1], v, Ki[2], w);
        const float dy = exact_dot3(Ki[3], u, Ki[4], v, Ki[5], w);
        const float dz = exact_dot3(Ki[6], u, Ki[7], v, Ki[8], w);
        const float dmin = a.depth_min[(size_t)b * n + ray], dmax = a.depth_max[(size_t)b * n + ray];
        const float bi = a.bins[(size_t)b * a.M + i];
        px = exact_lerp(exact_mul(dmin, dx), exact_mul(dmax, dx), bi);
        py = exact_lerp(exact_mul(dmin, dy), exact_mul(dmax, dy), bi);
        pz = exact_lerp(exact_mul(dmin, dz), exact_mul(dmax, dz), bi);
    }

    const char *maskb = reinterpret_cast<const char *>(a.mask_planes + (long long)b * a.mask_batch_stride);
    const unsigned plane_bytes = (unsigned)(a.H * a.W) << 2;       // 3 P planes stay below 2^32 bytes (checked on the host)
    const float uniform_w = a.uniform_part_weight ? 1.0f / (float)P : 0.0f;
    uint32_t bits = 0;
    int label = -1;
    float best = -1.0f, second = -1.0f;
    for (int k = 0; k < P; ++k) {
        float F[13], Cn[12], lx, ly, lz, cx, cy, cz;
        load_frames(l_parts, l_canon, k, F, Cn);
        part_point(F, Cn, px, py, pz, lx, ly, lz, cx, cy, cz);
        if (!ENARF_POINT_IN_PART(lx, ly, lz, cx, cy, cz)) continue;
        bits |= 1u << k;
        float w = uniform_w;
        if (!a.uniform_part_weight) w = part_probability(maskb, k, plane_bytes, cx, cy, cz, a.H, a.W, a.clamp_mask);
        if (w > best) {                    // strictly: the lowest index wins a tie
            second = best;
            best = w;
            label = k;
        } else {
            second = fmaxf(second, w);
        }
    }
    const size_t o = (size_t)b * a.M + i;
    a.label[o] = label;
    a.top[o] = label >= 0 ? best : 0.0f;
    a.second[o] = second;
    if (a.valid_bits) a.valid_bits[o] = bits;
}

__global__ void __launch_bounds__(kBlock) seg_composite_kernel(const enarf_seg_composite_args a) {
    const int lane = lane_id();
    const long long rid = (long long)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);      // b * n + ray
    if (rid >= (long long)a.B * a.n) return;                                                  // wave-uniform
    const int Nf = a.Nf, P = a.P;
    const int32_t *lab = a.labels + rid * Nf;
    const float *wgt = a.fine_weights + rid * (Nf - 1);
    int l[2];
    float w[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int e = 64 * s + lane;
        const bool in = e < Nf - 1;
        const int li = in ? lab[e] : -1;
        l[s] = (li >= 0 && li < P) ? li : -1;
        w[s] = (in && l[s] >= 0) ? wgt[e] : 0.0f;
    }
    float c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float t = 0.0f;
#pragma unroll
        for (int s = 0; s < 2; ++s) t += (l[s] >= 0) ? w[s] * a.palette[3 * l[s] + ch] : 0.0f;
        c[ch] = wave_sum(t);
    }
    // per-part masses: peel the distinct labels of the wave one at a time
    bool pend[2] = {l[0] >= 0, l[1] >= 0};
    float best = 0.0f;
    int best_k = -1;
    while (true) {
        const uint64_t b0 = __ballot(pend[0]), b1 = __ballot(pend[1]);
        if ((b0 | b1) == 0) break;
        const int k = b0 ? __shfl(l[0], __builtin_ctzll(b0)) : __shfl(l[1], __builtin_ctzll(b1));
        float t = 0.0f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bool hit = pend[s] && l[s] == k;
            t += hit ? w[s] : 0.0f;
            pend[s] = pend[s] && !hit;
        }
        const float m = wave_sum(t);
        if (m > best || (m == best && m > 0.0f && k < best_k)) { best = m; best_k = k; }
    }
    if (lane == 0) {
        const long long b = rid / a.n, ray = rid - b * a.n;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.color[(b * 3 + ch) * a.n + ray] = c[ch];
        a.part_mass[rid] = best;
        a.part_map[rid] = best_k;
    }
}

}  // namespace

extern "C" {

int enarf_seg_abi_version(void) { return ENARF_SEG_ABI_VERSION; }

const char *enarf_seg_last_error(void) { return enarf::host::last_error(); }

int enarf_seg_labels(const enarf_seg_label_args *args, void *stream) {
    const char *who = "enarf_seg_labels";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_seg_label_args &a = *args;
    if (const int e = enarf::host::check_part_planes(who, a.P, kMaxParts, a.H, a.W)) return e;
    if (a.B < 0 || a.B > 65535) return enarf::host::fail(ENARF_ERR_ARG, "%s: batch %d outside [0, 65535]", who, a.B);
    if (a.M < 0 || a.M / kBlock + 1 >= (1LL << 31)) return enarf::host::fail(ENARF_ERR_ARG, "%s: %lld points a image", who, (long long)a.M);
    if (a.mask_batch_stride < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: negative mask batch stride", who);
    if (!a.points) {
        if (a.n < 0 || a.Nf < 1 || (long long)a.n * a.Nf != a.M)
            return enarf::host::fail(ENARF_ERR_ARG, "%s: ray mode takes M = n Nf, got M %lld, n %d, Nf %d", who, (long long)a.M, a.n, a.Nf);
    } else if (a.point_batch_stride < 0 || a.point_stride < 0 || a.comp_stride < 0) {
        return enarf::host::fail(ENARF_ERR_ARG, "%s: negative point strides", who);
    }
    if (a.B == 0 || a.M == 0) return 0;
    if (!a.points && (!a.image_coord || !a.inv_intrinsics || !a.depth_min || !a.depth_max || !a.bins))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: ray mode needs image_coord, inv_intrinsics, depth_min, depth_max and bins", who);
    if (!a.parts || !a.canonical_pose || (!a.mask_planes && !a.uniform_part_weight) || !a.label || !a.top || !a.second)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null parts, canonical_pose, mask_planes, label, top or second", who);
    const dim3 grid((unsigned)((a.M + kBlock - 1) / kBlock), (unsigned)a.B);
    hipLaunchKernelGGL(seg_label_kernel, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_seg_labels: seg_label_kernel");
}

int enarf_seg_composite(const enarf_seg_composite_args *args, void *stream) {
    const char *who = "enarf_seg_composite";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_seg_composite_args &a = *args;
    if (a.P < 1 || a.P > kMaxParts) return enarf::host::fail(ENARF_ERR_ARG, "%s: %d parts outside [1, %d]", who, a.P, kMaxParts);
    if (a.Nf < 2 || a.Nf > ENARF_SEG_MAX_SAMPLES)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: Nf %d outside [2, %d]", who, a.Nf, ENARF_SEG_MAX_SAMPLES);
    if (a.B < 0 || a.n < 0 || (long long)a.B * a.n >= (1LL << 31) - 4)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: %d x %d rays outside [0, 2^31 - 4)", who, a.B, a.n);
    const long long rays = (long long)a.B * a.n;
    if (rays == 0) return 0;
    if (!a.labels || !a.fine_weights || !a.palette || !a.color || !a.part_mass || !a.part_map)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null labels, fine_weights, palette, color, part_mass or part_map", who);
    const long long blocks = (rays + kBlock / kWave - 1) / (kBlock / kWave);
    hipLaunchKernelGGL(seg_composite_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_seg_composite: seg_composite_kernel");
}

}  // extern "C"
