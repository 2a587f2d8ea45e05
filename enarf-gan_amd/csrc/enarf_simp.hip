// enarf_simp.hip - libenarf_simp.so: mesh simplification by uniform-grid vertex clustering with quadric placement (gfx950 /
// CDNA4 only, wave64). The contract is in include/enarf_simp.h.
//
//   simp_key_kernel      one lane per vertex: 12 bytes in, the 64-bit cell key out.
//   simp_corner_kernel   one lane per triangle: three gathers of vertex_cluster, the rotated cluster triple (or the
//                        sentinel of a dropped triangle) and the triangle's three incidence slots.
//   simp_place_kernel    <quadric or mean> one wavefront per cluster: the lanes stride the cluster's vertex segment and,
//                        for the quadric, its incidence segment, each with its partial mean, A (6) and b (3) in fp64
//                        registers; the 64 partials are folded by shuffles in a fixed order; lane 0 solves the 3 x 3
//                        system by Cholesky, clamps to the cell and stores. Segments are longer than a wavefront at every
//                        useful cell size: one lane per cluster would serialise hundreds of dependent gathers.
// The sums are store-then-sum-per-destination: the sorts between the kernels (the caller's) bring everything that adds to
// one cluster into one segment, so no atomics are needed and every sum has one order. Everything is fp64 from the stored
// inputs with FMA contraction off, so the float64 restatement of the contract (tests/simp_reference.py) differs only by
// the order of the sums.
#include "enarf_simp.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr long long kMaxCount = 1LL << 31;
constexpr long long kAxisMask = (1LL << ENARF_SIMP_AXIS_BITS) - 1;

__global__ void __launch_bounds__(kBlock) simp_key_kernel(const enarf_simp_keys_args a) {
#pragma clang fp contract(off)
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v >= a.V) return;
    const double h = (double)a.cell;
    long long key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = floor(((double)a.vertices[3 * v + k] - (double)a.origin[k]) / h);
        const long long ci = c > 0.0 ? (c < (double)kAxisMask ? (long long)c : kAxisMask) : 0;     // a NaN gives 0
        key = (key << ENARF_SIMP_AXIS_BITS) | ci;
    }
    a.keys[v] = key;
}

__global__ void __launch_bounds__(kBlock) simp_corner_kernel(const enarf_simp_corners_args a) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= a.T) return;
    int c[3] = {-1, -1, -1};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long v = a.triangles[3 * t + k];
        ok = ok && v >= 0 && v < a.V;
        if (ok) c[k] = a.vertex_cluster[v];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && c[k] >= 0 && c[k] < a.C;
    int inc[3], tri[3] = {-1, -1, -1};
    inc[0] = ok ? c[0] : ENARF_SIMP_NO_CLUSTER;
    inc[1] = (ok && c[1] != c[0]) ? c[1] : ENARF_SIMP_NO_CLUSTER;
    inc[2] = (ok && c[2] != c[0] && c[2] != c[1]) ? c[2] : ENARF_SIMP_NO_CLUSTER;
    if (ok && c[0] != c[1] && c[1] != c[2] && c[0] != c[2]) {
        // rotate the smallest cluster to the front: the three differ, so the smallest is unique
        if (c[0] < c[1] && c[0] < c[2]) {
            tri[0] = c[0]; tri[1] = c[1]; tri[2] = c[2];
        } else if (c[1] < c[2]) {
            tri[0] = c[1]; tri[1] = c[2]; tri[2] = c[0];
        } else {
            tri[0] = c[2]; tri[1] = c[0]; tri[2] = c[1];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.triples[3 * t + k] = tri[k];
        a.incidence[3 * t + k] = inc[k];
    }
}

// the 64 lanes' partial sums folded in a fixed order: lane l += lane l + 32, then + 16, 8, 4, 2, 1; lane 0 has the total
__device__ __forceinline__ double wave_fold(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ long long clamp_ll(long long x, long long lo, long long hi) { return x < lo ? lo : (x > hi ? hi : x); }

template <bool QUADRIC>
__global__ void __launch_bounds__(kBlock) simp_place_kernel(const enarf_simp_place_args a) {
#pragma clang fp contract(off)
    const long long cluster = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (cluster >= a.C) return;                                   // wave-uniform
    const int lane = threadIdx.x & 63;
    const long long key = a.keys[cluster];
    const double h = (double)a.cell;
    double lo[3];
    lo[0] = (double)a.origin[0] + (double)((key >> (2 * ENARF_SIMP_AXIS_BITS)) & kAxisMask) * h;
    lo[1] = (double)a.origin[1] + (double)((key >> ENARF_SIMP_AXIS_BITS) & kAxisMask) * h;
    lo[2] = (double)a.origin[2] + (double)(key & kAxisMask) * h;

    const long long v0 = clamp_ll(a.vertex_start[cluster], 0, a.V), v1 = clamp_ll(a.vertex_start[cluster + 1], v0, a.V);
    double m[3] = {0.0, 0.0, 0.0};
    for (long long i = v0 + lane; i < v1; i += 64) {
        const long long v = a.vertex_order[i];
        if (v < 0 || v >= a.V) continue;
        const float *q = a.vertices + 3 * v;
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] += (double)q[k] - lo[k];
    }
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};       // A: xx, xy, xz, yy, yz, zz
    if (QUADRIC) {
        const long long N = 3 * a.T;
        const long long s0 = clamp_ll(a.slot_start[cluster], 0, N), s1 = clamp_ll(a.slot_start[cluster + 1], s0, N);
        for (long long i = s0 + lane; i < s1; i += 64) {
            const long long s = a.slot_order[i];
            if (s < 0 || s >= N) continue;
            const long long t = s / 3;
            double p[3][3];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long v = a.triangles[3 * t + c];
                ok = ok && v >= 0 && v < a.V;
                const float *q = a.vertices + 3 * (ok ? v : 0);
#pragma unroll
                for (int k = 0; k < 3; ++k) p[c][k] = (double)q[k] - lo[k];
            }
            if (!ok) continue;
            double e1[3], e2[3], n[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                e1[k] = p[1][k] - p[0][k];
                e2[k] = p[2][k] - p[0][k];
            }
            n[0] = e1[1] * e2[2] - e1[2] * e2[1];
            n[1] = e1[2] * e2[0] - e1[0] * e2[2];
            n[2] = e1[0] * e2[1] - e1[1] * e2[0];
            const double d = (n[0] * p[0][0] + n[1] * p[0][1]) + n[2] * p[0][2];
            A[0] += n[0] * n[0]; A[1] += n[0] * n[1]; A[2] += n[0] * n[2];
            A[3] += n[1] * n[1]; A[4] += n[1] * n[2]; A[5] += n[2] * n[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k] += n[k] * d;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = wave_fold(m[k]);
    if (QUADRIC) {
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = wave_fold(A[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = wave_fold(b[k]);
    }
    if (lane != 0) return;
    const double count = (double)(v1 - v0);
    double x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = m[k] = m[k] / count;
    if (QUADRIC) {
        const double trace = (A[0] + A[3]) + A[5];
        if (trace > 0.0) {
            const double lam = a.reg * trace;
            const double r0 = b[0] + lam * m[0], r1 = b[1] + lam * m[1], r2 = b[2] + lam * m[2];
            // Cholesky of M = A + lam I = L L^T
            const double l00 = sqrt(A[0] + lam);
            const double l10 = A[1] / l00, l20 = A[2] / l00;
            const double l11 = sqrt((A[3] + lam) - l10 * l10);
            const double l21 = (A[4] - l20 * l10) / l11;
            const double l22 = sqrt(((A[5] + lam) - l20 * l20) - l21 * l21);
            const double y0 = r0 / l00;
            const double y1 = (r1 - l10 * y0) / l11;
            const double y2 = ((r2 - l20 * y0) - l21 * y1) / l22;
            x[2] = y2 / l22;
            x[1] = (y1 - l21 * x[2]) / l11;
            x[0] = ((y0 - l10 * x[1]) - l20 * x[2]) / l00;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = x[k] < 0.0 ? 0.0 : (x[k] > h ? h : x[k]);
        a.out[3 * cluster + k] = (float)(c + lo[k]);
    }
}

unsigned blocks(long long count, int per_block) { return (unsigned)((count + per_block - 1) / per_block); }

}  // namespace

extern "C" {

int enarf_simp_abi_version(void) { return ENARF_SIMP_ABI_VERSION; }

const char *enarf_simp_last_error(void) { return enarf::host::last_error(); }

int enarf_simp_keys(const enarf_simp_keys_args *args, void *stream) {
    const char *who = "enarf_simp_keys";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_simp_keys_args &a = *args;
    if (a.V < 0 || a.V >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld outside [0, 2^31)", who, (long long)a.V);
    if (!(a.cell > 0.0f) || !isfinite(a.cell))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the cell size must be finite and > 0, got %g", who, (double)a.cell);
    for (int k = 0; k < 3; ++k)
        if (!isfinite(a.origin[k])) return enarf::host::fail(ENARF_ERR_ARG, "%s: origin[%d] is not finite", who, k);
    if (a.V == 0) return 0;
    if (!a.vertices || !a.keys) return enarf::host::fail(ENARF_ERR_ARG, "%s: null vertices or keys", who);
    hipLaunchKernelGGL(simp_key_kernel, dim3(blocks(a.V, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_simp_keys: simp_key_kernel");
}

int enarf_simp_corners(const enarf_simp_corners_args *args, void *stream) {
    const char *who = "enarf_simp_corners";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_simp_corners_args &a = *args;
    if (a.V < 0 || a.V >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld outside [0, 2^31)", who, (long long)a.V);
    if (a.T < 0 || 3 * (long long)a.T >= kMaxCount)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: T = %lld: 3 T must lie in [0, 2^31)", who, (long long)a.T);
    if (a.C < 0 || a.C > a.V) return enarf::host::fail(ENARF_ERR_ARG, "%s: C = %d outside [0, V = %lld]", who, a.C, (long long)a.V);
    if (a.T == 0) return 0;
    if (!a.triangles || !a.triples || !a.incidence || (a.V > 0 && !a.vertex_cluster))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null triangles, vertex_cluster, triples or incidence", who);
    hipLaunchKernelGGL(simp_corner_kernel, dim3(blocks(a.T, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_simp_corners: simp_corner_kernel");
}

int enarf_simp_place(const enarf_simp_place_args *args, void *stream) {
    const char *who = "enarf_simp_place";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_simp_place_args &a = *args;
    if (a.V < 0 || a.V >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld outside [0, 2^31)", who, (long long)a.V);
    if (a.T < 0 || 3 * (long long)a.T >= kMaxCount)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: T = %lld: 3 T must lie in [0, 2^31)", who, (long long)a.T);
    if (a.C < 0 || a.C > a.V) return enarf::host::fail(ENARF_ERR_ARG, "%s: C = %d outside [0, V = %lld]", who, a.C, (long long)a.V);
    if (!(a.cell > 0.0f) || !isfinite(a.cell))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the cell size must be finite and > 0, got %g", who, (double)a.cell);
    for (int k = 0; k < 3; ++k)
        if (!isfinite(a.origin[k])) return enarf::host::fail(ENARF_ERR_ARG, "%s: origin[%d] is not finite", who, k);
    if (a.quadric && (!(a.reg > 0.0) || !isfinite(a.reg)))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: reg must be finite and > 0, got %g", who, a.reg);
    if (a.C == 0) return 0;
    if (!a.vertices || !a.keys || !a.vertex_order || !a.vertex_start || !a.out)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null vertices, keys, vertex_order, vertex_start or out", who);
    if (a.quadric && (!a.slot_start || (a.T > 0 && (!a.triangles || !a.slot_order))))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the quadric placement takes triangles, slot_order and slot_start", who);
    const dim3 grid(blocks(a.C, kWavesPerBlock)), block(kBlock);
    if (a.quadric)
        hipLaunchKernelGGL(simp_place_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(simp_place_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_simp_place: simp_place_kernel");
}

}  // extern "C"
