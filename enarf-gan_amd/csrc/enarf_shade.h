// enarf_shade.h - what the kernels that shade a rasterised mesh share (paint_shade_kernel in enarf_paint.hip,
// bake_shade_kernel in enarf_bake.hip, nmap_shade_kernel in enarf_nmap.hip) and what the kernels that fill the atlas share
// with them (bake_points_kernel, nmap_encode_kernel): the corners of a triangle, the atlas layout of include/enarf_bake.h
// with the corners a fragment's uv is mixed from, the four-texel tap of an RGBA8 or fp32 atlas, and the light and Phong
// terms. One definition, so a texel means the same to the library that bakes it and to every library that reads it.
// Device functions and small host functions only; each library keeps its own kernels. Everything is fp64 with FMA
// contraction off, every sum parenthesised as the float64 referees (tests/paint_reference.py, bake_reference.py,
// nmap_reference.py) restate it.
// Included after a public header (they define ENARF_ERR_ARG and ENARF_ERR_UNSUPPORTED).
#pragma once
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

// The atlas layout as a kernel takes it, by value. It sits beside the kernels, in the anonymous namespace of the one
// translation unit a library is, so that a kernel's symbol names no type with external linkage.
struct Layout {
    int c, n;                                   // cell size in texels, cells a row
};

}  // namespace

namespace enarf {
namespace shade {

constexpr long long kMaxCount = 1LL << 31;      // V and T stay below it

inline unsigned blocks(long long count, int per_block) { return (unsigned)((count + per_block - 1) / per_block); }

// the three vertex indices of triangle t; false when one of them is outside [0, V)
__device__ __forceinline__ bool corners_of(const int64_t *triangles, long long t, long long V, long long v[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = triangles[3 * t + k];
        ok = ok && v[k] >= 0 && v[k] < V;
    }
    return ok;
}

__device__ __forceinline__ double length3(const double a[3]) {
#pragma clang fp contract(off)
    return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
}

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double out[3]) {
#pragma clang fp contract(off)
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- the light and Phong terms

// max(|a|, 1e-6): what a normal and a view vector are divided by
__device__ __forceinline__ double floored_length(const double a[3]) { return fmax(length3(a), 1e-6); }

// c = -N . p / dp for a unit N and dp = max(|p|, 1e-6)
__device__ __forceinline__ double facing(const double N[3], const double p[3], double dp) {
#pragma clang fp contract(off)
    return -((N[0] * p[0] + N[1] * p[1]) + N[2] * p[2]) / dp;
}

// c = -N . p / max(|p|, 1e-6) with N = n / max(|n|, 1e-6)
__device__ __forceinline__ double light_term(const double n[3], const double p[3]) {
#pragma clang fp contract(off)
    const double dn = floored_length(n), dp = floored_length(p);
    const double N[3] = {n[0] / dn, n[1] / dn, n[2] / dn};
    return facing(N, p, dp);
}

// texel (0.5 + 0.3 max(c, 0)) + 0.2 max(2 c c - 1, 0)^64
__device__ __forceinline__ void phong(const double texel[3], double c, double out[3]) {
#pragma clang fp contract(off)
    double spec = 0.0;
    if (c > 0.0) {
        spec = fmax(2.0 * c * c - 1.0, 0.0);
#pragma unroll
        for (int i = 0; i < 6; ++i) spec *= spec;                          // ^64
    }
    const double k = 0.5 + 0.3 * (c > 0.0 ? c : 0.0), s = 0.2 * spec;        // a NaN light term counts as 0
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = texel[a] * k + s;
}

// ---- the atlas layout of include/enarf_bake.h

// a library's own limits, from its public header
struct AtlasLimits {
    int min_atlas, max_atlas, min_cell;
};

// the smallest n >= 1 with 2 n n >= T
inline long long cells_needed(long long T) {
    long long n = (long long)sqrt((double)T / 2.0);
    if (n < 1) n = 1;
    while (2 * n * n < T) ++n;
    while (n > 1 && 2 * (n - 1) * (n - 1) >= T) --n;
    return n;
}

// 0 and the layout, or the failure to return
inline int find_layout(const char *who, long long T, int A, const AtlasLimits &lim, Layout *out) {
    if (A < lim.min_atlas || A > lim.max_atlas)
        return host::fail(ENARF_ERR_ARG, "%s: atlas size %d outside [%d, %d]", who, A, lim.min_atlas, lim.max_atlas);
    if (T < 0 || T >= kMaxCount) return host::fail(ENARF_ERR_ARG, "%s: T = %lld outside [0, 2^31)", who, T);
    const long long need = cells_needed(T);
    const long long c = A / need;
    if (c < lim.min_cell)
        return host::fail(ENARF_ERR_UNSUPPORTED, "%s: %lld triangles need %lld cells of %d texels a row: an atlas of "
                          "at least %lld texels a side, got %d", who, T, need, lim.min_cell, need * lim.min_cell, A);
    out->c = (int)c;
    out->n = A / (int)c;
    return 0;
}

// the local corner k of half h, in texels
__device__ __forceinline__ void corner(int c, int h, int k, int &x, int &y) {
    if (h == 0) {
        x = k == 1 ? c - 3 : 1;
        y = k == 2 ? c - 3 : 1;
    } else {
        x = k == 1 ? 3 : c - 1;
        y = k == 2 ? 3 : c - 1;
    }
}

// ---- the bilinear tap

// one axis of the tap: the two clamped texel indices and their weights; a NaN coordinate clamps to texel 0
__device__ __forceinline__ void tap_axis(double u, int A, int &i0, int &i1, double &w0, double &w1) {
#pragma clang fp contract(off)
    const double s = u - 0.5, f = floor(s), top = (double)(A - 1);
    w1 = s - f;
    w0 = 1.0 - w1;
    i0 = (int)fmin(fmax(f, 0.0), top);
    i1 = (int)fmin(fmax(f + 1.0, 0.0), top);
}

struct Tap {
    long long e[4];                             // y0 x0, y0 x1, y1 x0, y1 x1
    double w[4];
};

// the four texels around (u, w) in an atlas of A texels a side, and their weights
__device__ __forceinline__ Tap tap_at(double u, double w, int A) {
#pragma clang fp contract(off)
    int x0, x1, y0, y1;
    double wx0, wx1, wy0, wy1;
    tap_axis(u, A, x0, x1, wx0, wx1);
    tap_axis(w, A, y0, y1, wy0, wy1);
    Tap tp;
    tp.w[0] = wx0 * wy0, tp.w[1] = wx1 * wy0, tp.w[2] = wx0 * wy1, tp.w[3] = wx1 * wy1;
    tp.e[0] = (long long)y0 * A + x0, tp.e[1] = (long long)y0 * A + x1;
    tp.e[2] = (long long)y1 * A + x0, tp.e[3] = (long long)y1 * A + x1;
    return tp;
}

// the tap of an RGBA8 texture; scale and shift decode a byte: (scale byte) / 255 - shift (1 and 0 for a colour, which
// is byte / 255 exactly; 2 and 1 for a normal)
__device__ __forceinline__ void tap_rgba8(const uint8_t *texture, const Tap &tp, double scale, double shift, double out[3]) {
#pragma clang fp contract(off)
    const uint32_t *tex = reinterpret_cast<const uint32_t *>(texture);
    const uint32_t t0 = tex[tp.e[0]], t1 = tex[tp.e[1]], t2 = tex[tp.e[2]], t3 = tex[tp.e[3]];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int s = 8 * ch;
        const double d0 = (scale * (double)((t0 >> s) & 255u)) / 255.0 - shift;
        const double d1 = (scale * (double)((t1 >> s) & 255u)) / 255.0 - shift;
        const double d2 = (scale * (double)((t2 >> s) & 255u)) / 255.0 - shift;
        const double d3 = (scale * (double)((t3 >> s) & 255u)) / 255.0 - shift;
        out[ch] = ((tp.w[0] * d0 + tp.w[1] * d1) + tp.w[2] * d2) + tp.w[3] * d3;
    }
}

__device__ __forceinline__ void tap_f32(const float *tex, const Tap &tp, double out[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        out[ch] = ((tp.w[0] * (double)tex[3 * tp.e[0] + ch] + tp.w[1] * (double)tex[3 * tp.e[1] + ch]) +
                   tp.w[2] * (double)tex[3 * tp.e[2] + ch]) + tp.w[3] * (double)tex[3 * tp.e[3] + ch];
}

}  // namespace shade
}  // namespace enarf
