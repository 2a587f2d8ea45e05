// enarf_bake.hip - libenarf_bake.so: the texture atlas of an extracted mesh (gfx950 / CDNA4 only, wave64). The contract,
// the atlas layout included, is in include/enarf_bake.h.
//
//   bake_points_kernel    one lane per texel of a band of atlas rows: the owner of the texel from the layout (integer
//                         arithmetic on the texel's column and row, nothing stored), the affine coordinates of the texel
//                         centre in the owner's corner frame, the surface point. Consecutive lanes write consecutive
//                         floats of each of the three point planes and of texel_face: every store is a full line.
//   bake_resolve_kernel   one lane per texel: the colour planes (or the label and its palette entry) to one RGBA8 dword,
//                         and optionally the three floats of the unquantised texture.
//   bake_shade_kernel     one lane per pixel, one launch per image: the fragment's uv from the layout and the stored b',
//                         four texel loads (one dword each for RGBA8), the bilinear mix as the albedo, and the point,
//                         light and Phong terms of paint_shade_kernel.
// No atomics, no LDS, no workspace. Everything is fp64 from the stored inputs with FMA contraction off, so the float64
// restatement of the contract (tests/bake_reference.py) is matched to the rounding of the stored values. The layout, the
// corners of a cell, the tap and the light and Phong terms are enarf_shade.h's, shared with enarf_paint.hip and
// enarf_nmap.hip; the point of a texel and the resolve arithmetic are this file's own.
#include "enarf_bake.h"
#include "enarf_device.h"
#include "enarf_host.h"
#include "enarf_shade.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

using enarf::level;
using namespace enarf::shade;

constexpr int kBlock = 256;
constexpr int kMaxR = ENARF_BAKE_MAX_SIZE;
constexpr AtlasLimits kLimits = {ENARF_BAKE_MIN_ATLAS, ENARF_BAKE_MAX_ATLAS, ENARF_BAKE_MIN_CELL};

__global__ void __launch_bounds__(kBlock) bake_points_kernel(const enarf_bake_points_args a, const Layout lay) {
#pragma clang fp contract(off)
    const long long count = (long long)a.rows * a.A;
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= count) return;
    const int x = (int)(e % a.A), y = a.row0 + (int)(e / a.A);
    const int c = lay.c, n = lay.n;
    const int cx = x / c, cy = y / c;
    long long t = -1, v[3] = {0, 0, 0};
    int i = 0, j = 0, h = 0;
    if (cx < n && cy < n) {
        i = x - cx * c;
        j = y - cy * c;
        h = (i + j + 1 <= c) ? 0 : 1;
        t = 2LL * ((long long)cy * n + cx) + h;
        if (t >= a.T || !corners_of(a.triangles, t, a.V, v)) t = -1;
    }
    double p[3] = {0.0, 0.0, 0.0};
    if (t >= 0) {
        const double L = (double)(c - 4), u = (double)i + 0.5, w = (double)j + 0.5;
        const double a1 = (h == 0 ? u - 1.0 : (double)(c - 1) - u) / L;
        const double a2 = (h == 0 ? w - 1.0 : (double)(c - 1) - w) / L;
        const double a0 = (1.0 - a1) - a2;
        const float *q0 = a.vertices + 3 * v[0], *q1 = a.vertices + 3 * v[1], *q2 = a.vertices + 3 * v[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = (a0 * (double)q0[k] + a1 * (double)q1[k]) + a2 * (double)q2[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.points[k * count + e] = (float)p[k];
    a.texel_face[e] = (int)t;
}

__global__ void __launch_bounds__(kBlock) bake_resolve_kernel(const enarf_bake_resolve_args a) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= a.count) return;
    const bool owned = a.texel_face[e] >= 0;
    double v[3];
    if (!owned) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = (double)a.fill[ch];
    } else if (a.colors) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double x = (double)a.colors[ch * a.count + e];
            v[ch] = a.unit ? x : (x + 1.0) / 2.0;
        }
    } else {
        const int l = a.labels[e];
        const bool known = l >= 0 && l < a.P;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = (double)(known ? a.palette[3 * l + ch] : a.neutral[ch]);
    }
    const uint32_t rgba = (uint32_t)level(v[0]) | ((uint32_t)level(v[1]) << 8) | ((uint32_t)level(v[2]) << 16) |
                          (owned ? 0xFF000000u : 0u);
    reinterpret_cast<uint32_t *>(a.texture)[e] = rgba;
    if (a.texture_f32) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.texture_f32[3 * e + ch] = (float)v[ch];
    }
}

__global__ void __launch_bounds__(kBlock) bake_shade_kernel(const enarf_bake_shade_args a, const Layout lay) {
#pragma clang fp contract(off)
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (long long)a.R * a.R) return;
    const long long f = a.pix_to_face[p];
    long long v[3] = {0, 0, 0};
    const bool drawn = f >= 0 && f < a.T && corners_of(a.triangles, f, a.V, v);
    double texel[3], shaded[3];
    if (!drawn) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) texel[ch] = shaded[ch] = (double)a.background[ch];
    } else {
        const float b0 = a.bary[3 * p], b1 = a.bary[3 * p + 1], b2 = a.bary[3 * p + 2];
        const int c = lay.c, n = lay.n, h = (int)(f & 1);
        const long long q = f >> 1;
        const int ox = (int)(q % n) * c, oy = (int)(q / n) * c;
        int ux[3], uy[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            corner(c, h, k, ux[k], uy[k]);
            ux[k] += ox;
            uy[k] += oy;
        }
        const double u = ((double)b0 * (double)ux[0] + (double)b1 * (double)ux[1]) + (double)b2 * (double)ux[2];
        const double w = ((double)b0 * (double)uy[0] + (double)b1 * (double)uy[1]) + (double)b2 * (double)uy[2];
        const Tap tp = tap_at(u, w, a.A);
        if (a.texture) tap_rgba8(a.texture, tp, 1.0, 0.0, texel);
        else tap_f32(a.texture_f32, tp, texel);
        if (a.lit) {
            const float *q0 = a.vertices + 3 * v[0], *q1 = a.vertices + 3 * v[1], *q2 = a.vertices + 3 * v[2];
            double nn[3], pt[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                nn[k] = (double)a.normals[3 * p + k];
                pt[k] = ((double)b0 * (double)q0[k] + (double)b1 * (double)q1[k]) + (double)b2 * (double)q2[k];
            }
            phong(texel, light_term(nn, pt), shaded);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) shaded[ch] = texel[ch];
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (a.albedo) a.albedo[3 * p + ch] = (float)texel[ch];
        if (a.shaded) a.shaded[3 * p + ch] = (float)shaded[ch];
        a.image[3 * p + ch] = level(shaded[ch]);
    }
}

}  // namespace

extern "C" {

int enarf_bake_abi_version(void) { return ENARF_BAKE_ABI_VERSION; }

const char *enarf_bake_last_error(void) { return enarf::host::last_error(); }

int enarf_bake_layout(int64_t T, int32_t A, int32_t *cell, int32_t *cells_per_row) {
    Layout lay;
    if (const int rc = find_layout("enarf_bake_layout", (long long)T, A, kLimits, &lay)) return rc;
    if (cell) *cell = lay.c;
    if (cells_per_row) *cells_per_row = lay.n;
    return 0;
}

int enarf_bake_points(const enarf_bake_points_args *args, void *stream) {
    const char *who = "enarf_bake_points";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_bake_points_args &a = *args;
    if (a.V < 0 || a.V >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld outside [0, 2^31)", who, (long long)a.V);
    Layout lay;
    if (const int rc = find_layout(who, (long long)a.T, a.A, kLimits, &lay)) return rc;
    if (a.row0 < 0 || a.rows < 1 || (long long)a.row0 + a.rows > a.A)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: rows [%d, %d + %d) outside the atlas of %d rows", who, a.row0, a.row0,
                                 a.rows, a.A);
    if (!a.points || !a.texel_face || (a.V > 0 && !a.vertices) || (a.T > 0 && !a.triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null points, texel_face, vertices or triangles", who);
    hipLaunchKernelGGL(bake_points_kernel, dim3(blocks((long long)a.rows * a.A, kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a, lay);
    return enarf::host::check_launch("enarf_bake_points: bake_points_kernel");
}

int enarf_bake_resolve(const enarf_bake_resolve_args *args, void *stream) {
    const char *who = "enarf_bake_resolve";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_bake_resolve_args &a = *args;
    const long long most = (long long)ENARF_BAKE_MAX_ATLAS * ENARF_BAKE_MAX_ATLAS;
    if (a.count < 1 || a.count > most)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: %lld texels outside [1, %lld]", who, (long long)a.count, most);
    if ((a.colors != nullptr) == (a.labels != nullptr))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: exactly one of colors and labels must be given", who);
    if (a.labels && (!a.palette || a.P < 1))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: label mode takes a palette of P >= 1 entries, got P = %d", who, a.P);
    if (!a.texel_face || !a.texture) return enarf::host::fail(ENARF_ERR_ARG, "%s: null texel_face or texture", who);
    if (reinterpret_cast<uintptr_t>(a.texture) & 3u)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the texture is written one 32-bit texel at a time: 4-byte alignment", who);
    hipLaunchKernelGGL(bake_resolve_kernel, dim3(blocks(a.count, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_bake_resolve: bake_resolve_kernel");
}

int enarf_bake_shade(const enarf_bake_shade_args *args, void *stream) {
    const char *who = "enarf_bake_shade";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_bake_shade_args &a = *args;
    if (a.R < 1 || a.R > kMaxR) return enarf::host::fail(ENARF_ERR_ARG, "%s: render size %d outside [1, %d]", who, a.R, kMaxR);
    if (a.V < 0 || a.V >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld outside [0, 2^31)", who, (long long)a.V);
    Layout lay;
    if (const int rc = find_layout(who, (long long)a.T, a.A, kLimits, &lay)) return rc;
    if ((a.texture != nullptr) == (a.texture_f32 != nullptr))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: exactly one of texture and texture_f32 must be given", who);
    if (reinterpret_cast<uintptr_t>(a.texture) & 3u)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the texture is read one 32-bit texel at a time: 4-byte alignment", who);
    if (!a.pix_to_face || !a.bary || !a.normals || !a.image || (a.V > 0 && !a.vertices) || (a.T > 0 && !a.triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null pix_to_face, bary, normals, image, vertices or triangles", who);
    hipLaunchKernelGGL(bake_shade_kernel, dim3(blocks((long long)a.R * a.R, kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a, lay);
    return enarf::host::check_launch("enarf_bake_shade: bake_shade_kernel");
}

}  // extern "C"
