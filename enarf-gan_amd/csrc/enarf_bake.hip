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
//                         light and Phong terms of enarf_paint.hip.
// No atomics, no LDS, no workspace. Everything is fp64 from the stored inputs with FMA contraction off, so the float64
// restatement of the contract (tests/bake_reference.py) is matched to the rounding of the stored values.
#include "enarf_bake.h"
#include "enarf_device.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

using enarf::level;

constexpr int kBlock = 256;
constexpr int kMaxR = ENARF_BAKE_MAX_SIZE;
constexpr long long kMaxCount = 1LL << 31;

struct Layout {
    int c, n;                                   // cell size in texels, cells a row
};

// the smallest n >= 1 with 2 n n >= T
long long cells_needed(long long T) {
    long long n = (long long)sqrt((double)T / 2.0);
    if (n < 1) n = 1;
    while (2 * n * n < T) ++n;
    while (n > 1 && 2 * (n - 1) * (n - 1) >= T) --n;
    return n;
}

// 0 and the layout, or the failure to return
int find_layout(const char *who, long long T, int A, Layout *out) {
    if (A < ENARF_BAKE_MIN_ATLAS || A > ENARF_BAKE_MAX_ATLAS)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: atlas size %d outside [%d, %d]", who, A, ENARF_BAKE_MIN_ATLAS,
                                 ENARF_BAKE_MAX_ATLAS);
    if (T < 0 || T >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: T = %lld outside [0, 2^31)", who, T);
    const long long need = cells_needed(T);
    const long long c = A / need;
    if (c < ENARF_BAKE_MIN_CELL)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: %lld triangles need %lld cells of %d texels a row: an atlas of "
                                 "at least %lld texels a side, got %d", who, T, need, ENARF_BAKE_MIN_CELL,
                                 need * ENARF_BAKE_MIN_CELL, A);
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

// c = -N . p / max(|p|, 1e-6) with N = n / max(|n|, 1e-6)
__device__ __forceinline__ double light_term(const double n[3], const double p[3]) {
#pragma clang fp contract(off)
    const double dn = fmax(sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]), 1e-6);
    const double dp = fmax(sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]), 1e-6);
    const double N0 = n[0] / dn, N1 = n[1] / dn, N2 = n[2] / dn;
    return -((N0 * p[0] + N1 * p[1]) + N2 * p[2]) / dp;
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

// one axis of the bilinear tap: the two clamped texel indices and their weights; a NaN coordinate clamps to texel 0
__device__ __forceinline__ void tap_axis(double u, int A, int &i0, int &i1, double &w0, double &w1) {
#pragma clang fp contract(off)
    const double s = u - 0.5, f = floor(s), top = (double)(A - 1);
    w1 = s - f;
    w0 = 1.0 - w1;
    i0 = (int)fmin(fmax(f, 0.0), top);
    i1 = (int)fmin(fmax(f + 1.0, 0.0), top);
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
        int x0, x1, y0, y1;
        double wx0, wx1, wy0, wy1;
        tap_axis(u, a.A, x0, x1, wx0, wx1);
        tap_axis(w, a.A, y0, y1, wy0, wy1);
        const double w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
        const long long e00 = (long long)y0 * a.A + x0, e01 = (long long)y0 * a.A + x1;
        const long long e10 = (long long)y1 * a.A + x0, e11 = (long long)y1 * a.A + x1;
        if (a.texture) {
            const uint32_t *tex = reinterpret_cast<const uint32_t *>(a.texture);
            const uint32_t t00 = tex[e00], t01 = tex[e01], t10 = tex[e10], t11 = tex[e11];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int s = 8 * ch;
                texel[ch] = ((w00 * ((double)((t00 >> s) & 255u) / 255.0) + w01 * ((double)((t01 >> s) & 255u) / 255.0)) +
                             w10 * ((double)((t10 >> s) & 255u) / 255.0)) + w11 * ((double)((t11 >> s) & 255u) / 255.0);
            }
        } else {
            const float *tex = a.texture_f32;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                texel[ch] = ((w00 * (double)tex[3 * e00 + ch] + w01 * (double)tex[3 * e01 + ch]) +
                             w10 * (double)tex[3 * e10 + ch]) + w11 * (double)tex[3 * e11 + ch];
        }
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

unsigned blocks(long long count) { return (unsigned)((count + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int enarf_bake_abi_version(void) { return ENARF_BAKE_ABI_VERSION; }

const char *enarf_bake_last_error(void) { return enarf::host::last_error(); }

int enarf_bake_layout(int64_t T, int32_t A, int32_t *cell, int32_t *cells_per_row) {
    Layout lay;
    if (const int rc = find_layout("enarf_bake_layout", (long long)T, A, &lay)) return rc;
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
    if (const int rc = find_layout(who, (long long)a.T, a.A, &lay)) return rc;
    if (a.row0 < 0 || a.rows < 1 || (long long)a.row0 + a.rows > a.A)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: rows [%d, %d + %d) outside the atlas of %d rows", who, a.row0, a.row0,
                                 a.rows, a.A);
    if (!a.points || !a.texel_face || (a.V > 0 && !a.vertices) || (a.T > 0 && !a.triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null points, texel_face, vertices or triangles", who);
    hipLaunchKernelGGL(bake_points_kernel, dim3(blocks((long long)a.rows * a.A)), dim3(kBlock), 0,
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
    hipLaunchKernelGGL(bake_resolve_kernel, dim3(blocks(a.count)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_bake_resolve: bake_resolve_kernel");
}

int enarf_bake_shade(const enarf_bake_shade_args *args, void *stream) {
    const char *who = "enarf_bake_shade";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_bake_shade_args &a = *args;
    if (a.R < 1 || a.R > kMaxR) return enarf::host::fail(ENARF_ERR_ARG, "%s: render size %d outside [1, %d]", who, a.R, kMaxR);
    if (a.V < 0 || a.V >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld outside [0, 2^31)", who, (long long)a.V);
    Layout lay;
    if (const int rc = find_layout(who, (long long)a.T, a.A, &lay)) return rc;
    if ((a.texture != nullptr) == (a.texture_f32 != nullptr))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: exactly one of texture and texture_f32 must be given", who);
    if (reinterpret_cast<uintptr_t>(a.texture) & 3u)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the texture is read one 32-bit texel at a time: 4-byte alignment", who);
    if (!a.pix_to_face || !a.bary || !a.normals || !a.image || (a.V > 0 && !a.vertices) || (a.T > 0 && !a.triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null pix_to_face, bary, normals, image, vertices or triangles", who);
    hipLaunchKernelGGL(bake_shade_kernel, dim3(blocks((long long)a.R * a.R)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a, lay);
    return enarf::host::check_launch("enarf_bake_shade: bake_shade_kernel");
}

}  // extern "C"
