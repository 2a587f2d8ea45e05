// enarf_nmap.hip - libenarf_nmap.so: tangent-space normal maps in the texture atlas of an extracted mesh (gfx950 / CDNA4
// only, wave64). The contract, the tangent frame included, is in include/enarf_nmap.h; the atlas layout in enarf_bake.h.
//
//   nmap_encode_kernel   one lane per texel: the owner's three corners, its frame (t^, b^, n^), the vector of the texel
//                        from the three planes (consecutive lanes read consecutive floats) in that frame, one RGBA8 dword
//                        and optionally the three floats of the unquantised map.
//   nmap_shade_kernel    one lane per pixel, one launch per image: the fragment's uv from the layout and the stored b',
//                        four texel loads of the normal map and four of the albedo (one dword each for RGBA8), the frame
//                        of the face from the vertices of this call, the shading normal, and the point, light and Phong
//                        terms of paint_shade_kernel.
// No atomics, no LDS, no workspace. Everything is fp64 from the stored inputs with FMA contraction off, so the float64
// restatement of the contract (tests/nmap_reference.py) is matched to the rounding of the stored values. The layout, the
// corners of a cell, the tap and the light and Phong terms are enarf_shade.h's, the definitions enarf_bake.hip bakes and
// shades with; the frame of a face and the encoding of a channel are this file's own.
#include "enarf_nmap.h"
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
constexpr int kMaxR = ENARF_NMAP_MAX_SIZE;
constexpr AtlasLimits kLimits = {ENARF_NMAP_MIN_ATLAS, ENARF_NMAP_MAX_ATLAS, ENARF_NMAP_MIN_CELL};

__device__ __forceinline__ bool positive_finite(double x) { return x > 0.0 && x < (double)INFINITY; }

// the frame of triangle t (valid vertex indices v): false when it has none
__device__ __forceinline__ bool frame_of(const float *vertices, const long long v[3], long long t, double tg[3], double bt[3],
                                         double nr[3]) {
#pragma clang fp contract(off)
    const float *q0 = vertices + 3 * v[0], *q1 = vertices + 3 * v[1], *q2 = vertices + 3 * v[2];
    double e1[3], e2[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = (double)q1[k] - (double)q0[k];
        e2[k] = (double)q2[k] - (double)q0[k];
    }
    cross3(e1, e2, c);
    const double l1 = length3(e1), lc = length3(c);
    if (!positive_finite(l1) || !positive_finite(lc)) return false;
    const double s = (t & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        nr[k] = c[k] / lc;
        tg[k] = (s * e1[k]) / l1;
    }
    cross3(tg, nr, bt);
    return true;
}

// floor(255 clamp((c + 1) / 2, 0, 1) + 0.5)
__device__ __forceinline__ uint32_t channel(double c) {
#pragma clang fp contract(off)
    double h = (c + 1.0) / 2.0;
    h = h > 0.0 ? (h < 1.0 ? h : 1.0) : 0.0;
    return (uint32_t)(int)floor(255.0 * h + 0.5);
}

__global__ void __launch_bounds__(kBlock) nmap_encode_kernel(const enarf_nmap_encode_args a) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= a.count) return;
    const long long t = a.texel_face[e];
    double q[3] = {0.0, 0.0, 1.0};
    long long v[3] = {0, 0, 0};
    double tg[3], bt[3], nr[3];
    if (t >= 0 && t < a.T && corners_of(a.triangles, t, a.V, v) && frame_of(a.vertices, v, t, tg, bt, nr)) {
        double g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = (double)a.vectors[k * a.count + e];
            g[k] = a.negate ? -x : x;
        }
        const double m = length3(g);
        if (m > (double)a.min_length && m < (double)INFINITY) {
            q[0] = ((g[0] * tg[0] + g[1] * tg[1]) + g[2] * tg[2]) / m;
            q[1] = ((g[0] * bt[0] + g[1] * bt[1]) + g[2] * bt[2]) / m;
            q[2] = ((g[0] * nr[0] + g[1] * nr[1]) + g[2] * nr[2]) / m;
        }
    }
    const uint32_t rgba = channel(q[0]) | (channel(q[1]) << 8) | (channel(q[2]) << 16) | (t >= 0 ? 0xFF000000u : 0u);
    reinterpret_cast<uint32_t *>(a.texture)[e] = rgba;
    if (a.texture_f32) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.texture_f32[3 * e + k] = (float)q[k];
    }
}

__global__ void __launch_bounds__(kBlock) nmap_shade_kernel(const enarf_nmap_shade_args a, const Layout lay) {
#pragma clang fp contract(off)
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (long long)a.R * a.R) return;
    const long long f = a.pix_to_face[p];
    long long v[3] = {0, 0, 0};
    const bool drawn = f >= 0 && f < a.T && corners_of(a.triangles, f, a.V, v);
    double texel[3], shaded[3], ns[3];
    if (!drawn) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            texel[ch] = shaded[ch] = (double)a.background[ch];
            if (a.normal) ns[ch] = (double)a.normals[3 * p + ch];
        }
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
        if (a.texture) {
            tap_rgba8(a.texture, tp, 1.0, 0.0, texel);
        } else if (a.texture_f32) {
            tap_f32(a.texture_f32, tp, texel);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) texel[ch] = (double)a.base_color[ch];
        }
        const bool want_normal = a.lit || a.normal;
        double unit[3] = {0.0, 0.0, 0.0};                                    // the N of the light term
        if (want_normal) {
            double tg[3], bt[3], nr[3];
            if (frame_of(a.vertices, v, f, tg, bt, nr)) {
                double m[3];
                if (a.normal_texture) tap_rgba8(a.normal_texture, tp, 2.0, 1.0, m);
                else tap_f32(a.normal_texture_f32, tp, m);
                const double lm = length3(m);
                if (!positive_finite(lm)) m[0] = 0.0, m[1] = 0.0, m[2] = 1.0;
                double wv[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) wv[k] = (m[0] * tg[k] + m[1] * bt[k]) + m[2] * nr[k];
                const double lw = length3(wv);
#pragma unroll
                for (int k = 0; k < 3; ++k) ns[k] = unit[k] = wv[k] / lw;
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) ns[k] = (double)a.normals[3 * p + k];
                const double dn = floored_length(ns);
#pragma unroll
                for (int k = 0; k < 3; ++k) unit[k] = ns[k] / dn;
            }
        }
        if (a.lit) {
            const float *q0 = a.vertices + 3 * v[0], *q1 = a.vertices + 3 * v[1], *q2 = a.vertices + 3 * v[2];
            double pt[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                pt[k] = ((double)b0 * (double)q0[k] + (double)b1 * (double)q1[k]) + (double)b2 * (double)q2[k];
            phong(texel, facing(unit, pt, floored_length(pt)), shaded);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) shaded[ch] = texel[ch];
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (a.albedo) a.albedo[3 * p + ch] = (float)texel[ch];
        if (a.normal) a.normal[3 * p + ch] = (float)ns[ch];
        if (a.shaded) a.shaded[3 * p + ch] = (float)shaded[ch];
        a.image[3 * p + ch] = level(shaded[ch]);
    }
}

}  // namespace

extern "C" {

int enarf_nmap_abi_version(void) { return ENARF_NMAP_ABI_VERSION; }

const char *enarf_nmap_last_error(void) { return enarf::host::last_error(); }

int enarf_nmap_encode(const enarf_nmap_encode_args *args, void *stream) {
    const char *who = "enarf_nmap_encode";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_nmap_encode_args &a = *args;
    const long long most = (long long)ENARF_NMAP_MAX_ATLAS * ENARF_NMAP_MAX_ATLAS;
    if (a.count < 0 || a.count > most)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: %lld texels outside [0, %lld]", who, (long long)a.count, most);
    if (a.V < 0 || a.V >= kMaxCount || a.T < 0 || a.T >= kMaxCount)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld, T = %lld: both must lie in [0, 2^31)", who, (long long)a.V,
                                 (long long)a.T);
    if (!(a.min_length >= 0.0f)) return enarf::host::fail(ENARF_ERR_ARG, "%s: min_length must be >= 0", who);
    if (a.count == 0) return 0;
    if (!a.texel_face || !a.vectors || !a.texture || (a.V > 0 && !a.vertices) || (a.T > 0 && !a.triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null texel_face, vectors, texture, vertices or triangles", who);
    if (reinterpret_cast<uintptr_t>(a.texture) & 3u)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the texture is written one 32-bit texel at a time: 4-byte alignment", who);
    hipLaunchKernelGGL(nmap_encode_kernel, dim3(blocks(a.count, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_nmap_encode: nmap_encode_kernel");
}

int enarf_nmap_shade(const enarf_nmap_shade_args *args, void *stream) {
    const char *who = "enarf_nmap_shade";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_nmap_shade_args &a = *args;
    if (a.R < 1 || a.R > kMaxR) return enarf::host::fail(ENARF_ERR_ARG, "%s: render size %d outside [1, %d]", who, a.R, kMaxR);
    if (a.V < 0 || a.V >= kMaxCount) return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld outside [0, 2^31)", who, (long long)a.V);
    Layout lay;
    if (const int rc = find_layout(who, (long long)a.T, a.A, kLimits, &lay)) return rc;
    if ((a.normal_texture != nullptr) == (a.normal_texture_f32 != nullptr))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: exactly one of normal_texture and normal_texture_f32 must be given", who);
    if (a.texture && a.texture_f32)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: at most one of texture and texture_f32 may be given", who);
    if ((reinterpret_cast<uintptr_t>(a.normal_texture) & 3u) || (reinterpret_cast<uintptr_t>(a.texture) & 3u))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: an RGBA8 texture is read one 32-bit texel at a time: 4-byte alignment", who);
    if (!a.pix_to_face || !a.bary || !a.normals || !a.image || (a.V > 0 && !a.vertices) || (a.T > 0 && !a.triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null pix_to_face, bary, normals, image, vertices or triangles", who);
    hipLaunchKernelGGL(nmap_shade_kernel, dim3(blocks((long long)a.R * a.R, kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a, lay);
    return enarf::host::check_launch("enarf_nmap_shade: nmap_shade_kernel");
}

}  // extern "C"
