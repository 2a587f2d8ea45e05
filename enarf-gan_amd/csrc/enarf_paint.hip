// enarf_paint.hip - libenarf_paint.so: deferred shading of a rasterised mesh with a colour or a part label per vertex
// (gfx950 / CDNA4 only, wave64). The contract is in include/enarf_paint.h.
//
//   paint_shade_kernel   one lane per pixel, one launch per image: the fragment of the pixel (face id, stored b', stored
//                        normal) is turned into a texel - the barycentric mix of the three vertex colours, or the palette
//                        entry of the corner with the largest b' -, the point and the light term are rebuilt from the same
//                        b', and albedo, shaded and the 8-bit image are written. No atomics, no LDS, no workspace: every
//                        output is a function of the inputs alone. Background pixels read nothing through their face id,
//                        so a wave over background costs three loads and the stores.
// Everything is fp64 from the fp32 inputs with FMA contraction off, as in enarf_raster.hip, so the float64 restatement
// of the contract (tests/paint_reference.py) is matched to the rounding of the stored fp32. The corners of a face and
// the light and Phong terms are enarf_shade.h's, which the textured shades (enarf_bake.hip, enarf_nmap.hip) use too.
#include "enarf_paint.h"
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
constexpr int kMaxR = ENARF_PAINT_MAX_SIZE;

// the corner of the largest stored b', compared as fp32: a later corner wins only when strictly larger
__device__ __forceinline__ int top_corner(float b0, float b1, float b2) {
    int k = 0;
    float best = b0;
    if (b1 > best) { best = b1; k = 1; }
    if (b2 > best) k = 2;
    return k;
}

__global__ void __launch_bounds__(kBlock) paint_shade_kernel(const enarf_paint_shade_args a) {
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
        if (a.vertex_colors) {
            const float *c0 = a.vertex_colors + 3 * v[0], *c1 = a.vertex_colors + 3 * v[1], *c2 = a.vertex_colors + 3 * v[2];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                texel[ch] = ((double)b0 * (double)c0[ch] + (double)b1 * (double)c1[ch]) + (double)b2 * (double)c2[ch];
        } else {
            const int k = top_corner(b0, b1, b2);
            const int l = a.vertex_labels[k == 0 ? v[0] : k == 1 ? v[1] : v[2]];
            const bool known = l >= 0 && l < a.P;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) texel[ch] = (double)(known ? a.palette[3 * l + ch] : a.neutral[ch]);
        }
        if (a.lit) {
            const float *q0 = a.vertices + 3 * v[0], *q1 = a.vertices + 3 * v[1], *q2 = a.vertices + 3 * v[2];
            double n[3], q[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                n[c] = (double)a.normals[3 * p + c];
                q[c] = ((double)b0 * (double)q0[c] + (double)b1 * (double)q1[c]) + (double)b2 * (double)q2[c];
            }
            phong(texel, light_term(n, q), shaded);
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

int enarf_paint_abi_version(void) { return ENARF_PAINT_ABI_VERSION; }

const char *enarf_paint_last_error(void) { return enarf::host::last_error(); }

int enarf_paint_shade(const enarf_paint_shade_args *args, void *stream) {
    const char *who = "enarf_paint_shade";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_paint_shade_args &a = *args;
    if (a.R < 1 || a.R > kMaxR) return enarf::host::fail(ENARF_ERR_ARG, "%s: render size %d outside [1, %d]", who, a.R, kMaxR);
    if (a.V < 0 || a.V >= kMaxCount || a.T < 0 || a.T >= kMaxCount)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld, T = %lld: both must lie in [0, 2^31)", who, (long long)a.V,
                                 (long long)a.T);
    // without vertices neither array has an address: only then may both be null
    if ((a.vertex_colors && a.vertex_labels) || (a.V > 0 && !a.vertex_colors && !a.vertex_labels))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: exactly one of vertex_colors and vertex_labels must be given", who);
    if (a.vertex_labels && (!a.palette || a.P < 1))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: label mode takes a palette of P >= 1 entries, got P = %d", who, a.P);
    if (!a.pix_to_face || !a.bary || !a.normals || !a.image || (a.V > 0 && !a.vertices) || (a.T > 0 && !a.triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null pix_to_face, bary, normals, image, vertices or triangles", who);
    hipLaunchKernelGGL(paint_shade_kernel, dim3(blocks((long long)a.R * a.R, kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_paint_shade: paint_shade_kernel");
}

}  // extern "C"
