// enarf_parts.h - the part-membership walk: which parts contain a point, and with what probability. One definition for
// the kernels that ask (the forward march and the query through query_tile, the backward, seg_label_kernel,
// skin_weights_kernel), so their validity bits and part probabilities agree bit for bit. Needs no QueryCtx.
#pragma once
#include "enarf_device.h"

namespace enarf {

// part frames / canonical frames in LDS: strides chosen so that 16 different parts read in one wave
// instruction spread over the banks (16-float stride would put parts k and k+2 on the same banks)
constexpr int kLdsPartStride = 20;   // 16 used
constexpr int kLdsCanonStride = 12;

// stage one image's (P, 16) part frames and the (P, 4, 4) canonical poses into LDS; the caller synchronises
__device__ __forceinline__ void stage_frames(float *l_parts, float *l_canon, const float *parts_b,
                                             const float *canonical_pose, int P, int tid, int nthreads) {
    for (int i = tid; i < P * kPartStride; i += nthreads)
        l_parts[(i / kPartStride) * kLdsPartStride + (i % kPartStride)] = parts_b[i];
    for (int i = tid; i < P * 12; i += nthreads) {   // (P,4,4) -> Rc row-major 9 + tc 3
        const int k = i / 12, e = i % 12;
        l_canon[i] = (e < 9) ? canonical_pose[k * 16 + (e / 3) * 4 + (e % 3)] : canonical_pose[k * 16 + (e - 9) * 4 + 3];
    }
}

__device__ __forceinline__ void load_frames(const float *l_parts, const float *l_canon, int k, float F[13], float Cn[12]) {
    const f32x4 *pf = reinterpret_cast<const f32x4 *>(l_parts + k * kLdsPartStride);
    const f32x4 *pc = reinterpret_cast<const f32x4 *>(l_canon + k * kLdsCanonStride);
    const f32x4 f0 = pf[0], f1 = pf[1], f2 = pf[2], f3 = pf[3];
    const f32x4 c0 = pc[0], c1 = pc[1], c2 = pc[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { F[i] = f0[i]; F[4 + i] = f1[i]; F[8 + i] = f2[i]; }
    F[12] = f3[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) { Cn[i] = c0[i]; Cn[4 + i] = c1[i]; Cn[8 + i] = c2[i]; }
}

// the point in the part's local frame (l) and in its canonical frame (c)
__device__ __forceinline__ void part_point(const float F[13], const float Cn[12], float px, float py, float pz, float &lx,
                                           float &ly, float &lz, float &cx, float &cy, float &cz) {
    exact_local(F, px, py, pz, lx, ly, lz);
    exact_canonical(Cn, F[12], lx, ly, lz, cx, cy, cz);
}

// The membership test on part_point's results: the part contains the point when the local point is in the closed unit cube
// and the canonical point in the open one. A macro, because the callers put it in one short-circuit chain with their own
// guards (`active && has &&` in the march and the backward, a `continue` in seg and skin): behind a function call the
// chain reaches the optimiser in another block order, and the march, the query and the backward compile to other code
// (profiles/r16_parts.log lists the kernels)
#define ENARF_POINT_IN_PART(lx, ly, lz, cx, cy, cz) \
    (::enarf::in_unit_cube_incl(lx, ly, lz) && ::enarf::in_unit_cube_strict(cx, cy, cz))

// sigmoid(bilinear(plane)) of one part-probability plane at (x, y) (sampling.py:43-48, :62). A part's probability is
// (s0 * s1) * s2 over its planes xy, yz, zx. The gather rounds of query_tile (enarf_query.h) and of the backward
// (bwd_gather_tile, bwd_backward_tile in enarf_render_bwd.hip) are the other implementation of the same formula: there lane
// g of a quad samples plane g and the product is formed from three quad broadcasts. An edit to one form belongs in the other
// (part_probability below is the one-lane form).
__device__ __forceinline__ float plane_sigmoid(const char *__restrict__ maskb, unsigned plane_off, float x, float y, int H,
                                               int W, int clamp_mask) {
    const Taps t = make_taps(x, y, H, W);
    float m00, m01, m10, m11;
    load_row_pair(maskb, plane_off, t.o00, t.xe, m00, m01);
    load_row_pair(maskb, plane_off, t.o10, t.xe, m10, m11);
    float macc = m00 * t.w00;
    macc += m01 * t.w01;
    macc += m10 * t.w10;
    macc += m11 * t.w11;
    if (clamp_mask) macc = fminf(fmaxf(macc, -2.0f), 5.0f);
    return sigmoidf_(macc);
}

// the probability of part k at its canonical point, one lane doing the three planes; plane_bytes = 4 H W, and the 3 P planes
// stay below 2^32 bytes (host::check_part_planes)
__device__ __forceinline__ float part_probability(const char *maskb, int k, unsigned plane_bytes, float cx, float cy, float cz,
                                                  int H, int W, int clamp_mask) {
    const unsigned off = (unsigned)(3 * k) * plane_bytes;
    const float s0 = plane_sigmoid(maskb, off, cx, cy, H, W, clamp_mask);
    const float s1 = plane_sigmoid(maskb, off + plane_bytes, cy, cz, H, W, clamp_mask);
    const float s2 = plane_sigmoid(maskb, off + 2u * plane_bytes, cz, cx, H, W, clamp_mask);
    return (s0 * s1) * s2;
}

}  // namespace enarf
