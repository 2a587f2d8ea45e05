// enarf_grad.h - what the kernels that differentiate the query with respect to its sample point share (pgrad_query_kernel
// in enarf_pgrad.hip, nrm_gradient_kernel in enarf_nrm.hip): the dense fp32 MLP weights in LDS, the slope of the styled
// activation, and the bilinear taps with the derivatives of their weights. Device functions only; each library keeps its
// own kernels.
#pragma once
#include "enarf_device.h"

namespace enarf {

// dense weights in LDS (floats)
constexpr int LW_W1 = 0;                               // [64 units][32 channels]
constexpr int LW_W2T = LW_W1 + kHid * kFeat;           // [64 layer-1 units][64 layer-2 units]
constexpr int LW_W3 = LW_W2T + kHid * kHid;            // [4][64]
constexpr int LW_B1 = LW_W3 + 4 * kHid;
constexpr int LW_B2 = LW_B1 + kHid;
constexpr int LW_B3 = LW_B2 + kHid;
constexpr int LW_FLOATS = LW_B3 + 4;                   // 6532 floats = 26128 B

// one image's demodulated fp32 weights out of the pack's MFMA operand order (enarf_device.h) into dense rows: W1
// [unit][32], W2 transposed [layer-1 unit][64], W3 [4][64], then b1, b2 and b3's 4 of 16; the caller synchronises
__device__ __forceinline__ void stage_dense_weights(float *l_w, const float *pf, int tid, int nthreads) {
    for (int e = tid; e < kHid * kFeat; e += nthreads) {
        const int o = e >> 5, c = e & 31;
        l_w[LW_W1 + e] = pf[PK_W1 + ((o >> 4) * 8 + (c & 7)) * 64 + (c >> 3) * 16 + (o & 15)];
    }
    for (int e = tid; e < kHid * kHid; e += nthreads) {    // e = (layer-1 unit c, layer-2 unit o): W2[o][c]
        const int c = e >> 6, o = e & 63;
        const int q = (c >> 4) * 4 + (c & 3), g = (c & 15) >> 2;
        l_w[LW_W2T + e] = pf[PK_W2 + ((o >> 4) * 16 + q) * 64 + g * 16 + (o & 15)];
    }
    for (int e = tid; e < 4 * kHid; e += nthreads) {
        const int o = e >> 6, c = e & 63;
        const int q = (c >> 4) * 4 + (c & 3), g = (c & 15) >> 2;
        l_w[LW_W3 + e] = pf[PK_W3 + q * 64 + g * 16 + o];
    }
    for (int e = tid; e < 2 * kHid + 4; e += nthreads) l_w[LW_B1 + e] = pf[PK_B1 + e];    // b1, b2, then b3's 4 of 16
}

constexpr float kSqrt2 = 1.41421356237309515f;
__device__ __forceinline__ float act_slope(bool positive) { return positive ? kSqrt2 : 0.2f * kSqrt2; }

// the four taps of make_taps (nw, ne, sw, se) with the derivative of each tap's weight with respect to the sampled
// coordinate: d ix / d x = W / 2, the floor is a constant, a tap outside the plane weighs zero and so does its derivative
struct GTaps { int o[4]; float w[4], wx[4], wy[4]; };
__device__ __forceinline__ GTaps grad_taps(float x, float y, int H, int W) {
    const Taps t = make_taps(x, y, H, W);
    GTaps g;
    g.o[0] = t.o00; g.o[1] = t.o01; g.o[2] = t.o10; g.o[3] = t.o11;
    g.w[0] = t.w00; g.w[1] = t.w01; g.w[2] = t.w10; g.w[3] = t.w11;
    float ix, iy;
    {
#pragma clang fp contract(off)
        ix = ((x + 1.0f) * (float)W - 1.0f) / 2.0f;
        iy = ((y + 1.0f) * (float)H - 1.0f) / 2.0f;
    }
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const bool bx0 = (x0 >= 0) & (x0 < W), bx1 = (x1 >= 0) & (x1 < W);
    const bool by0 = (y0 >= 0) & (y0 < H), by1 = (y1 >= 0) & (y1 < H);
    const float zx0 = bx0 ? (fx + 1.0f) - ix : 0.0f, zx1 = bx1 ? ix - fx : 0.0f;
    const float zy0 = by0 ? (fy + 1.0f) - iy : 0.0f, zy1 = by1 ? iy - fy : 0.0f;
    const float hx = 0.5f * (float)W, hy = 0.5f * (float)H;
    const float dx0 = bx0 ? -hx : 0.0f, dx1 = bx1 ? hx : 0.0f, dy0 = by0 ? -hy : 0.0f, dy1 = by1 ? hy : 0.0f;
    g.wx[0] = dx0 * zy0; g.wx[1] = dx1 * zy0; g.wx[2] = dx0 * zy1; g.wx[3] = dx1 * zy1;
    g.wy[0] = zx0 * dy0; g.wy[1] = zx1 * dy0; g.wy[2] = zx0 * dy1; g.wy[3] = zx1 * dy1;
    return g;
}

// the coordinates plane pl is sampled at: (c[pl], c[(pl + 1) % 3])   (sampling.py:30)
__device__ __forceinline__ void plane_xy(int pl, float cx, float cy, float cz, float &qx, float &qy) {
    qx = (pl == 0) ? cx : (pl == 1) ? cy : cz;
    qy = (pl == 0) ? cy : (pl == 1) ? cz : cx;
}

}  // namespace enarf
