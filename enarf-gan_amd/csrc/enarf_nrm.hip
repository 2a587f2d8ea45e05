// enarf_nrm.hip - libenarf_nrm.so: normals from the field's own density gradient (gfx950 / CDNA4 only, wave64). The
// contract is in include/enarf_nrm.h.
//
//   nrm_gradient_kernel  one lane per point, a workgroup per 256 points of one image, one launch. pgrad_query_kernel's
//                        chain (enarf_pgrad.hip) cut down to the one output a normal needs: the same dense fp32 weights
//                        in LDS (enarf_grad.h), the same walk 1 (enarf_parts.h) and the same rolled forward loop over the
//                        64 layer-1 units, then only the density row of the last layer; the backward starts from that one
//                        pre-activation with upstream 1, and a lane whose density head is off skips it and walk 2
//                        altogether (its gradient is an exact zero). Walk 2 chains each valid part's gradient at the
//                        canonical point to the point; no record entries, no reductions, no fp64, no workspace.
//   nrm_ray_kernel       one lane per ray: the fine weights times the samples' gradients summed in ascending order in
//                        fp64 (FMA contraction off, as enarf_geom.hip), the validity rule, the fallback and the shade.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "enarf_nrm.h"
#include "enarf_parts.h"
#include "enarf_grad.h"
#include "enarf_host.h"

namespace {

using namespace enarf;

constexpr int kBlock = ENARF_NRM_BLOCK;
constexpr int kMaxParts = ENARF_NRM_MAX_PARTS;
static_assert(kMaxParts == ENARF_MAX_PARTS, "the bit mask of the march");

// two waves a SIMD: the walks' gathers are latency the second wave hides. Left alone the register allocator takes 284
// registers and one wave; a third wave costs more in spills than it hides (DESIGN.md 3.21 has the three timings)
__global__ void __launch_bounds__(kBlock, 2) nrm_gradient_kernel(const enarf_nrm_gradient_args a) {
    __shared__ __attribute__((aligned(16))) float l_w[(LW_FLOATS + 3) / 4 * 4];
    __shared__ __attribute__((aligned(16))) float l_parts[kMaxParts * kLdsPartStride];
    __shared__ __attribute__((aligned(16))) float l_canon[kMaxParts * kLdsCanonStride];
    const int tid = threadIdx.x, P = a.P, H = a.H, W = a.W;
    const int b = blockIdx.y, blk = blockIdx.x;

    // ---- staging: part frames and the dense weights (enarf_grad.h)
    stage_frames(l_parts, l_canon, a.parts + (size_t)b * P * kPartStride, a.canonical_pose, P, tid, kBlock);
    stage_dense_weights(l_w, reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.mlp_pack) + (size_t)b * kPackBytes),
                        tid, kBlock);
    __syncthreads();

    const long long i = (long long)blk * kBlock + tid;
    if (i >= a.N) return;                                   // no barrier below
    const float *pts = a.points + (size_t)b * 3 * a.N;
    const float px = pts[i], py = pts[a.N + i], pz = pts[2 * a.N + i];

    const float *featp = a.feat_cl + (size_t)b * a.feat_batch_stride;
    const float *maskp = a.mask_planes + (size_t)b * a.mask_batch_stride;
    const char *maskb = reinterpret_cast<const char *>(maskp);
    const size_t plane = (size_t)H * W;
    const unsigned plane_bytes = (unsigned)plane << 2;      // 3 P planes stay below 2^32 bytes (checked on the host)
    const bool uniform = a.uniform_part_weight != 0;
    const float uniform_w = 1.0f / (float)P;

    // ---- walk 1: validity, the weighted feature, the largest weight and the first part that has it
    uint32_t bits = 0;
    int kmax = -1;
    float wmax = 0.0f;
    float feat[kFeat];
#pragma unroll
    for (int c = 0; c < kFeat; ++c) feat[c] = 0.0f;
    for (int k = 0; k < P; ++k) {
        float F[13], Cn[12], lx, ly, lz, cx, cy, cz;
        load_frames(l_parts, l_canon, k, F, Cn);
        part_point(F, Cn, px, py, pz, lx, ly, lz, cx, cy, cz);
        if (!ENARF_POINT_IN_PART(lx, ly, lz, cx, cy, cz)) continue;
        bits |= 1u << k;
        const float w = uniform ? uniform_w : part_probability(maskb, k, plane_bytes, cx, cy, cz, H, W, a.clamp_mask);
        if (w > wmax) { wmax = w; kmax = k; }
        float acc[kFeat];
#pragma unroll
        for (int c = 0; c < kFeat; ++c) acc[c] = 0.0f;
#pragma unroll 1
        for (int pl = 0; pl < 3; ++pl) {                   // rolled: one plane's 32 texel loads in flight, not all 96
            float qx, qy;
            plane_xy(pl, cx, cy, cz, qx, qy);
            const Taps t = make_taps(qx, qy, H, W);
            const int o[4] = {t.o00, t.o01, t.o10, t.o11};
            const float tw[4] = {t.w00, t.w01, t.w10, t.w11};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 *v = reinterpret_cast<const f32x4 *>(featp + (pl * plane + (size_t)o[j]) * kFeat);
#pragma unroll
                for (int c4 = 0; c4 < kFeat / 4; ++c4) {
                    const f32x4 q = v[c4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[4 * c4 + r] += q[r] * tw[j];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kFeat; ++c) feat[c] += acc[c] * w;
    }

    // ---- the MLP forward to the density head, and from it backward: gf = d density / d feature, g_wm = d density / d (max w)
    float density = 0.0f, g_wm = 0.0f;
    float gf[kFeat];
#pragma unroll
    for (int c = 0; c < kFeat; ++c) gf[c] = 0.0f;
    bool on = false;                                        // the density head passes a gradient
    if (bits) {
        float z2[kHid];
#pragma unroll
        for (int j = 0; j < kHid; ++j) z2[j] = l_w[LW_B2 + j];
        uint64_t s1 = 0, s2 = 0;                            // units whose pre-activation is positive
#pragma unroll 1
        for (int o = 0; o < kHid; ++o) {
            const f32x4 *w1 = reinterpret_cast<const f32x4 *>(l_w + LW_W1 + o * kFeat);
            float z = l_w[LW_B1 + o];
#pragma unroll
            for (int c4 = 0; c4 < kFeat / 4; ++c4) {
                const f32x4 q = w1[c4];
#pragma unroll
                for (int r = 0; r < 4; ++r) z += q[r] * feat[4 * c4 + r];
            }
            s1 |= (uint64_t)(z > 0.0f) << o;
            const float h = styled_act(z);
            const f32x4 *w2 = reinterpret_cast<const f32x4 *>(l_w + LW_W2T + o * kHid);
#pragma unroll
            for (int j4 = 0; j4 < kHid / 4; ++j4) {
                const f32x4 q = w2[j4];
#pragma unroll
                for (int r = 0; r < 4; ++r) z2[4 * j4 + r] += q[r] * h;
            }
        }
        float z3 = l_w[LW_B3 + 3];                          // row 3 of the last layer: the density head
#pragma unroll
        for (int j = 0; j < kHid; ++j) {
            s2 |= (uint64_t)(z2[j] > 0.0f) << j;
            z3 += l_w[LW_W3 + 3 * kHid + j] * styled_act(z2[j]);
        }
        const float h = styled_act(z3);
        float factor = 10.0f;
        bool to_wmax = false;
        if (a.multiply_density_with_weight) {
            // the factor max w over ALL parts, an invalid one weighs 0.125 (density_head in enarf_march.h); its gradient
            // goes to the part that has it, nowhere when that is an invalid part or every weight is 1 / P
            const bool invalid_wins = !uniform && __popc(bits) < P && !(wmax >= 0.125f);
            const float wm = uniform ? uniform_w : invalid_wins ? 0.125f : wmax;
            factor = 10.0f * wm;
            to_wmax = !uniform && !invalid_wins;
        }
        density = fmaxf(h, 0.0f) * factor;
        on = h >= 0.0f;                                     // MyReLU's rule under the upstream 1: the plain derivative
        if (on) {
            if (to_wmax) g_wm = 10.0f * fmaxf(h, 0.0f);
            const float gz3 = factor * act_slope(z3 > 0.0f);
#pragma unroll
            for (int j = 0; j < kHid; ++j)                  // d density / d z2, in place
                z2[j] = (l_w[LW_W3 + 3 * kHid + j] * gz3) * act_slope((s2 >> j) & 1);
#pragma unroll 1
            for (int o = 0; o < kHid; ++o) {
                const f32x4 *w2 = reinterpret_cast<const f32x4 *>(l_w + LW_W2T + o * kHid);
                float g = 0.0f;
#pragma unroll
                for (int j4 = 0; j4 < kHid / 4; ++j4) {
                    const f32x4 q = w2[j4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) g += q[r] * z2[4 * j4 + r];
                }
                g *= act_slope((s1 >> o) & 1);
                const f32x4 *w1 = reinterpret_cast<const f32x4 *>(l_w + LW_W1 + o * kFeat);
#pragma unroll
                for (int c4 = 0; c4 < kFeat / 4; ++c4) {
                    const f32x4 q = w1[c4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) gf[4 * c4 + r] += q[r] * g;
                }
            }
        }
    }

    // ---- walk 2: each valid part's gradient at its canonical point, chained through Rc, the scale and R to the point
    float gpx = 0.0f, gpy = 0.0f, gpz = 0.0f;
    if (on) {
        for (int k = 0; k < P; ++k) {
            if (!((bits >> k) & 1u)) continue;
            float F[13], Cn[12], lx, ly, lz, cx, cy, cz;
            load_frames(l_parts, l_canon, k, F, Cn);
            part_point(F, Cn, px, py, pz, lx, ly, lz, cx, cy, cz);
            float w = uniform_w, sg[3] = {0.0f, 0.0f, 0.0f};
            if (!uniform) {
                const unsigned off = (unsigned)(3 * k) * plane_bytes;
                sg[0] = plane_sigmoid(maskb, off, cx, cy, H, W, a.clamp_mask);
                sg[1] = plane_sigmoid(maskb, off + plane_bytes, cy, cz, H, W, a.clamp_mask);
                sg[2] = plane_sigmoid(maskb, off + 2u * plane_bytes, cz, cx, H, W, a.clamp_mask);
                w = (sg[0] * sg[1]) * sg[2];
            }
            // the planes one at a time in a rolled loop, so that one plane's 32 texel loads are in flight and not all 96:
            // its four sums go to statically indexed slots through selects
            float ga[3] = {0.0f, 0.0f, 0.0f}, gb[3] = {0.0f, 0.0f, 0.0f};     // gf . d f_k / d (plane pl's two coordinates)
            float ma[3] = {0.0f, 0.0f, 0.0f}, mb[3] = {0.0f, 0.0f, 0.0f};     // d m_p / d (its two coordinates)
            float e_f = 0.0f;                               // gf . f_k, the gradient that reaches w_k
#pragma unroll 1
            for (int pl = 0; pl < 3; ++pl) {
                float qx, qy;
                plane_xy(pl, cx, cy, cz, qx, qy);
                const GTaps t = grad_taps(qx, qy, H, W);
                float sa = 0.0f, sb = 0.0f, sma = 0.0f, smb = 0.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 *tv = reinterpret_cast<const f32x4 *>(featp + (pl * plane + (size_t)t.o[j]) * kFeat);
                    float dot = 0.0f;
#pragma unroll
                    for (int c4 = 0; c4 < kFeat / 4; ++c4) {
                        const f32x4 q = tv[c4];
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) dot += q[rr] * gf[4 * c4 + rr];
                    }
                    e_f += dot * t.w[j];
                    sa += dot * t.wx[j];
                    sb += dot * t.wy[j];
                }
                if (!uniform) {                             // part-probability plane pl has the same cell: one tap set
                    const float *mp = maskp + (size_t)(3 * k + pl) * plane;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float m = mp[t.o[j]];
                        sma += m * t.wx[j];
                        smb += m * t.wy[j];
                    }
                }
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    ga[s] = (pl == s) ? sa : ga[s];
                    gb[s] = (pl == s) ? sb : gb[s];
                    ma[s] = (pl == s) ? sma : ma[s];
                    mb[s] = (pl == s) ? smb : mb[s];
                }
            }
            float Gc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                Gc[pl] += w * ga[pl];
                Gc[(pl + 1) % 3] += w * gb[pl];
            }
            if (!uniform) {                                 // the weight's term waits for e_f
                const float gw = e_f + (k == kmax ? g_wm : 0.0f);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    const float f = gw * (w * (1.0f - sg[pl]));     // dw_k / dm_p = w_k (1 - s_p), clamped or not
                    Gc[pl] += f * ma[pl];
                    Gc[(pl + 1) % 3] += f * mb[pl];
                }
            }
            const float dq0 = (Cn[0] * Gc[0] + Cn[3] * Gc[1]) + Cn[6] * Gc[2];      // Rc^T G_c
            const float dq1 = (Cn[1] * Gc[0] + Cn[4] * Gc[1]) + Cn[7] * Gc[2];
            const float dq2 = (Cn[2] * Gc[0] + Cn[5] * Gc[1]) + Cn[8] * Gc[2];
            const float dl0 = F[12] * dq0, dl1 = F[12] * dq1, dl2 = F[12] * dq2;
            gpx += (F[0] * dl0 + F[1] * dl1) + F[2] * dl2;                          // R dl
            gpy += (F[3] * dl0 + F[4] * dl1) + F[5] * dl2;
            gpz += (F[6] * dl0 + F[7] * dl1) + F[8] * dl2;
        }
    }
    a.density[(size_t)b * a.N + i] = density;
    float *gp = a.gradient + (size_t)b * 3 * a.N;
    gp[i] = gpx; gp[a.N + i] = gpy; gp[2 * a.N + i] = gpz;
}

__global__ void __launch_bounds__(kBlock) nrm_ray_kernel(const enarf_nrm_ray_args a) {
#pragma clang fp contract(off)
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int b = blockIdx.y, Nf = a.Nf;
    if (r >= a.n) return;
    const long long ray = (long long)b * a.n + r;
    const float *w = a.weights + ray * (Nf - 1);
    const float *g = a.gradient + (long long)b * 3 * a.n * Nf + r * Nf;
    const long long comp = a.n * Nf;                       // floats between two components of the gradient
    double G[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < Nf - 1; ++i) {
        const double wi = (double)w[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) G[k] = G[k] + wi * (double)g[k * comp + i];
    }
    const double m = sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
    const uint8_t in = a.flags_in ? a.flags_in[ray] : (uint8_t)0;
    const bool field = a.mask[ray] >= a.mask_threshold && m > (double)a.min_gradient && m < HUGE_VAL;
    const bool fall = !field && a.fallback && (in & ENARF_NRM_FLAG_NORMAL);
    double N[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (field) N[k] = -G[k] / m;
        else if (fall) N[k] = (double)a.fallback[3 * ray + k];
        a.normals[3 * ray + k] = (float)N[k];
    }
    a.flags[ray] = (uint8_t)((in & ~ENARF_NRM_FLAG_FIELD) | (field ? ENARF_NRM_FLAG_FIELD : 0));
    if (a.magnitude) a.magnitude[ray] = (float)m;
    if (a.image) {
        double v[3] = {(double)a.background[0], (double)a.background[1], (double)a.background[2]};
        if (a.shade == ENARF_NRM_SHADE_NORMAL && (field || fall)) {
            v[0] = 0.5 + 0.5 * N[0];
            v[1] = 0.5 + 0.5 * -N[1];
            v[2] = 0.5 + 0.5 * -N[2];
        } else if (a.shade == ENARF_NRM_SHADE_LIT && (field || fall)) {
            const double p0 = (double)a.points[3 * ray], p1 = (double)a.points[3 * ray + 1], p2 = (double)a.points[3 * ray + 2];
            const double dp = fmax(sqrt((p0 * p0 + p1 * p1) + p2 * p2), 1e-6);
            const double cs = -((N[0] * p0 + N[1] * p1) + N[2] * p2) / dp;
            double spec = 0.0;
            if (cs > 0.0) {
                spec = fmax(2.0 * cs * cs - 1.0, 0.0);
#pragma unroll
                for (int k = 0; k < 6; ++k) spec *= spec;                  // ^64
            }
            v[0] = v[1] = v[2] = (0.5 + 0.3 * (cs > 0.0 ? cs : 0.0)) + 0.2 * spec;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.image[3 * ray + k] = level(v[k]);
    }
}

}  // namespace

extern "C" {

int enarf_nrm_abi_version(void) { return ENARF_NRM_ABI_VERSION; }

const char *enarf_nrm_last_error(void) { return enarf::host::last_error(); }

int enarf_nrm_field_gradient(const enarf_nrm_gradient_args *args, void *stream) {
    const char *who = "enarf_nrm_field_gradient";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_nrm_gradient_args &a = *args;
    if (a.B < 1 || a.N < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: B %d, N %lld", who, a.B, (long long)a.N);
    if (a.B > 65535 || a.N / kBlock + 1 >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: B %d above 65535 or N %lld needs 2^31 workgroups", who, a.B, (long long)a.N);
    if (const int e = enarf::host::check_part_planes(who, a.P, kMaxParts, a.H, a.W)) return e;
    if (96LL * a.H * a.W >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: planes %d x %d: 96 H W must stay below 2^31 floats", who, a.H, a.W);
    if (a.feat_batch_stride < 0 || a.mask_batch_stride < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: negative batch strides", who);
    if (a.N == 0) return 0;
    if (!a.points || !a.parts || !a.canonical_pose || !a.feat_cl || (!a.mask_planes && !a.uniform_part_weight) || !a.mlp_pack ||
        !a.density || !a.gradient)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null points, parts, canonical_pose, feat_cl, mask_planes, mlp_pack, density or gradient", who);
    if (((uintptr_t)a.feat_cl & 15) || ((a.feat_batch_stride * 4) & 15))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: feat_cl must be 16-byte aligned per image", who);
    const unsigned nblk = (unsigned)((a.N + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(nrm_gradient_kernel, dim3(nblk, (unsigned)a.B), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_nrm_field_gradient: nrm_gradient_kernel");
}

int enarf_nrm_ray_normals(const enarf_nrm_ray_args *args, void *stream) {
    const char *who = "enarf_nrm_ray_normals";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_nrm_ray_args &a = *args;
    if (a.B < 1 || a.n < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: B %d, n %lld", who, a.B, (long long)a.n);
    if (a.Nf < 2 || a.Nf > ENARF_NRM_MAX_SAMPLES)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: Nf %d outside [2, %d]", who, a.Nf, ENARF_NRM_MAX_SAMPLES);
    if (a.B > 65535) return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: B %d above 65535", who, a.B);
    if (a.n * a.Nf >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: n %lld with Nf %d: n Nf must stay below 2^31", who, (long long)a.n, a.Nf);
    if (a.shade < ENARF_NRM_SHADE_NONE || a.shade > ENARF_NRM_SHADE_LIT)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: shade mode %d outside [-1, 1]", who, a.shade);
    if ((a.shade == ENARF_NRM_SHADE_NONE) != (a.image == nullptr))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: an image goes with a shade mode, and a shade mode with an image", who);
    if ((a.fallback == nullptr) != (a.flags_in == nullptr))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: fallback normals go with their flags", who);
    if (a.n == 0) return 0;
    if (a.shade == ENARF_NRM_SHADE_LIT && !a.points) return enarf::host::fail(ENARF_ERR_ARG, "%s: the lit shade takes points", who);
    if (!a.gradient || !a.weights || !a.mask || !a.normals || !a.flags)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null gradient, weights, mask, normals or flags", who);
    const unsigned nblk = (unsigned)((a.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(nrm_ray_kernel, dim3(nblk, (unsigned)a.B), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_nrm_ray_normals: nrm_ray_kernel");
}

}  // extern "C"
