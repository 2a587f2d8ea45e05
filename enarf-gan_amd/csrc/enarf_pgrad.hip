// enarf_pgrad.hip - libenarf_pgrad.so: the query's gradient with respect to the sample points and the part records
// (gfx950 / CDNA4 only, wave64). The contract is in include/enarf_pgrad.h.
//
//   pgrad_query_kernel   one lane per point, a workgroup per 256 points of one image. The image's demodulated fp32 MLP
//                        weights are re-laid from the pack's MFMA operand order into dense rows in LDS (W1 [unit][32],
//                        W2 transposed [layer-1 unit][64], W3 [4][64]) beside the part frames. Walk 1 (enarf_parts.h)
//                        rebuilds the weighted feature; the MLP runs forward and backward as two rolled loops over the 64
//                        layer-1 units (unit o is finished and scattered into layer 2's 64 accumulators at once, so every
//                        register array is indexed statically and layer 1 keeps only its 64 sign bits); walk 2 forms each
//                        valid part's gradient at the canonical point, chains it to the point and to the record, and the
//                        wave sums the record's 13 entries in fp64. No atomics: a workgroup's four wave sums meet in LDS
//                        and go to the workspace as one partial.
//   pgrad_finish_kernel  a workgroup per (part, image): the partials summed in a fixed order in fp64, rounded once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "enarf_pgrad.h"
#include "enarf_parts.h"
#include "enarf_grad.h"
#include "enarf_host.h"

namespace {

using namespace enarf;

constexpr int kBlock = ENARF_PGRAD_BLOCK;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxParts = ENARF_PGRAD_MAX_PARTS;
constexpr int kRec = 13;                               // record entries that carry a gradient: R 9, t 3, s 1
static_assert(kMaxParts == ENARF_MAX_PARTS, "the bit mask of the march");
static_assert(kWaves == 4, "the partial adds four wave sums");

__global__ void __launch_bounds__(kBlock) pgrad_query_kernel(const enarf_pgrad_query_args a, const int nblk) {
    __shared__ __attribute__((aligned(16))) float l_w[(LW_FLOATS + 3) / 4 * 4];
    __shared__ __attribute__((aligned(16))) float l_parts[kMaxParts * kLdsPartStride];
    __shared__ __attribute__((aligned(16))) float l_canon[kMaxParts * kLdsCanonStride];
    __shared__ double l_acc[kWaves * kMaxParts * kRec];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = a.P, H = a.H, W = a.W;
    const int b = blockIdx.y, blk = blockIdx.x;

    // ---- staging: part frames, dense weights out of the pack's MFMA operand order (enarf_grad.h), zeroed wave sums
    stage_frames(l_parts, l_canon, a.parts + (size_t)b * P * kPartStride, a.canonical_pose, P, tid, kBlock);
    const float *pf = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.mlp_pack) + (size_t)b * kPackBytes);
    stage_dense_weights(l_w, pf, tid, kBlock);
    for (int e = tid; e < kWaves * P * kRec; e += kBlock) l_acc[e] = 0.0;
    __syncthreads();

    const long long i = (long long)blk * kBlock + tid;
    const bool live = i < a.N;
    const float *pts = a.points + (size_t)b * 3 * a.N;
    const float px = live ? pts[i] : 0.0f, py = live ? pts[a.N + i] : 0.0f, pz = live ? pts[2 * a.N + i] : 0.0f;

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
    if (live) {
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
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                float qx, qy;
                plane_xy(pl, cx, cy, cz, qx, qy);
                const GTaps t = grad_taps(qx, qy, H, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 *v = reinterpret_cast<const f32x4 *>(featp + (pl * plane + (size_t)t.o[j]) * kFeat);
#pragma unroll
                    for (int c4 = 0; c4 < kFeat / 4; ++c4) {
                        const f32x4 q = v[c4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[4 * c4 + r] += q[r] * t.w[j];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kFeat; ++c) feat[c] += acc[c] * w;
        }
    }

    // ---- the MLP forward and backward: gf = dL / d feature, g_wm = dL / d (the largest weight)
    float gf[kFeat], g_wm = 0.0f;
#pragma unroll
    for (int c = 0; c < kFeat; ++c) gf[c] = 0.0f;
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
        float z3[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) z3[o] = l_w[LW_B3 + o];
#pragma unroll
        for (int j = 0; j < kHid; ++j) {
            s2 |= (uint64_t)(z2[j] > 0.0f) << j;
            const float h = styled_act(z2[j]);
#pragma unroll
            for (int o = 0; o < 4; ++o) z3[o] += l_w[LW_W3 + o * kHid + j] * h;
        }
        // heads (triplane_nerf.py:44-47): tanh colour; the density's ReLU with its own backward rule (activation.py:12-16)
        const float *gdp = a.g_density ? a.g_density + (size_t)b * a.N : nullptr;
        const float *gcp = a.g_color ? a.g_color + (size_t)b * 3 * a.N : nullptr;
        float gz3[4];
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const float col = tanhf(styled_act(z3[o]));
            const float g = gcp ? gcp[(size_t)o * a.N + i] : 0.0f;
            gz3[o] = g * (1.0f - col * col) * act_slope(z3[o] > 0.0f);
        }
        {
            const float h = styled_act(z3[3]);
            const float gd = gdp ? gdp[i] : 0.0f;
            float factor = 10.0f;
            if (a.multiply_density_with_weight) {
                // the factor max w over ALL parts, an invalid one weighs 0.125 (density_head in enarf_march.h); its
                // gradient goes to the part that has it, nowhere when that is an invalid part or every weight is 1 / P
                const bool invalid_wins = !uniform && __popc(bits) < P && !(wmax >= 0.125f);
                const float wm = uniform ? uniform_w : invalid_wins ? 0.125f : wmax;
                factor = 10.0f * wm;
                if (!uniform && !invalid_wins) g_wm = gd * (10.0f * fmaxf(h, 0.0f));
            }
            const float gr = gd * factor;
            const float gh = (h >= 0.0f) ? gr : (gr < 0.0f) ? 0.1f * gr : 0.0f;
            gz3[3] = gh * act_slope(z3[3] > 0.0f);
        }
#pragma unroll
        for (int j = 0; j < kHid; ++j) {                    // dL / d z2, in place
            float g = 0.0f;
#pragma unroll
            for (int o = 0; o < 4; ++o) g += l_w[LW_W3 + o * kHid + j] * gz3[o];
            z2[j] = g * act_slope((s2 >> j) & 1);
        }
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

    // ---- walk 2: each valid part's gradient at its canonical point, chained to the point and to the part's record
    float gpx = 0.0f, gpy = 0.0f, gpz = 0.0f;
    for (int k = 0; k < P; ++k) {
        const bool v = (bits >> k) & 1u;
        if (__ballot(v) == 0) continue;                     // wave-uniform: no lane of this wave is in part k
        float r[kRec];
#pragma unroll
        for (int e = 0; e < kRec; ++e) r[e] = 0.0f;
        if (v) {
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
            float Gc[3] = {0.0f, 0.0f, 0.0f}, e_f = 0.0f;   // e_f = gf . f_k, the gradient that reaches w_k
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                float qx, qy;
                plane_xy(pl, cx, cy, cz, qx, qy);
                const GTaps t = grad_taps(qx, qy, H, W);
                float ga = 0.0f, gb = 0.0f;
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
                    ga += dot * t.wx[j];
                    gb += dot * t.wy[j];
                }
                Gc[pl] += w * ga;
                Gc[(pl + 1) % 3] += w * gb;
            }
            if (!uniform) {
                const float gw = e_f + (k == kmax ? g_wm : 0.0f);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    float qx, qy;
                    plane_xy(pl, cx, cy, cz, qx, qy);
                    const GTaps t = grad_taps(qx, qy, H, W);
                    const float *mp = maskp + (size_t)(3 * k + pl) * plane;
                    float ma = 0.0f, mb = 0.0f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float m = mp[t.o[j]];
                        ma += m * t.wx[j];
                        mb += m * t.wy[j];
                    }
                    const float f = gw * (w * (1.0f - sg[pl]));     // dw_k / dm_p = w_k (1 - s_p), clamped or not
                    Gc[pl] += f * ma;
                    Gc[(pl + 1) % 3] += f * mb;
                }
            }
            const float d0 = px - F[9], d1 = py - F[10], d2 = pz - F[11];
            const float dq0 = (Cn[0] * Gc[0] + Cn[3] * Gc[1]) + Cn[6] * Gc[2];      // Rc^T G_c
            const float dq1 = (Cn[1] * Gc[0] + Cn[4] * Gc[1]) + Cn[7] * Gc[2];
            const float dq2 = (Cn[2] * Gc[0] + Cn[5] * Gc[1]) + Cn[8] * Gc[2];
            const float dl0 = F[12] * dq0, dl1 = F[12] * dq1, dl2 = F[12] * dq2;
            const float dd0 = (F[0] * dl0 + F[1] * dl1) + F[2] * dl2;               // R dl
            const float dd1 = (F[3] * dl0 + F[4] * dl1) + F[5] * dl2;
            const float dd2 = (F[6] * dl0 + F[7] * dl1) + F[8] * dl2;
            gpx += dd0; gpy += dd1; gpz += dd2;
            r[0] = d0 * dl0; r[1] = d0 * dl1; r[2] = d0 * dl2;
            r[3] = d1 * dl0; r[4] = d1 * dl1; r[5] = d1 * dl2;
            r[6] = d2 * dl0; r[7] = d2 * dl1; r[8] = d2 * dl2;
            r[9] = -dd0; r[10] = -dd1; r[11] = -dd2;
            r[12] = (lx * dq0 + ly * dq1) + lz * dq2;
        }
#pragma unroll
        for (int e = 0; e < kRec; ++e) {
            double x = (double)r[e];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
            if (lane == 0) l_acc[(wave * P + k) * kRec + e] = x;
        }
    }
    if (live) {
        float *gp = a.g_points + (size_t)b * 3 * a.N;
        gp[i] = gpx; gp[a.N + i] = gpy; gp[2 * a.N + i] = gpz;
    }
    __syncthreads();
    double *ws = reinterpret_cast<double *>(a.workspace) + ((size_t)b * nblk + blk) * (size_t)(P * kRec);
    for (int e = tid; e < P * kRec; e += kBlock)
        ws[e] = ((l_acc[e] + l_acc[P * kRec + e]) + l_acc[2 * P * kRec + e]) + l_acc[3 * P * kRec + e];
}

// grid (P, B): thread (chunk = tid / 16, entry = tid % 16) adds the partials chunk, chunk + 16, ... in ascending order, then
// the 16 chunk sums are added in ascending order
__global__ void __launch_bounds__(kBlock) pgrad_finish_kernel(const double *__restrict__ ws, float *__restrict__ g_parts,
                                                              const int P, const int nblk) {
    __shared__ double red[16][16];
    const int tid = threadIdx.x, e = tid & 15, chunk = tid >> 4, k = blockIdx.x, b = blockIdx.y;
    double acc = 0.0;
    if (e < kRec) {
        const double *src = ws + (size_t)b * nblk * (size_t)(P * kRec) + (size_t)k * kRec + e;
        for (int blk = chunk; blk < nblk; blk += 16) acc += src[(size_t)blk * (size_t)(P * kRec)];
    }
    red[chunk][e] = acc;
    __syncthreads();
    if (tid < 16) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) s += red[c][tid];
        g_parts[((size_t)b * P + k) * kPartStride + tid] = (tid < kRec) ? (float)s : 0.0f;
    }
}

// 0 when the sizes are taken, else the failure to return
int check_sizes(const char *who, int B, int P, long long N) {
    if (B < 1 || N < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: B %d, N %lld", who, B, N);
    if (P < 1 || P > kMaxParts) return enarf::host::fail(ENARF_ERR_ARG, "%s: %d parts outside [1, %d]", who, P, kMaxParts);
    if (B > 65535 || N / kBlock + 1 >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: B %d above 65535 or N %lld needs 2^31 workgroups", who, B, N);
    return 0;
}

}  // namespace

extern "C" {

int enarf_pgrad_abi_version(void) { return ENARF_PGRAD_ABI_VERSION; }

const char *enarf_pgrad_last_error(void) { return enarf::host::last_error(); }

size_t enarf_pgrad_workspace_bytes(int32_t B, int32_t P, int64_t N) {
    if (check_sizes("enarf_pgrad_workspace_bytes", B, P, (long long)N) || N == 0) return 0;
    const size_t nblk = (size_t)((N + kBlock - 1) / kBlock);
    return enarf::host::align256((size_t)B * nblk * (size_t)P * kRec * sizeof(double));
}

int enarf_pgrad_query(const enarf_pgrad_query_args *args, void *stream) {
    const char *who = "enarf_pgrad_query";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_pgrad_query_args &a = *args;
    if (const int e = check_sizes(who, a.B, a.P, (long long)a.N)) return e;
    if (const int e = enarf::host::check_part_planes(who, a.P, kMaxParts, a.H, a.W)) return e;
    if (96LL * a.H * a.W >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: planes %d x %d: 96 H W must stay below 2^31 floats", who, a.H, a.W);
    if (a.feat_batch_stride < 0 || a.mask_batch_stride < 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: negative batch strides", who);
    if (!a.g_parts) return enarf::host::fail(ENARF_ERR_ARG, "%s: null g_parts", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.N == 0) {
        const hipError_t e = hipMemsetAsync(a.g_parts, 0, (size_t)a.B * a.P * kPartStride * sizeof(float), s);
        if (e != hipSuccess) return enarf::host::fail((int)e, "%s: clearing g_parts failed: %s", who, hipGetErrorString(e));
        return 0;
    }
    if (!a.points || !a.parts || !a.canonical_pose || !a.feat_cl || (!a.mask_planes && !a.uniform_part_weight) || !a.mlp_pack ||
        !a.g_points || !a.workspace)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null points, parts, canonical_pose, feat_cl, mask_planes, mlp_pack, g_points or workspace", who);
    if (((uintptr_t)a.feat_cl & 15) || ((a.feat_batch_stride * 4) & 15) || ((uintptr_t)a.workspace & 7))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: feat_cl must be 16-byte aligned per image, the workspace 8-byte aligned", who);
    const int nblk = (int)((a.N + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pgrad_query_kernel, dim3((unsigned)nblk, (unsigned)a.B), dim3(kBlock), 0, s, a, nblk);
    if (const int e = enarf::host::check_launch("enarf_pgrad_query: pgrad_query_kernel")) return e;
    hipLaunchKernelGGL(pgrad_finish_kernel, dim3((unsigned)a.P, (unsigned)a.B), dim3(kBlock), 0, s,
                       reinterpret_cast<const double *>(a.workspace), a.g_parts, a.P, nblk);
    return enarf::host::check_launch("enarf_pgrad_query: pgrad_finish_kernel");
}

}  // extern "C"
