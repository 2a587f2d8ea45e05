// enarf_sgrad.hip - libenarf_sgrad.so: the gradient of the multi-avatar composite with respect to the avatars' densities and
// colours (gfx950 / CDNA4 only, wave64). The contract is in include/enarf_sgrad.h.
//
//   sgrad_composite_bwd_kernel<kPer>   one wavefront (one workgroup of 64 lanes) per (frame, ray), one launch for all
//                           frames; a lane owns kPer = 1, 2, 4 or 8 breakpoints (K Nf <= 64 kPer).
//     1 load and screen     as the forward (enarf_scene.hip, restated here, not shared: the forward's bits do not depend
//     2 merge by ranking    on this file): avatar by avatar the ray's samples go to LDS with the depths a running maximum;
//     3 optical depth       element e = k Nf + i finds its position among all breakpoints by binary searches in the other
//                           avatars' lists and, from the same counts, every avatar's active interval on the segment it
//                           starts; tau goes to LDS in merged order and becomes its exclusive prefix sum. The position of
//                           every element is kept in LDS as well: a sample's run ends where the avatar's next one starts.
//     4 segment terms       u_j and r_j per segment; u_j r_j to LDS in merged order and, in place, its exclusive suffix
//                           sum S_j (a lane takes consecutive positions serially, a Hillis-Steele scan across the lanes,
//                           as the prefix); then E_j + u_j h_j replaces S_j and u_j replaces the prefix.
//     5 runs                the lane that owns element (k, i) adds E_j + u_j h_j and u_j over its run directly, in
//                           ascending j (no difference of prefix sums: a far sample's run is many orders smaller than
//                           the prefix before it), and stores the sample's four gradients with plain stores. Samples
//                           that get no gradient (a last sample, an avatar that takes no part) store zeros.
//   No atomics and no dependence on timing: two runs give identical bits. Everything is fp64 from the stored fp32 with
//   FMA contraction off. LDS: 44 bytes a breakpoint (the forward's 32, a second fp64 array and the positions) and 64 bytes
//   for the upstream instance-mass gradients: at most 22592 bytes a wavefront, sized by the launch.
#include "enarf_sgrad.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kWave = 64;
constexpr int kMaxK = ENARF_SGRAD_MAX_AVATARS;
constexpr int kMaxNf = ENARF_SGRAD_MAX_SAMPLES;
constexpr int kMaxM = ENARF_SGRAD_MAX_MERGED;
constexpr int kMaxPer = kMaxM / kWave;               // elements a lane owns at most
constexpr long long kMaxRays = 1LL << 31;
// 44, where the forward (enarf_scene.hip) has 8 + 6 * 4 = 32: u and E + u h fp64; D, s, 3 c, merged t fp32; position int32
constexpr int kBytesPerBreakpoint = 2 * 8 + 6 * 4 + 4;
constexpr int kBytesPerRay = kMaxK * 8;                  // the upstream instance-mass gradients, fp64

// number of the Nf ascending values of `list` that are < d, or <= d with `or_equal`
__device__ __forceinline__ int count_before(const float *list, int Nf, float d, bool or_equal) {
    int lo = 0, hi = Nf;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float x = list[mid];
        if (or_equal ? x <= d : x < d) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// kPer: elements a lane owns, K Nf <= 64 kPer (1, 2, 4 or 8)
template <int kPer>
__global__ void __launch_bounds__(kWave) sgrad_composite_bwd_kernel(const enarf_sgrad_composite_bwd_args a) {
#pragma clang fp contract(off)
    extern __shared__ double s_mem[];
    const int lane = threadIdx.x, K = a.K, Nf = a.Nf, KNf = K * Nf;
    const long long ray = blockIdx.x;                                   // < F n, checked on the host
    const int f = (int)(ray / a.n), r = (int)(ray - (long long)f * a.n);
    double *s_gI = s_mem;                                               // [kMaxK] upstream instance-mass gradients
    double *s_U = s_mem + kMaxK;                                        // [KNf] merged order: tau, its prefix, then u
    double *s_G = s_U + KNf;                                            // [KNf] merged order: u r, its suffix, then E + u h
    float *s_D = reinterpret_cast<float *>(s_G + KNf);                  // [KNf] running-maximum depths, avatar by avatar
    float *s_S = s_D + KNf;                                             // [KNf] densities
    float *s_C = s_S + KNf;                                             // [3][KNf] colours
    float *s_T = s_C + 3 * KNf;                                         // [KNf] merged breakpoints
    int *s_P = reinterpret_cast<int *>(s_T + KNf);                      // [KNf] position of every element

    const long long pix = (long long)f * a.n + r;
    const double gM = a.g_mask ? (double)a.g_mask[pix] : 0.0, gD = a.g_disparity ? (double)a.g_disparity[pix] : 0.0;
    double gC[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) gC[ch] = a.g_color ? (double)a.g_color[((long long)f * 3 + ch) * a.n + r] : 0.0;
    if (lane < kMaxK)
        s_gI[lane] = (lane < K && a.g_instance_mass) ? (double)a.g_instance_mass[((long long)f * K + lane) * a.n + r] : 0.0;

    // ---- 1: load, screen, running maximum -----------------------------------------------------------------------------
    unsigned part = 0u;                                                 // wave-uniform bit mask over the avatars
    for (int k = 0; k < K; ++k) {
        const long long img = (long long)f * K + k;
        if (a.valid && a.valid[img * a.n + r] == 0) continue;
        const long long base = (img * a.n + r) * Nf, cbase = (img * 3 * a.n + r) * Nf, cstride = (long long)a.n * Nf;
        bool bad = false;
        float carry = -HUGE_VALF;
        for (int c0 = 0; c0 < Nf; c0 += kWave) {
            const int i = c0 + lane;
            const bool in = i < Nf;
            float d = 1.0f, s = 0.0f, c[3] = {0.0f, 0.0f, 0.0f};
            if (in) {
                d = a.depth[base + i];
                s = a.density[base + i];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch] = a.color[cbase + ch * cstride + i];
            }
            const bool reject = !(isfinite(d) && isfinite(s) && isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) &&
                                  d > 0.0f && s >= 0.0f);
            bad = bad || __ballot(reject) != 0ull;
            float m = in ? d : -HUGE_VALF;
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const float up = __shfl_up(m, off, kWave);
                if (lane >= off) m = fmaxf(m, up);
            }
            m = fmaxf(m, carry);
            carry = __shfl(m, kWave - 1, kWave);
            if (in) {
                const int e = k * Nf + i;
                s_D[e] = m;
                s_S[e] = s;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) s_C[ch * KNf + e] = c[ch];
            }
        }
        if (!bad) part |= 1u << k;
    }
    const int M = __popc(part) * Nf;
    __syncthreads();

    // ---- 2: the position of every breakpoint, the active intervals and sigma of the segment it starts ---------------------
    int pos[kPer];
    unsigned long long act[kPer];             // byte k: 1 + the active interval of avatar k, 0 without one
    double tau[kPer];                         // sigma first, then tau
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        const int e = lane + kWave * m;
        pos[m] = -1, act[m] = 0ull, tau[m] = 0.0;
        if (e >= KNf) continue;
        const int k = e / Nf, i = e - k * Nf;
        if (!((part >> k) & 1u)) continue;
        const float d = s_D[e];
        int p = i;
        double sigma = 0.0;
        unsigned long long packed = 0ull;
        for (int o = 0; o < K; ++o) {
            if (!((part >> o) & 1u)) continue;
            int cnt = i + 1;
            if (o != k) {
                cnt = count_before(s_D + o * Nf, Nf, d, o < k);
                p += cnt;
            }
            if (cnt >= 1 && cnt <= Nf - 1) {                           // interval cnt - 1 in [0, Nf - 2]
                packed |= (unsigned long long)cnt << (8 * o);
                sigma = sigma + (double)s_S[o * Nf + cnt - 1];
            }
        }
        pos[m] = p, act[m] = packed, tau[m] = sigma;
        s_T[p] = d;
        s_P[e] = p;
    }
    __syncthreads();

    // ---- 3: tau in merged order and its exclusive prefix sum ---------------------------------------------------------------
    const double scale = (double)a.render_scale;
    double len[kPer];                         // a_j
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        len[m] = 0.0;
        if (pos[m] < 0) continue;
        const double t0 = (double)s_T[pos[m]];
        const double t1 = pos[m] + 1 < M ? (double)s_T[pos[m] + 1] : t0;
        len[m] = (t1 - t0) * scale;
        tau[m] = (tau[m] * (t1 - t0)) * scale;
        s_U[pos[m]] = tau[m];
    }
    __syncthreads();
    const int per = (M + kWave - 1) / kWave, j0 = lane * per;          // this lane's consecutive positions, both scans
    {
        double run = 0.0;
        for (int q = 0; q < per; ++q)
            if (j0 + q < M) run = run + s_U[j0 + q];
        double incl = run;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const double up = __shfl_up(incl, off, kWave);
            if (lane >= off) incl = up + incl;
        }
        const double before = __shfl_up(incl, 1, kWave);
        run = lane == 0 ? 0.0 : before;
        for (int q = 0; q < per; ++q) {
            if (j0 + q >= M) break;
            const double x = s_U[j0 + q];
            s_U[j0 + q] = run;
            run = run + x;
        }
    }
    __syncthreads();

    // ---- 4: u and r of every segment; S, the exclusive suffix sum of u r; E + u h ------------------------------------------
    double tev[kPer], uv[kPer], uh[kPer];     // T exp(-tau) v, u v, u h
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        tev[m] = 0.0, uv[m] = 0.0, uh[m] = 0.0;
        if (pos[m] < 0) continue;
        const int p = pos[m];
        const double T = exp(-s_U[p]);
        double sigma = 0.0, num[3] = {0.0, 0.0, 0.0}, mass = 0.0;
#pragma unroll
        for (int o = 0; o < kMaxK; ++o) {
            const int cnt = (int)((act[m] >> (8 * o)) & 0xFFull);
            if (o < K && cnt > 0) {
                const int e = o * Nf + cnt - 1;
                const double s = (double)s_S[e];
                sigma = sigma + s;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) num[ch] = num[ch] + s * (double)s_C[ch * KNf + e];
                mass = mass + s_gI[o] * s;
            }
        }
        const double h = gM + gD / (double)s_T[p];
        const double rr = (((gC[0] * num[0] + gC[1] * num[1]) + gC[2] * num[2]) + sigma * h) + mass;
        double u;
        if (sigma > 0.0) {
            u = (T * -expm1(-tau[m])) / sigma;
            const double v = rr / sigma;
            tev[m] = (T * exp(-tau[m])) * v;
            uv[m] = u * v;
        } else {
            u = T * len[m];
        }
        if (p == M - 1) u = 0.0;                                        // the last breakpoint starts no segment
        uh[m] = u * h;
        s_U[p] = u;
        s_G[p] = u * rr;
    }
    __syncthreads();
    {
        double run = 0.0;
        for (int q = per - 1; q >= 0; --q)
            if (j0 + q < M) run = run + s_G[j0 + q];
        double incl = run;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const double down = __shfl_down(incl, off, kWave);
            if (lane + off < kWave) incl = incl + down;
        }
        const double after = __shfl_down(incl, 1, kWave);
        run = lane == kWave - 1 ? 0.0 : after;
        for (int q = per - 1; q >= 0; --q) {
            if (j0 + q >= M) continue;
            const double x = s_G[j0 + q];
            s_G[j0 + q] = run;
            run = run + x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        if (pos[m] < 0) continue;
        const double S = s_G[pos[m]];                                   // read and replaced by the lane that owns it
        s_G[pos[m]] = (len[m] * (tev[m] - S) - uv[m]) + uh[m];
    }
    __syncthreads();

    // ---- 5: every sample's run, summed in ascending j; the stores ---------------------------------------------------------
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        const int e = lane + kWave * m;
        if (e >= KNf) continue;
        const int k = e / Nf, i = e - k * Nf;
        double gd = 0.0, gc[3] = {0.0, 0.0, 0.0};
        if (pos[m] >= 0 && i < Nf - 1) {
            const int end = s_P[e + 1];                                 // (k, i + 1): the same avatar, so it takes part
            double sum_g = 0.0, sum_u = 0.0;
            for (int j = pos[m]; j < end; ++j) {
                sum_g = sum_g + s_G[j];
                sum_u = sum_u + s_U[j];
            }
            const double s = (double)s_S[e];
            double dot = 0.0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                dot = dot + gC[ch] * (double)s_C[ch * KNf + e];
                gc[ch] = (gC[ch] * s) * sum_u;
            }
            gd = sum_g + (dot + s_gI[k]) * sum_u;
        }
        const long long img = (long long)f * K + k;
        if (a.g_density) a.g_density[(img * a.n + r) * Nf + i] = (float)gd;
        if (a.g_sample_color) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) a.g_sample_color[((img * 3 + ch) * a.n + r) * Nf + i] = (float)gc[ch];
        }
    }
}

}  // namespace

extern "C" {

int enarf_sgrad_abi_version(void) { return ENARF_SGRAD_ABI_VERSION; }

const char *enarf_sgrad_last_error(void) { return enarf::host::last_error(); }

int enarf_sgrad_composite_bwd(const enarf_sgrad_composite_bwd_args *args, void *stream) {
    const char *who = "enarf_sgrad_composite_bwd";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_sgrad_composite_bwd_args &a = *args;
    if (a.K < 1 || a.K > kMaxK)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: %d avatars outside [1, %d]", who, a.K, kMaxK);
    if (a.Nf < 2 || a.Nf > kMaxNf)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: %d samples a ray outside [2, %d]", who, a.Nf, kMaxNf);
    if (a.K * a.Nf > kMaxM)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: %d avatars of %d samples are %d breakpoints a ray, more than %d", who,
                                 a.K, a.Nf, a.K * a.Nf, kMaxM);
    if (a.F < 0 || a.n < 0 || (long long)a.F * a.n >= kMaxRays)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: F = %d frames of n = %d rays: F, n >= 0 and F n < 2^31", who, a.F, a.n);
    if (!a.g_color && !a.g_mask && !a.g_disparity && !a.g_instance_mass)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: no upstream gradient given", who);
    if (!a.g_density && !a.g_sample_color) return enarf::host::fail(ENARF_ERR_ARG, "%s: no output asked for", who);
    const long long rays = (long long)a.F * a.n;
    if (rays == 0) return 0;
    if (!a.depth || !a.density || !a.color) return enarf::host::fail(ENARF_ERR_ARG, "%s: null depth, density or color", who);
    const size_t lds = (size_t)a.K * a.Nf * kBytesPerBreakpoint + kBytesPerRay;
    const int merged = a.K * a.Nf;
    const dim3 grid((unsigned)rays), block(kWave);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (merged <= kWave) hipLaunchKernelGGL(sgrad_composite_bwd_kernel<1>, grid, block, lds, s, a);
    else if (merged <= 2 * kWave) hipLaunchKernelGGL(sgrad_composite_bwd_kernel<2>, grid, block, lds, s, a);
    else if (merged <= 4 * kWave) hipLaunchKernelGGL(sgrad_composite_bwd_kernel<4>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(sgrad_composite_bwd_kernel<kMaxPer>, grid, block, lds, s, a);
    return enarf::host::check_launch("enarf_sgrad_composite_bwd: sgrad_composite_bwd_kernel");
}

}  // extern "C"
