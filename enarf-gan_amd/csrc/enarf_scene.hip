// enarf_scene.hip - libenarf_scene.so: several avatars marched on the same rays, composed into one image (gfx950 / CDNA4
// only, wave64). The contract is in include/enarf_scene.h.
//
//   scene_composite_kernel<kPer>   one wavefront (one workgroup of 64 lanes) per (frame, ray), one launch for all frames;
//                           a lane owns kPer = 1, 2, 4 or 8 breakpoints (K Nf <= 64 kPer: 53, 64, 114 and 138 VGPRs, so the
//                           usual two avatars of 64 samples run at 8 waves a SIMD and only the cap at 3).
//     1 load and screen     avatar by avatar, lane i takes sample i (and i + 64): a ballot finds a value the contract
//                           rejects, a wave max-scan makes the depths a running maximum; depths, densities and colours
//                           of the ray go to LDS.
//     2 merge by ranking    element e = k Nf + i (lane e mod 64): its position among all breakpoints is i plus, for every
//                           other avatar, the number of that avatar's breakpoints ordered before it - a binary search in
//                           the avatar's list in LDS (<= for a lower avatar index, < for a higher one: the key (depth,
//                           avatar, sample)). The same counts are every avatar's active interval on the segment that
//                           starts at the breakpoint; they are kept packed, a byte an avatar.
//     3 optical depth       sigma of the segment from the active intervals, the next breakpoint from the merged list in
//                           LDS, tau scattered to LDS in merged order; an exclusive prefix sum there (a lane takes
//                           consecutive positions serially, a Hillis-Steele scan across the lanes).
//     4 weights and sums    w = exp(-prefix) (-expm1(-tau)); each lane adds its elements in order, then fixed butterflies
//                           across the wave; lane 0 stores the ray's outputs.
//   No atomics and no dependence on timing: two runs give identical bits. Everything is fp64 from the stored fp32 with
//   FMA contraction off, so the float64 restatement of the contract (tests/scene_reference.py) is matched to the rounding
//   of the stored fp32. LDS: 32 bytes a breakpoint, at most 16 KiB a wavefront, sized by the launch.
#include "enarf_scene.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kWave = 64;
constexpr int kMaxK = ENARF_SCENE_MAX_AVATARS;
constexpr int kMaxNf = ENARF_SCENE_MAX_SAMPLES;
constexpr int kMaxM = ENARF_SCENE_MAX_MERGED;
constexpr int kMaxPer = kMaxM / kWave;               // elements a lane owns at most
constexpr long long kMaxRays = 1LL << 31;
constexpr int kBytesPerBreakpoint = 8 + 6 * 4;       // tau fp64; D, s, 3 c, merged t fp32

__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, kWave);      // both partners form the same sum
    return v;
}

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

// kPer: elements a lane owns, K Nf <= 64 kPer (1, 2, 4 or 8: the short lists keep fewer registers and more waves)
template <int kPer>
__global__ void __launch_bounds__(kWave) scene_composite_kernel(const enarf_scene_composite_args a) {
#pragma clang fp contract(off)
    extern __shared__ double s_mem[];
    const int lane = threadIdx.x, K = a.K, Nf = a.Nf, KNf = K * Nf;
    const long long ray = blockIdx.x;                                   // < F n, checked on the host
    const int f = (int)(ray / a.n), r = (int)(ray - (long long)f * a.n);
    double *s_tau = s_mem;                                              // [KNf] merged order: tau, then its prefix
    float *s_D = reinterpret_cast<float *>(s_mem + KNf);                // [KNf] running-maximum depths, avatar by avatar
    float *s_S = s_D + KNf;                                             // [KNf] densities
    float *s_C = s_S + KNf;                                             // [3][KNf] colours
    float *s_T = s_C + 3 * KNf;                                         // [KNf] merged breakpoints

    // ---- 1: load, screen, running maximum -----------------------------------------------------------------------------
    unsigned part = 0u, skipped = 0u;                                   // wave-uniform bit masks over the avatars
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
        if (bad) skipped |= 1u << k;
        else part |= 1u << k;
    }
    const int M = __popc(part) * Nf;
    const long long mbase = ray * KNf;                                  // of t, source and weight
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
        if (a.out_t) a.out_t[mbase + p] = d;
        if (a.out_source) a.out_source[mbase + p] = e;
    }
    for (int p = M + lane; p < KNf; p += kWave) {                       // the padding behind the M breakpoints
        if (a.out_t) a.out_t[mbase + p] = HUGE_VALF;
        if (a.out_source) a.out_source[mbase + p] = -1;
        if (a.out_weight) a.out_weight[mbase + p] = 0.0f;
    }
    __syncthreads();

    // ---- 3: tau in merged order and its exclusive prefix sum ---------------------------------------------------------------
    const double scale = (double)a.render_scale;
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        if (pos[m] < 0) continue;
        const double t0 = (double)s_T[pos[m]];
        const double t1 = pos[m] + 1 < M ? (double)s_T[pos[m] + 1] : t0;
        tau[m] = (tau[m] * (t1 - t0)) * scale;
        s_tau[pos[m]] = tau[m];
    }
    __syncthreads();
    {
        const int per = (M + kWave - 1) / kWave, j0 = lane * per;      // this lane's consecutive positions
        double run = 0.0;
        for (int q = 0; q < per; ++q)
            if (j0 + q < M) run = run + s_tau[j0 + q];
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
            const double x = s_tau[j0 + q];
            s_tau[j0 + q] = run;
            run = run + x;
        }
    }
    __syncthreads();

    // ---- 4: weights, the lane's sums in element order, the wave's sums ---------------------------------------------------
    double mask = 0.0, disparity = 0.0, colour[3] = {0.0, 0.0, 0.0}, mass[kMaxK];
#pragma unroll
    for (int o = 0; o < kMaxK; ++o) mass[o] = 0.0;
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        if (pos[m] < 0) continue;
        const double w = exp(-s_tau[pos[m]]) * -expm1(-tau[m]);
        if (a.out_weight) a.out_weight[mbase + pos[m]] = (float)w;
        double s_act[kMaxK], sigma = 0.0, num[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int o = 0; o < kMaxK; ++o) {
            s_act[o] = 0.0;
            const int cnt = (int)((act[m] >> (8 * o)) & 0xFFull);
            if (o < K && cnt > 0) {
                const int e = o * Nf + cnt - 1;
                s_act[o] = (double)s_S[e];
                sigma = sigma + s_act[o];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) num[ch] = num[ch] + s_act[o] * (double)s_C[ch * KNf + e];
            }
        }
        mask = mask + w;
        disparity = disparity + w / (double)s_T[pos[m]];
        if (sigma > 0.0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) colour[ch] = colour[ch] + w * (num[ch] / sigma);
#pragma unroll
            for (int o = 0; o < kMaxK; ++o) mass[o] = mass[o] + w * (s_act[o] / sigma);
        }
    }
    mask = wave_sum(mask);
    disparity = wave_sum(disparity);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) colour[ch] = wave_sum(colour[ch]);
#pragma unroll
    for (int o = 0; o < kMaxK; ++o)
        if (o < K) mass[o] = wave_sum(mass[o]);
    if (lane != 0) return;

    const long long pix = (long long)f * a.n + r;
    if (a.out_mask) a.out_mask[pix] = (float)mask;
    if (a.out_disparity) a.out_disparity[pix] = (float)disparity;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        if (a.out_color) a.out_color[((long long)f * 3 + ch) * a.n + r] = (float)colour[ch];
    int best = 0;
    double best_mass = mass[0];
#pragma unroll
    for (int o = 1; o < kMaxK; ++o)
        if (o < K && mass[o] > best_mass) best = o, best_mass = mass[o];
#pragma unroll
    for (int o = 0; o < kMaxK; ++o)
        if (o < K && a.out_instance_mass) a.out_instance_mass[((long long)f * K + o) * a.n + r] = (float)mass[o];
    if (a.out_instance) a.out_instance[pix] = (part != 0u && (float)mask >= a.threshold) ? best : -1;
    if (a.out_skipped) a.out_skipped[pix] = (int32_t)skipped;
}

}  // namespace

extern "C" {

int enarf_scene_abi_version(void) { return ENARF_SCENE_ABI_VERSION; }

const char *enarf_scene_last_error(void) { return enarf::host::last_error(); }

int enarf_scene_composite(const enarf_scene_composite_args *args, void *stream) {
    const char *who = "enarf_scene_composite";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_scene_composite_args &a = *args;
    if (a.K < 1 || a.K > kMaxK)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: %d avatars outside [1, %d]", who, a.K, kMaxK);
    if (a.Nf < 2 || a.Nf > kMaxNf)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: %d samples a ray outside [2, %d]", who, a.Nf, kMaxNf);
    if (a.K * a.Nf > kMaxM)
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: %d avatars of %d samples are %d breakpoints a ray, more than %d", who,
                                 a.K, a.Nf, a.K * a.Nf, kMaxM);
    if (a.F < 0 || a.n < 0 || (long long)a.F * a.n >= kMaxRays)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: F = %d frames of n = %d rays: F, n >= 0 and F n < 2^31", who, a.F, a.n);
    if (!a.out_color && !a.out_mask && !a.out_disparity && !a.out_instance_mass && !a.out_instance && !a.out_skipped &&
        !a.out_t && !a.out_source && !a.out_weight)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: no output asked for", who);
    const long long rays = (long long)a.F * a.n;
    if (rays == 0) return 0;
    if (!a.depth || !a.density || !a.color) return enarf::host::fail(ENARF_ERR_ARG, "%s: null depth, density or color", who);
    const size_t lds = (size_t)a.K * a.Nf * kBytesPerBreakpoint;
    const int merged = a.K * a.Nf;
    const dim3 grid((unsigned)rays), block(kWave);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (merged <= kWave) hipLaunchKernelGGL(scene_composite_kernel<1>, grid, block, lds, s, a);
    else if (merged <= 2 * kWave) hipLaunchKernelGGL(scene_composite_kernel<2>, grid, block, lds, s, a);
    else if (merged <= 4 * kWave) hipLaunchKernelGGL(scene_composite_kernel<4>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(scene_composite_kernel<kMaxPer>, grid, block, lds, s, a);
    return enarf::host::check_launch("enarf_scene_composite: scene_composite_kernel");
}

}  // extern "C"
