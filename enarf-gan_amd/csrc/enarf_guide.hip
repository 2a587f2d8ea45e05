// enarf_guide.hip - the mask-guidance loss of the GAN path (libenarf_guide.so, include/enarf_guide.h).
//
// The N mask values are cut into consecutive chunks, one workgroup of 256 threads each; a thread walks its chunk in
// rows of 256 (element = chunk start + 256 * row + thread), so a thread's terms come in index order.
//
// Forward. guide_hist_kernel runs once per 8-bit digit of the order-preserving key, most significant first: a workgroup
// first resolves the digits already known from the earlier passes' global histograms (a 256-wide scan per pass, the same
// in every workgroup), then counts the digit of its chunk's values that match that prefix in an LDS histogram and adds
// its non-empty bins to the pass's global histogram (integer atomics: order-independent). guide_sum_kernel resolves all
// four digits (T = the k-th smallest key, Q = how many values equal to T belong to the k smallest) and, per chunk, adds
// m^2 over key < T and (1 - m)^2 over the on-bone pixels in fp64 and counts the values with key == T and the on-bone
// pixels. guide_finish_kernel (one workgroup) adds the partials in index order, deals Q over the chunks from the left
// (the lowest flat indices win a tie), and stores the three fp32 results and the state of the backward.
//
// Backward. guide_bwd_kernel, one workgroup per chunk: an element is selected when key < T, or key == T and fewer than
// the chunk's share of tied values precede it in the chunk (a 256-wide scan per row, only in the one chunk whose share
// is neither nothing nor everything).
#include "enarf_guide.h"
#include "enarf_device.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

using enarf::block_sum;

constexpr int kBlock = 256;
constexpr int kMaxBlocks = ENARF_GUIDE_MAX_BLOCKS;
constexpr int kPasses = ENARF_GUIDE_PASSES;
constexpr int kBins = 1 << ENARF_GUIDE_RADIX_BITS;
static_assert(kBins == kBlock, "one thread per histogram bin");
static_assert(kPasses * ENARF_GUIDE_RADIX_BITS == 32, "the passes cover the key");
static_assert(kMaxBlocks % kBlock == 0, "the finish deals whole runs of chunks to its threads");

struct Geometry {
    long long N, chunk_len;
    int chunks;
};

Geometry geometry_of(long long N) {
    long long blocks0 = (N + kBlock - 1) / kBlock;
    if (blocks0 > kMaxBlocks) blocks0 = kMaxBlocks;
    const long long per = (N + blocks0 - 1) / blocks0;
    const long long chunk_len = (per + kBlock - 1) / kBlock * kBlock;
    return Geometry{N, chunk_len, (int)((N + chunk_len - 1) / chunk_len)};
}

// scratch of the forward (ENARF_GUIDE_WORK_BYTES)
struct Work {
    double push[kMaxBlocks], bone[kMaxBlocks];
    unsigned int hist[kPasses][kBins];
    int ties[kMaxBlocks], n_bone[kMaxBlocks];
};
static_assert(sizeof(Work) == ENARF_GUIDE_WORK_BYTES, "ENARF_GUIDE_WORK_BYTES is the size of Work");

struct Args {
    const float *fake, *bone;
    long long N, chunk_len, k;
    int s, S, rate, with_push;
    double coef;
};

__device__ __forceinline__ unsigned int key_of(float v) {
    const unsigned int b = __float_as_uint(v);
    if (v != v) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned int key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// whether pixel i of the (B, s, s) mask lies under the (B, S, S) bone mask max-pooled by rate and thresholded
__device__ __forceinline__ bool on_bone(const Args &a, long long i) {
    if (a.rate == 1 && a.S == a.s) return a.bone[i] > 0.5f;
    const long long ss = (long long)a.s * a.s;
    const long long b = i / ss;
    const int r = (int)(i - b * ss), y = r / a.s, x = r - y * a.s;
    const float *p = a.bone + (b * a.S + (long long)y * a.rate) * a.S + (long long)x * a.rate;
    bool any = false, nan = false;
    for (int dy = 0; dy < a.rate; ++dy)
        for (int dx = 0; dx < a.rate; ++dx) {
            const float v = p[(long long)dy * a.S + dx];
            any |= v > 0.5f;
            nan |= v != v;
        }
    return any && !nan;
}

// inclusive prefix sum over the workgroup's 256 threads in thread order; `tot` holds 4 counters
__device__ __forceinline__ unsigned int block_scan(unsigned int v, unsigned int *tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    __syncthreads();                                    // the previous call's readers are done with `tot`
    if (lane == 63) tot[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += tot[w];
    return v;
}

struct Select {
    unsigned int tot[4];
    unsigned int bin, rest;
};

// the leading `passes` digits of the k-th smallest key from the global histograms, and k's rank among the values that
// share them (0 for k == 0: nothing is selected and the prefix stays 0). Every thread of the workgroup calls it.
__device__ __forceinline__ void resolve(const unsigned int (*hist)[kBins], int passes, unsigned int k, Select &sh,
                                        unsigned int &prefix, unsigned int &rest) {
    prefix = 0u, rest = k;
    for (int p = 0; p < passes; ++p) {
        const unsigned int v = hist[p][threadIdx.x];
        const unsigned int incl = block_scan(v, sh.tot);
        if (threadIdx.x == 0) sh.bin = 0u, sh.rest = 0u;
        __syncthreads();
        if (v > 0u && incl >= rest && incl - v < rest) sh.bin = threadIdx.x, sh.rest = rest - (incl - v);
        __syncthreads();
        prefix = (prefix << ENARF_GUIDE_RADIX_BITS) | sh.bin, rest = sh.rest;
        __syncthreads();                                // before the next pass resets sh.bin
    }
}

__global__ __launch_bounds__(kBlock) void guide_hist_kernel(Args a, int pass, Work *w) {
    __shared__ Select sh;
    __shared__ unsigned int local[kBins];
    unsigned int prefix, rest;
    resolve(w->hist, pass, (unsigned int)a.k, sh, prefix, rest);
    local[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 32 - ENARF_GUIDE_RADIX_BITS * (pass + 1);
    const long long begin = (long long)blockIdx.x * a.chunk_len;
    for (long long off = threadIdx.x; off < a.chunk_len; off += kBlock) {
        const long long i = begin + off;
        if (i >= a.N) break;
        const unsigned int key = key_of(a.fake[i]);
        if (pass == 0 || (key >> (shift + ENARF_GUIDE_RADIX_BITS)) == prefix) atomicAdd(&local[(key >> shift) & (kBins - 1)], 1u);
    }
    __syncthreads();
    const unsigned int n = local[threadIdx.x];
    if (n) atomicAdd(&w->hist[pass][threadIdx.x], n);
}

__global__ __launch_bounds__(kBlock) void guide_sum_kernel(Args a, Work *w, int *state) {
    __shared__ Select sh;
    __shared__ double red[4];
    unsigned int T = 0u, Q = 0u;
    if (a.with_push) resolve(w->hist, kPasses, (unsigned int)a.k, sh, T, Q);
    double push = 0.0, bone = 0.0;
    unsigned int ties = 0u, n_bone = 0u;
    const long long begin = (long long)blockIdx.x * a.chunk_len;
    for (long long off = threadIdx.x; off < a.chunk_len; off += kBlock) {
        const long long i = begin + off;
        if (i >= a.N) break;
        const float m = a.fake[i];
        if (a.with_push) {
            const unsigned int key = key_of(m);
            if (key < T) push += (double)m * (double)m;
            ties += key == T;
        }
        if (on_bone(a, i)) {
            const double d = 1.0 - (double)m;
            bone += d * d;
            ++n_bone;
        }
    }
    push = block_sum(push, red);
    bone = block_sum(bone, red);
    // integer sums: any order gives the same value
    const unsigned int ties_all = block_scan(ties, sh.tot), bone_all = block_scan(n_bone, sh.tot);
    if (threadIdx.x == kBlock - 1) {
        w->push[blockIdx.x] = push, w->bone[blockIdx.x] = bone;
        w->ties[blockIdx.x] = (int)ties_all, w->n_bone[blockIdx.x] = (int)bone_all;
        if (blockIdx.x == 0) state[0] = (int)T, state[1] = (int)Q;
    }
}

__global__ __launch_bounds__(kBlock) void guide_finish_kernel(Args a, int chunks, const Work *w, int *state, float *out) {
    __shared__ Select sh;
    __shared__ double red[4];
    double push = 0.0, bone = 0.0;
    unsigned int n_bone = 0u;
    for (int c = threadIdx.x; c < chunks; c += kBlock) push += w->push[c], bone += w->bone[c], n_bone += (unsigned int)w->n_bone[c];
    push = block_sum(push, red);
    bone = block_sum(bone, red);
    n_bone = block_scan(n_bone, sh.tot);
    __syncthreads();
    if (threadIdx.x == kBlock - 1) sh.bin = n_bone;
    __syncthreads();
    n_bone = sh.bin;
    // deal the Q selected ties over the chunks from the left: a thread owns kMaxBlocks / 256 consecutive chunks
    constexpr int kRun = kMaxBlocks / kBlock;
    const unsigned int Q = (unsigned int)state[1];
    unsigned int mine = 0u;
    for (int j = 0; j < kRun; ++j) {
        const int c = threadIdx.x * kRun + j;
        if (c < chunks) mine += (unsigned int)w->ties[c];
    }
    unsigned int before = block_scan(mine, sh.tot) - mine;
    for (int j = 0; j < kRun; ++j) {
        const int c = threadIdx.x * kRun + j;
        if (c >= chunks) break;
        const unsigned int n = (unsigned int)w->ties[c];
        const unsigned int left = Q > before ? Q - before : 0u;
        state[4 + c] = left >= n ? -1 : (int)left;      // -1: every tied value of the chunk is selected
        before += n;
    }
    if (threadIdx.x == 0) {
        double p = 0.0;
        if (a.with_push) {
            if (Q > 0u) {
                const double t = (double)value_of((unsigned int)state[0]);
                push += (double)Q * (t * t);
            }
            p = push / (double)a.k;
        }
        const double b = bone / (double)n_bone;
        out[0] = (float)((p + b) * a.coef), out[1] = (float)p, out[2] = (float)b;
        state[2] = (int)n_bone, state[3] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void guide_bwd_kernel(Args a, const int *state, const float *up, float *d_fake) {
    __shared__ unsigned int tot[4];
    const unsigned int T = (unsigned int)state[0];
    const int share = a.with_push ? state[4 + blockIdx.x] : 0;
    const double g = (double)*up * a.coef * 2.0;
    const double g_push = g / (double)a.k, g_bone = g / (double)state[2];
    const long long begin = (long long)blockIdx.x * a.chunk_len;
    unsigned int before = 0u;                           // tied values of the chunk in the rows above
    for (long long off = threadIdx.x; off < a.chunk_len; off += kBlock) {   // whole rows: the scan needs every thread
        const long long i = begin + off;
        const bool live = i < a.N;
        const float m = live ? a.fake[i] : 0.0f;
        const unsigned int key = key_of(m);
        const bool tie = live && a.with_push && key == T;
        bool selected = live && a.with_push && key < T;
        if (share < 0) {
            selected |= tie;
        } else if (share > 0) {
            const unsigned int incl = block_scan(tie ? 1u : 0u, tot);
            selected |= tie && before + incl <= (unsigned int)share;
            __syncthreads();
            before += tot[0] + tot[1] + tot[2] + tot[3];
        }
        if (live) {
            const double d_push = selected ? g_push * (double)m : 0.0;
            const double d_bone = (g_bone * -(1.0 - (double)m)) * (on_bone(a, i) ? 1.0 : 0.0);
            d_fake[i] = (float)(d_push + d_bone);
        }
    }
}

int check_args(const char *who, const float *fake, const float *bone, int64_t B, int s, int S, int64_t k, int with_push,
               Args *a, Geometry *g) {
    if (B < 1 || s < 1)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: an empty mask (B %lld, s %d): N == 0 is refused", who, (long long)B, s);
    if (S < s)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: bone mask side %d below the mask's %d: a rate of 0", who, S, s);
    const int rate = S / s;
    if (S / rate != s)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: a %d x %d bone mask pooled by %d is %d x %d, not the mask's %d x %d",
                                 who, S, S, rate, S / rate, S / rate, s, s);
    if (B >= (1LL << 31) || (long long)B * s >= (1LL << 31) || (long long)B * s * s >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: B %lld x %d x %d values: N must stay below 2^31", who, (long long)B, s, s);
    const long long N = (long long)B * s * s;
    if (with_push && (k < 0 || k > N))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: k %lld outside [0, N = %lld]", who, (long long)k, N);
    if (!fake || !bone) return enarf::host::fail(ENARF_ERR_ARG, "%s: null fake_mask or bone_mask", who);
    *g = geometry_of(N);
    *a = Args{fake, bone, N, g->chunk_len, with_push ? (long long)k : 0, s, S, rate, with_push != 0, 0.0};
    return 0;
}

}  // namespace

extern "C" {

int enarf_guide_abi_version(void) { return ENARF_GUIDE_ABI_VERSION; }

const char *enarf_guide_last_error(void) { return enarf::host::last_error(); }

int enarf_guide_loss_fwd(const float *fake_mask, const float *bone_mask, int64_t B, int s, int S, int64_t k,
                         int with_push, double coef, void *work, int32_t *state, float *out, void *stream) {
    const char *who = "enarf_guide_loss_fwd";
    Args a;
    Geometry g;
    if (const int rc = check_args(who, fake_mask, bone_mask, B, s, S, k, with_push, &a, &g)) return rc;
    if (!work || !state || !out) return enarf::host::fail(ENARF_ERR_ARG, "%s: null work, state or out", who);
    if (reinterpret_cast<uintptr_t>(work) % 8) return enarf::host::fail(ENARF_ERR_ARG, "%s: work is not 8-byte aligned", who);
    a.coef = coef;
    Work *w = static_cast<Work *>(work);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.with_push) {
        const hipError_t e = hipMemsetAsync(w->hist, 0, sizeof(w->hist), st);
        if (e != hipSuccess) return enarf::host::fail((int)e, "%s: memset failed: %s", who, hipGetErrorString(e));
        for (int pass = 0; pass < kPasses; ++pass) {
            hipLaunchKernelGGL(guide_hist_kernel, dim3((unsigned)g.chunks), dim3(kBlock), 0, st, a, pass, w);
            if (const int rc = enarf::host::check_launch("enarf_guide_loss_fwd: guide_hist_kernel")) return rc;
        }
    }
    hipLaunchKernelGGL(guide_sum_kernel, dim3((unsigned)g.chunks), dim3(kBlock), 0, st, a, w, state);
    if (const int rc = enarf::host::check_launch("enarf_guide_loss_fwd: guide_sum_kernel")) return rc;
    hipLaunchKernelGGL(guide_finish_kernel, dim3(1), dim3(kBlock), 0, st, a, g.chunks, w, state, out);
    return enarf::host::check_launch("enarf_guide_loss_fwd: guide_finish_kernel");
}

int enarf_guide_loss_bwd(const float *fake_mask, const float *bone_mask, int64_t B, int s, int S, int64_t k,
                         int with_push, double coef, const int32_t *state, const float *up, float *d_fake_mask,
                         void *stream) {
    const char *who = "enarf_guide_loss_bwd";
    Args a;
    Geometry g;
    if (const int rc = check_args(who, fake_mask, bone_mask, B, s, S, k, with_push, &a, &g)) return rc;
    if (!state || !up || !d_fake_mask) return enarf::host::fail(ENARF_ERR_ARG, "%s: null state, up or d_fake_mask", who);
    a.coef = coef;
    hipLaunchKernelGGL(guide_bwd_kernel, dim3((unsigned)g.chunks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a,
                       state, up, d_fake_mask);
    return enarf::host::check_launch("enarf_guide_loss_bwd: guide_bwd_kernel");
}

}  // extern "C"
