// enarf_geom.hip - libenarf_geom.so: geometry buffers of a march and the running depth error of an evaluation set
// (gfx950 / CDNA4 only, wave64). The contract is in include/enarf_geom.h.
//
//   geom_buffers_kernel      one lane per pixel, 16 x 16 pixel tiles, one launch per batch: the (disparity, mask) of the
//                            pixel and of its four neighbours become depths and camera-space points, the differences of
//                            the usable neighbours a screen-space normal, and depth, points, normals, flags and the 8-bit
//                            shape image are written. No atomics, no LDS, no workspace: the 5-point stencil is served by
//                            the cache, and no address is formed from a neighbour outside the image.
//   geom_err_partial_kernel  one record of partial sums per workgroup (squared inverse-depth error over all pixels and
//                            over the target's foreground, silhouette intersection and union), a fixed tree in LDS.
//   geom_err_finish_kernel   one workgroup: the records added in index order, then added to the state.
// Everything is fp64 from the fp32 inputs with FMA contraction off, as in enarf_raster.hip and enarf_paint.hip, so the
// float64 restatement of the contract (tests/geom_reference.py) is matched to the rounding of the stored fp32.
#include "enarf_geom.h"
#include "enarf_device.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

using enarf::level;

constexpr int kTile = 16;
constexpr int kBlock = 256;
constexpr int kMaxSize = ENARF_GEOM_MAX_SIZE;
constexpr long long kMaxCount = 1LL << 31;
constexpr int kWords = ENARF_GEOM_STATE_WORDS;
constexpr int kPerLane = 8;              // pixels a lane takes before another workgroup is added

struct Sample {
    bool valid;
    double z, p[3];
};

// depth and point of pixel (r, c) of image b; (r, c) must be inside the image
__device__ __forceinline__ Sample sample_at(const enarf_geom_buffers_args &a, const float *K, long long base, int r, int c) {
#pragma clang fp contract(off)
    const long long i = base + (long long)r * a.W + c;
    const float q = a.disparity[i], m = a.mask[i];
    Sample s;
    s.valid = isfinite(q) && isfinite(m) && m >= a.mask_threshold && q > 0.0f;
    s.z = 0.0;
    if (s.valid) s.z = a.normalise ? (double)a.depth_scale * ((double)m / (double)q) : (double)a.depth_scale / (double)q;
    const double x = (double)a.x0 + ((double)c + 0.5) * (double)a.step;
    const double y = (double)a.y0 + ((double)r + 0.5) * (double)a.step;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        s.p[k] = s.z * (((double)K[3 * k] * x + (double)K[3 * k + 1] * y) + (double)K[3 * k + 2]);
    return s;
}

__device__ __forceinline__ bool usable(const Sample &n, double z, double edge) {
#pragma clang fp contract(off)
    if (!n.valid) return false;
    return edge < 0.0 || fabs(n.z - z) <= edge * z;
}

// the difference along one axis: `lo` at c - 1 (r - 1), `hi` at c + 1 (r + 1); false when neither neighbour is usable
__device__ __forceinline__ bool difference(const Sample &lo, bool use_lo, const Sample &me, const Sample &hi, bool use_hi,
                                           double d[3]) {
#pragma clang fp contract(off)
    if (!use_lo && !use_hi) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (use_hi ? hi.p[k] : me.p[k]) - (use_lo ? lo.p[k] : me.p[k]);
    return true;
}

__global__ void __launch_bounds__(kBlock) geom_buffers_kernel(const enarf_geom_buffers_args a) {
#pragma clang fp contract(off)
    const int tiles_x = (a.W + kTile - 1) / kTile, tiles_y = (a.H + kTile - 1) / kTile;
    const long long tile = blockIdx.x;
    const int b = (int)(tile / ((long long)tiles_x * tiles_y));
    const int t = (int)(tile - (long long)b * tiles_x * tiles_y);
    const int r = (t / tiles_x) * kTile + (int)threadIdx.x / kTile, c = (t % tiles_x) * kTile + (int)threadIdx.x % kTile;
    if (b >= a.B || r >= a.H || c >= a.W) return;
    const long long base = (long long)b * a.H * a.W, i = base + (long long)r * a.W + c;
    const float *K = a.inv_intrinsics + (a.KB > 1 ? 9LL * b : 0LL);
    const Sample me = sample_at(a, K, base, r, c);

    double N[3] = {0.0, 0.0, 0.0};
    bool has_normal = false;
    if (me.valid && (a.normals || a.flags || (a.image && a.shade != ENARF_GEOM_SHADE_DEPTH))) {
        const double edge = (double)a.edge;
        Sample left = me, right = me, up = me, down = me;
        bool use_l = false, use_r = false, use_u = false, use_d = false;
        if (c > 0) { left = sample_at(a, K, base, r, c - 1); use_l = usable(left, me.z, edge); }
        if (c + 1 < a.W) { right = sample_at(a, K, base, r, c + 1); use_r = usable(right, me.z, edge); }
        if (r > 0) { up = sample_at(a, K, base, r - 1, c); use_u = usable(up, me.z, edge); }
        if (r + 1 < a.H) { down = sample_at(a, K, base, r + 1, c); use_d = usable(down, me.z, edge); }
        double dx[3], dy[3];
        const bool has_dx = difference(left, use_l, me, right, use_r, dx);
        const bool has_dy = difference(up, use_u, me, down, use_d, dy);
        if (has_dx && has_dy) {
            const double n0 = dy[1] * dx[2] - dy[2] * dx[1];
            const double n1 = dy[2] * dx[0] - dy[0] * dx[2];
            const double n2 = dy[0] * dx[1] - dy[1] * dx[0];
            const double l = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            if (l > 0.0 && l < HUGE_VAL) {
                has_normal = true;
                N[0] = n0 / l, N[1] = n1 / l, N[2] = n2 / l;
                if ((N[0] * me.p[0] + N[1] * me.p[1]) + N[2] * me.p[2] > 0.0) N[0] = -N[0], N[1] = -N[1], N[2] = -N[2];
            }
        }
    }

    if (a.depth) a.depth[i] = (float)me.z;
    if (a.flags) a.flags[i] = (uint8_t)((me.valid ? ENARF_GEOM_FLAG_VALID : 0) | (has_normal ? ENARF_GEOM_FLAG_NORMAL : 0));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (a.points) a.points[3 * i + k] = (float)me.p[k];
        if (a.normals) a.normals[3 * i + k] = (float)N[k];
    }
    if (a.image) {
        double v[3] = {(double)a.background[0], (double)a.background[1], (double)a.background[2]};
        if (a.shade == ENARF_GEOM_SHADE_NORMAL && has_normal) {
            v[0] = 0.5 + 0.5 * N[0];
            v[1] = 0.5 + 0.5 * -N[1];
            v[2] = 0.5 + 0.5 * -N[2];
        } else if (a.shade == ENARF_GEOM_SHADE_LIT && has_normal) {
            const double dp = fmax(sqrt((me.p[0] * me.p[0] + me.p[1] * me.p[1]) + me.p[2] * me.p[2]), 1e-6);
            const double cs = -((N[0] * me.p[0] + N[1] * me.p[1]) + N[2] * me.p[2]) / dp;
            double spec = 0.0;
            if (cs > 0.0) {
                spec = fmax(2.0 * cs * cs - 1.0, 0.0);
#pragma unroll
                for (int k = 0; k < 6; ++k) spec *= spec;                  // ^64
            }
            v[0] = v[1] = v[2] = (0.5 + 0.3 * (cs > 0.0 ? cs : 0.0)) + 0.2 * spec;
        } else if (a.shade == ENARF_GEOM_SHADE_DEPTH && me.valid) {
            const double inv_far = 1.0 / (double)a.far_depth;
            v[0] = v[1] = v[2] = (1.0 / me.z - inv_far) / (1.0 / (double)a.near_depth - inv_far);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.image[3 * i + k] = level(v[k]);
    }
}

struct ErrSums {
    double sse_all, sse_fg;
    long long n_fg, inter, uni;
};

__global__ void __launch_bounds__(kBlock) geom_err_partial_kernel(const float *__restrict__ disparity,
                                                                   const float *__restrict__ mask,
                                                                   const float *__restrict__ target, long long n,
                                                                   float mask_threshold, long long *__restrict__ workspace) {
#pragma clang fp contract(off)
    __shared__ double s_all[kBlock], s_fg[kBlock];
    __shared__ long long s_nfg[kBlock], s_inter[kBlock], s_uni[kBlock];
    const int t = threadIdx.x;
    ErrSums e = {0.0, 0.0, 0, 0, 0};
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + t; i < n; i += stride) {
        const float q = disparity[i], g = target[i];
        const double d = (double)q - (double)g, sq = d * d;
        const bool fg = g > 0.0f;
        const bool sil = mask ? mask[i] >= mask_threshold : q > 0.0f;
        e.sse_all = e.sse_all + sq;
        if (fg) e.sse_fg = e.sse_fg + sq;
        e.n_fg += fg;
        e.inter += sil && fg;
        e.uni += sil || fg;
    }
    s_all[t] = e.sse_all, s_fg[t] = e.sse_fg, s_nfg[t] = e.n_fg, s_inter[t] = e.inter, s_uni[t] = e.uni;
    __syncthreads();
    for (int s = kBlock / 2; s >= 1; s >>= 1) {
        if (t < s) {
            s_all[t] = s_all[t] + s_all[t + s];
            s_fg[t] = s_fg[t] + s_fg[t + s];
            s_nfg[t] += s_nfg[t + s];
            s_inter[t] += s_inter[t + s];
            s_uni[t] += s_uni[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        long long *rec = workspace + (long long)blockIdx.x * kWords;
        rec[0] = 0;
        rec[1] = __double_as_longlong(s_all[0]);
        rec[2] = s_nfg[0];
        rec[3] = __double_as_longlong(s_fg[0]);
        rec[4] = s_inter[0];
        rec[5] = s_uni[0];
        rec[6] = 0;
        rec[7] = 0;
    }
}

// lane w < 8 owns word w of the records and of the state: words 1 and 3 are fp64 sums, the others int64
__global__ void __launch_bounds__(64) geom_err_finish_kernel(const long long *__restrict__ workspace, int records, long long n,
                                                             long long *__restrict__ state) {
#pragma clang fp contract(off)
    const int w = threadIdx.x;
    if (w >= kWords) return;
    if (w == 1 || w == 3) {
        double sum = 0.0;
        for (int k = 0; k < records; ++k) sum = sum + __longlong_as_double(workspace[(long long)k * kWords + w]);
        state[w] = __double_as_longlong(__longlong_as_double(state[w]) + sum);
    } else {
        long long sum = w == 0 ? n : w == 6 ? 1 : 0;
        for (int k = 0; k < records; ++k) sum += workspace[(long long)k * kWords + w];
        if (w != 7) state[w] += sum;
    }
}

long long err_records(long long n) {
    if (n < 1 || n >= kMaxCount) return 0;
    const long long per_group = (long long)kBlock * kPerLane;
    const long long g = (n + per_group - 1) / per_group;
    return g < ENARF_GEOM_MAX_RECORDS ? g : ENARF_GEOM_MAX_RECORDS;
}

}  // namespace

extern "C" {

int enarf_geom_abi_version(void) { return ENARF_GEOM_ABI_VERSION; }

const char *enarf_geom_last_error(void) { return enarf::host::last_error(); }

int enarf_geom_buffers(const enarf_geom_buffers_args *args, void *stream) {
    const char *who = "enarf_geom_buffers";
    if (!args) return enarf::host::fail(ENARF_ERR_ARG, "%s: null args", who);
    const enarf_geom_buffers_args &a = *args;
    if (a.H < 1 || a.H > kMaxSize || a.W < 1 || a.W > kMaxSize)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: image size %d x %d outside [1, %d]", who, a.H, a.W, kMaxSize);
    if (a.B < 1 || (long long)a.B * a.H * a.W >= kMaxCount)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: B = %d with %d x %d pixels: B H W must lie in [1, 2^31)", who, a.B, a.H, a.W);
    if (a.KB != 1 && a.KB != a.B)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: %d inv_intrinsics for a batch of %d (1 or B)", who, a.KB, a.B);
    if (a.shade < ENARF_GEOM_SHADE_NORMAL || a.shade > ENARF_GEOM_SHADE_DEPTH)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: shade mode %d outside [0, 2]", who, a.shade);
    if (a.image && a.shade == ENARF_GEOM_SHADE_DEPTH && !(a.near_depth > 0.0f && a.far_depth > 0.0f && a.near_depth != a.far_depth))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: the depth shade takes near > 0, far > 0, near != far, got %g and %g", who,
                                 (double)a.near_depth, (double)a.far_depth);
    if (!a.disparity || !a.mask || !a.inv_intrinsics)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null disparity, mask or inv_intrinsics", who);
    if (!a.depth && !a.points && !a.normals && !a.flags && !a.image)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: no output asked for", who);
    const long long tiles = (long long)a.B * ((a.H + kTile - 1) / kTile) * ((a.W + kTile - 1) / kTile);   // <= B H W < 2^31
    hipLaunchKernelGGL(geom_buffers_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return enarf::host::check_launch("enarf_geom_buffers: geom_buffers_kernel");
}

int64_t enarf_geom_err_records(int64_t n) { return err_records((long long)n); }

int enarf_geom_err_update(const float *disparity, const float *mask, const float *target, int64_t n, float mask_threshold,
                          void *workspace, int64_t workspace_records, void *state, void *stream) {
    const char *who = "enarf_geom_err_update";
    const long long records = err_records((long long)n);
    if (records == 0) return enarf::host::fail(ENARF_ERR_ARG, "%s: n = %lld outside [1, 2^31)", who, (long long)n);
    if (!disparity || !target || !workspace || !state)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null disparity, target, workspace or state", who);
    if (workspace_records < records)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: a workspace of %lld records, %lld needed", who, (long long)workspace_records,
                                 records);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(geom_err_partial_kernel, dim3((unsigned)records), dim3(kBlock), 0, s, disparity, mask, target,
                       (long long)n, mask_threshold, static_cast<long long *>(workspace));
    int rc = enarf::host::check_launch("enarf_geom_err_update: geom_err_partial_kernel");
    if (rc != 0) return rc;
    hipLaunchKernelGGL(geom_err_finish_kernel, dim3(1), dim3(64), 0, s, static_cast<const long long *>(workspace), (int)records,
                       (long long)n, static_cast<long long *>(state));
    return enarf::host::check_launch("enarf_geom_err_update: geom_err_finish_kernel");
}

}  // extern "C"
