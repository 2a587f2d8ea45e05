// enarf_raster.hip - hard-Phong rasterisation of one device-resident mesh (libenarf_raster.so, include/enarf_raster.h).
//
// One call, eight launches (and four fills of the workspace), no host synchronisation:
//   raster_project_kernel  per vertex: the pixel-space position (u / s, v / s) in fp64 and z;
//   raster_depth_kernel    per triangle: the pixel centres of its clipped bounding box; a covered centre does one 64-bit
//                          atomicMin of key = (fp32 bits of zbuf) << 32 | triangle id into the R x R key buffer (all
//                          ones = empty). zbuf > 0, so the bits order like the value; min is order-free, so the winner
//                          needs no sort. A box above kBigPixels is listed instead (one integer atomic) for
//   raster_big_kernel      a workgroup per listed triangle, striding over its box (a full-screen triangle on one lane
//                          would serialise the launch);
//   raster_mark_kernel     per pixel: the winner's vertices get a compact slot (a claim by compare-and-swap, then a slot
//                          counter); only these vertices' normals are ever needed;
//   raster_count_kernel    per triangle: the number of incident faces of every slotted vertex;
//   raster_scan_kernel     one block: exclusive int64 offsets of those counts;
//   raster_fill_kernel     per triangle: the incident face ids into each slotted vertex's list (arrival order);
//   raster_vnormal_kernel  per slot: the list sorted by face id (so the sum has the contract's order, whatever the
//                          arrival order was), the area-weighted normal summed in fp64 and normalised;
//   raster_shade_kernel    per pixel: the key decoded, b' and zbuf recomputed by the same device function the depth
//                          pass ran (zbuf has exactly the key's bits), the normal interpolated, Phong, every output.
// Geometry is fp64 throughout, with FMA contraction off in the functions both passes share. Every result is a function
// of the inputs alone: keys by min, slots only name storage, lists are sorted before they are summed.
#include "enarf_raster.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

using enarf::host::align256;

constexpr int kBlock = 256;
constexpr int kBigPixels = 256;       // a bounding box above this many pixel centres goes to raster_big_kernel
constexpr int kBigBlocks = 1024;
constexpr int kScanThreads = 1024;
constexpr int kMaxR = 4096;
constexpr long long kMaxCount = 1LL << 31;
constexpr unsigned long long kEmpty = ~0ull;

struct Layout {
    long long cap;                    // slots: at most min(V, 3 R^2) vertices belong to a winning triangle
    size_t pxy, pz, keys, slot, ctr, big, svert, cnt, off, nrm, list, bytes;
};

inline Layout layout(long long V, long long T, int R) {
    Layout l;
    const long long px = (long long)R * R;
    l.cap = V < 3 * px ? V : 3 * px;
    l.pxy = 0;
    l.pz = align256(l.pxy + 16 * (size_t)V);
    l.keys = align256(l.pz + 4 * (size_t)V);
    l.slot = align256(l.keys + 8 * (size_t)px);
    l.ctr = align256(l.slot + 4 * (size_t)V);
    l.big = l.ctr + 256;
    l.svert = align256(l.big + 4 * (size_t)T);
    l.cnt = align256(l.svert + 4 * (size_t)l.cap);
    l.off = align256(l.cnt + 4 * (size_t)l.cap);
    l.nrm = align256(l.off + 8 * (size_t)(l.cap + 1));
    l.list = align256(l.nrm + 24 * (size_t)l.cap);
    l.bytes = align256(l.list + 12 * (size_t)T);
    return l;
}

__device__ __forceinline__ long long gid() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ void __launch_bounds__(kBlock)
raster_project_kernel(const float *__restrict__ verts, long long V, const float *__restrict__ K, double s,
                      double2 *__restrict__ pxy, float *__restrict__ pz) {
#pragma clang fp contract(off)
    const long long i = gid();
    if (i >= V) return;
    const double x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    pxy[i] = make_double2((fx * x / z + cx) / s, (fy * y / z + cy) / s);
    pz[i] = verts[3 * i + 2];
}

struct Tri {
    double x[3], y[3], z[3], area;
};

// false when the triangle is not drawn: an index outside [0, V), a vertex with z <= 0 or not finite, zero area
__device__ __forceinline__ bool load_tri(const int64_t *__restrict__ tris, long long t, long long V,
                                         const double2 *__restrict__ pxy, const float *__restrict__ pz, Tri &tr) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long v = tris[3 * t + k];
        if (v < 0 || v >= V) return false;
        const double2 p = pxy[v];
        const float z = pz[v];
        if (!(z > 0.0f) || !isfinite(z) || !isfinite(p.x) || !isfinite(p.y)) return false;
        tr.x[k] = p.x;
        tr.y[k] = p.y;
        tr.z[k] = z;
    }
    tr.area = (tr.x[1] - tr.x[0]) * (tr.y[2] - tr.y[0]) - (tr.y[1] - tr.y[0]) * (tr.x[2] - tr.x[0]);
    return tr.area != 0.0 && isfinite(tr.area);
}

// the pixel-centre range that can be covered, clipped to the screen; false when empty. Conservative: cover() decides.
__device__ __forceinline__ bool box(const Tri &tr, int R, int &c0, int &c1, int &r0, int &r1) {
    const double xl = fmin(tr.x[0], fmin(tr.x[1], tr.x[2])), xh = fmax(tr.x[0], fmax(tr.x[1], tr.x[2]));
    const double yl = fmin(tr.y[0], fmin(tr.y[1], tr.y[2])), yh = fmax(tr.y[0], fmax(tr.y[1], tr.y[2]));
    const double cl = fmax(floor(xl - 0.5), 0.0), ch = fmin(ceil(xh - 0.5), R - 1.0);
    const double rl = fmax(floor(yl - 0.5), 0.0), rh = fmin(ceil(yh - 0.5), R - 1.0);
    if (!(cl <= ch) || !(rl <= rh)) return false;
    c0 = (int)cl, c1 = (int)ch, r0 = (int)rl, r1 = (int)rh;
    return true;
}

// the one coverage / depth function of the depth and shade passes: at centre (x, y), b_i = w_i / area (all > 0 to
// cover), b'_i = (b_i / z_i) / S, zbuf = 1 / S
__device__ __forceinline__ bool cover(const Tri &tr, double x, double y, double bp[3], double &zb) {
#pragma clang fp contract(off)
    const double w0 = (tr.x[1] - x) * (tr.y[2] - y) - (tr.y[1] - y) * (tr.x[2] - x);
    const double w1 = (tr.x[2] - x) * (tr.y[0] - y) - (tr.y[2] - y) * (tr.x[0] - x);
    const double w2 = (tr.x[0] - x) * (tr.y[1] - y) - (tr.y[0] - y) * (tr.x[1] - x);
    // b_i > 0 needs w_i of the area's sign: reject there before any division
    if (tr.area > 0.0 ? !(w0 > 0.0 && w1 > 0.0 && w2 > 0.0) : !(w0 < 0.0 && w1 < 0.0 && w2 < 0.0)) return false;
    const double b0 = w0 / tr.area, b1 = w1 / tr.area, b2 = w2 / tr.area;
    if (!(b0 > 0.0 && b1 > 0.0 && b2 > 0.0)) return false;
    const double q0 = b0 / tr.z[0], q1 = b1 / tr.z[1], q2 = b2 / tr.z[2];
    const double S = q0 + q1 + q2;
    zb = 1.0 / S;
    bp[0] = q0 / S;
    bp[1] = q1 / S;
    bp[2] = q2 / S;
    return true;
}

__device__ __forceinline__ void raster_pixel(const Tri &tr, long long t, int r, int c, int R,
                                             unsigned long long *__restrict__ keys) {
    double bp[3], zb;
    if (!cover(tr, c + 0.5, r + 0.5, bp, zb)) return;
    const unsigned long long key = (unsigned long long)__float_as_uint((float)zb) << 32 | (unsigned long long)t;
    atomicMin(keys + (size_t)r * R + c, key);
}

__global__ void __launch_bounds__(kBlock)
raster_depth_kernel(const int64_t *__restrict__ tris, long long T, long long V, const double2 *__restrict__ pxy,
                    const float *__restrict__ pz, int R, unsigned long long *__restrict__ keys, int *__restrict__ nbig,
                    int *__restrict__ big) {
    const long long t = gid();
    if (t >= T) return;
    Tri tr;
    int c0, c1, r0, r1;
    if (!load_tri(tris, t, V, pxy, pz, tr) || !box(tr, R, c0, c1, r0, r1)) return;
    if ((long long)(c1 - c0 + 1) * (r1 - r0 + 1) > kBigPixels) {
        big[atomicAdd(nbig, 1)] = (int)t;              // at most one entry per triangle: the list holds T
        return;
    }
    for (int r = r0; r <= r1; ++r)
        for (int c = c0; c <= c1; ++c) raster_pixel(tr, t, r, c, R, keys);
}

__global__ void __launch_bounds__(kBlock)
raster_big_kernel(const int64_t *__restrict__ tris, long long V, const double2 *__restrict__ pxy,
                  const float *__restrict__ pz, int R, unsigned long long *__restrict__ keys,
                  const int *__restrict__ nbig, const int *__restrict__ big) {
    const int n = *nbig;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const long long t = big[i];
        Tri tr;
        int c0, c1, r0, r1;
        if (!load_tri(tris, t, V, pxy, pz, tr) || !box(tr, R, c0, c1, r0, r1)) continue;
        const int w = c1 - c0 + 1;
        const long long npx = (long long)w * (r1 - r0 + 1);
        for (long long p = threadIdx.x; p < npx; p += blockDim.x)
            raster_pixel(tr, t, r0 + (int)(p / w), c0 + (int)(p % w), R, keys);
    }
}

__global__ void __launch_bounds__(kBlock)
raster_mark_kernel(const unsigned long long *__restrict__ keys, long long npx, const int64_t *__restrict__ tris,
                   int *__restrict__ slot, int *__restrict__ nslots, int *__restrict__ svert, long long cap) {
    const long long p = gid();
    if (p >= npx) return;
    const unsigned long long key = keys[p];
    if (key == kEmpty) return;
    const long long t = (long long)(key & 0xFFFFFFFFull);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long v = tris[3 * t + k];           // a drawn triangle: in range
        if (atomicCAS(slot + v, -1, -2) == -1) {        // the first claim names the slot; later kernels read it
            const int s = atomicAdd(nslots, 1);
            if (s < cap) {
                slot[v] = s;
                svert[s] = (int)v;
            }
        }
    }
}

// the three vertex ids of triangle t, false when one is outside [0, V) (such a face has no normal)
__device__ __forceinline__ bool tri_ids(const int64_t *__restrict__ tris, long long t, long long V, long long v[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = tris[3 * t + k];
        if (v[k] < 0 || v[k] >= V) return false;
    }
    return true;
}

__global__ void __launch_bounds__(kBlock)
raster_count_kernel(const int64_t *__restrict__ tris, long long T, long long V, const int *__restrict__ slot,
                    int *__restrict__ cnt) {
    const long long t = gid();
    long long v[3];
    if (t >= T || !tri_ids(tris, t, V, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int s = slot[v[k]];
        if (s >= 0) atomicAdd(cnt + s, 1);
    }
}

// one block: cnt[0, n) -> off[0, n] exclusive (off[n] = the total), n = the slot count
__global__ void __launch_bounds__(kScanThreads)
raster_scan_kernel(const int *__restrict__ cnt, const int *__restrict__ nslots, long long cap, long long *__restrict__ off) {
    __shared__ long long part[kScanThreads];
    const int t = threadIdx.x;
    const long long n = *nslots < cap ? *nslots : cap;
    const long long seg = (n + kScanThreads - 1) / kScanThreads;
    const long long s0 = t * seg, s1 = s0 + seg < n ? s0 + seg : n;
    long long a = 0;
    for (long long s = s0; s < s1; ++s) a += cnt[s];
    part[t] = a;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {      // Hillis-Steele inclusive scan over the per-thread sums
        const long long x = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    long long c = part[t] - a;
    for (long long s = s0; s < s1; ++s) {
        off[s] = c;
        c += cnt[s];
    }
    if (t == kScanThreads - 1) off[n] = part[t];
}

__global__ void __launch_bounds__(kBlock)
raster_fill_kernel(const int64_t *__restrict__ tris, long long T, long long V, const int *__restrict__ slot,
                   int *__restrict__ cnt, const long long *__restrict__ off, int *__restrict__ list) {
    const long long t = gid();
    long long v[3];
    if (t >= T || !tri_ids(tris, t, V, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int s = slot[v[k]];
        if (s < 0) continue;
        const int pos = atomicSub(cnt + s, 1) - 1;     // the count pass counted this corner: 0 <= pos < count
        if (pos >= 0) list[off[s] + pos] = (int)t;
    }
}

__device__ void sift_down(int *a, long long root, long long n) {
    const int x = a[root];
    while (2 * root + 1 < n) {
        long long ch = 2 * root + 1;
        if (ch + 1 < n && a[ch + 1] > a[ch]) ++ch;
        if (a[ch] <= x) break;
        a[root] = a[ch];
        root = ch;
    }
    a[root] = x;
}

// in-place heapsort, ascending: O(n log n) however long a vertex's list is
__device__ void sort_ids(int *a, long long n) {
    for (long long i = n / 2 - 1; i >= 0; --i) sift_down(a, i, n);
    for (long long e = n - 1; e > 0; --e) {
        const int x = a[0];
        a[0] = a[e];
        a[e] = x;
        sift_down(a, 0, e);
    }
}

__global__ void __launch_bounds__(kBlock)
raster_vnormal_kernel(const float *__restrict__ verts, const int64_t *__restrict__ tris, const int *__restrict__ nslots,
                      long long cap, const long long *__restrict__ off, int *__restrict__ list, double *__restrict__ nrm) {
#pragma clang fp contract(off)
    const long long s = gid();
    if (s >= *nslots || s >= cap) return;
    int *L = list + off[s];
    const long long n = off[s + 1] - off[s];
    sort_ids(L, n);
    double nx = 0.0, ny = 0.0, nz = 0.0;
    for (long long j = 0; j < n; ++j) {
        const long long f = L[j];
        const float *a = verts + 3 * tris[3 * f], *b = verts + 3 * tris[3 * f + 1], *c = verts + 3 * tris[3 * f + 2];
        const double e1x = (double)b[0] - a[0], e1y = (double)b[1] - a[1], e1z = (double)b[2] - a[2];
        const double e2x = (double)c[0] - a[0], e2y = (double)c[1] - a[1], e2z = (double)c[2] - a[2];
        nx += e1y * e2z - e1z * e2y;
        ny += e1z * e2x - e1x * e2z;
        nz += e1x * e2y - e1y * e2x;
    }
    const double d = fmax(sqrt(nx * nx + ny * ny + nz * nz), 1e-6);
    nrm[3 * s] = nx / d;
    nrm[3 * s + 1] = ny / d;
    nrm[3 * s + 2] = nz / d;
}

__global__ void __launch_bounds__(kBlock)
raster_shade_kernel(const unsigned long long *__restrict__ keys, int R, const int64_t *__restrict__ tris, long long V,
                    const float *__restrict__ verts, const double2 *__restrict__ pxy, const float *__restrict__ pz,
                    const int *__restrict__ slot, const double *__restrict__ nrm, uint8_t *__restrict__ image,
                    int64_t *__restrict__ pix_to_face, float *__restrict__ zbuf, float *__restrict__ bary,
                    float *__restrict__ normals) {
#pragma clang fp contract(off)
    const long long p = gid();
    if (p >= (long long)R * R) return;
    const int r = (int)(p / R), c = (int)(p % R);
    const unsigned long long key = keys[p];
    Tri tr;
    double bp[3], zb;
    const long long t = (long long)(key & 0xFFFFFFFFull);
    if (key == kEmpty || !load_tri(tris, t, V, pxy, pz, tr) || !cover(tr, c + 0.5, r + 0.5, bp, zb)) {
        image[3 * p] = image[3 * p + 1] = image[3 * p + 2] = 255;
        if (pix_to_face) pix_to_face[p] = -1;
        if (zbuf) zbuf[p] = -1.0f;
        if (bary) bary[3 * p] = bary[3 * p + 1] = bary[3 * p + 2] = -1.0f;
        if (normals) normals[3 * p] = normals[3 * p + 1] = normals[3 * p + 2] = 0.0f;
        return;
    }
    double n[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long v = tris[3 * t + k];
        const int sv = slot[v];                              // every vertex of a winning triangle has a slot
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            n[a] += bp[k] * (sv >= 0 ? nrm[3 * (long long)sv + a] : 0.0);
            q[a] += bp[k] * (double)verts[3 * v + a];
        }
    }
    const double dn = fmax(sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-6);
    const double dq = fmax(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), 1e-6);
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] /= dn;
    const double cs = -(n[0] * q[0] + n[1] * q[1] + n[2] * q[2]) / dq;      // N . L, L = -p / |p|
    double spec = 0.0;
    if (cs > 0.0) {
        spec = fmax(2.0 * cs * cs - 1.0, 0.0);
#pragma unroll
        for (int i = 0; i < 6; ++i) spec *= spec;                          // ^64
    }
    const double colour = 0.5 + 0.3 * fmax(cs, 0.0) + 0.2 * spec;
    const double lv = fmin(fmax(floor(255.0 * colour), 0.0), 255.0);
    const uint8_t u = (uint8_t)(int)lv;
    image[3 * p] = image[3 * p + 1] = image[3 * p + 2] = u;
    if (pix_to_face) pix_to_face[p] = t;
    if (zbuf) zbuf[p] = (float)zb;
    if (bary) {
        bary[3 * p] = (float)bp[0];
        bary[3 * p + 1] = (float)bp[1];
        bary[3 * p + 2] = (float)bp[2];
    }
    if (normals) {
        normals[3 * p] = (float)n[0];
        normals[3 * p + 1] = (float)n[1];
        normals[3 * p + 2] = (float)n[2];
    }
}

int check_sizes(const char *who, long long V, long long T, int R) {
    if (V < 0 || V >= kMaxCount || T < 0 || T >= kMaxCount)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: V = %lld, T = %lld: both must lie in [0, 2^31)", who, V, T);
    if (R < 1 || R > kMaxR)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: render size %d outside [1, %d]", who, R, kMaxR);
    return 0;
}

inline unsigned blocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int enarf_raster_abi_version(void) { return ENARF_RASTER_ABI_VERSION; }

const char *enarf_raster_last_error(void) { return enarf::host::last_error(); }

size_t enarf_raster_workspace_bytes(int64_t V, int64_t T, int R) {
    if (V < 0 || V >= kMaxCount || T < 0 || T >= kMaxCount || R < 1 || R > kMaxR) return 0;
    return layout(V, T, R).bytes;
}

int enarf_raster_mesh(const float *vertices, int64_t V, const int64_t *triangles, int64_t T, const float *K_device,
                      int img_size, int R, void *workspace, uint8_t *image, int64_t *pix_to_face, float *zbuf,
                      float *bary, float *normals, void *stream) {
    const char *who = "enarf_raster_mesh";
    if (int rc = check_sizes(who, V, T, R)) return rc;
    if (img_size < 1) return enarf::host::fail(ENARF_ERR_ARG, "%s: img_size %d must be >= 1", who, img_size);
    if (!K_device || !workspace || !image || (V > 0 && !vertices) || (T > 0 && !triangles))
        return enarf::host::fail(ENARF_ERR_ARG, "%s: null K, workspace, image, vertices or triangles", who);
    const Layout l = layout(V, T, R);
    const long long npx = (long long)R * R;
    char *ws = static_cast<char *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto *pxy = reinterpret_cast<double2 *>(ws + l.pxy);
    auto *pz = reinterpret_cast<float *>(ws + l.pz);
    auto *keys = reinterpret_cast<unsigned long long *>(ws + l.keys);
    auto *slot = reinterpret_cast<int *>(ws + l.slot);
    auto *ctr = reinterpret_cast<int *>(ws + l.ctr);       // ctr[0]: big triangles listed, ctr[1]: slots named
    auto *big = reinterpret_cast<int *>(ws + l.big);
    auto *svert = reinterpret_cast<int *>(ws + l.svert);
    auto *cnt = reinterpret_cast<int *>(ws + l.cnt);
    auto *off = reinterpret_cast<long long *>(ws + l.off);
    auto *nrm = reinterpret_cast<double *>(ws + l.nrm);
    auto *list = reinterpret_cast<int *>(ws + l.list);
    hipError_t e = hipMemsetAsync(keys, 0xFF, 8 * (size_t)npx, st);
    if (e == hipSuccess) e = hipMemsetAsync(ctr, 0, 256, st);
    if (e == hipSuccess && V > 0) e = hipMemsetAsync(slot, 0xFF, 4 * (size_t)V, st);
    if (e == hipSuccess && l.cap > 0) e = hipMemsetAsync(cnt, 0, 4 * (size_t)l.cap, st);
    if (e != hipSuccess) return enarf::host::fail((int)e, "%s: workspace fill failed: %s", who, hipGetErrorString(e));
    if (V > 0 && T > 0) {
        hipLaunchKernelGGL(raster_project_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, vertices, (long long)V, K_device,
                           (double)img_size / R, pxy, pz);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_project_kernel")) return rc;
        hipLaunchKernelGGL(raster_depth_kernel, dim3(blocks(T)), dim3(kBlock), 0, st, triangles, (long long)T,
                           (long long)V, pxy, pz, R, keys, ctr, big);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_depth_kernel")) return rc;
        hipLaunchKernelGGL(raster_big_kernel, dim3(kBigBlocks), dim3(kBlock), 0, st, triangles, (long long)V, pxy, pz, R,
                           keys, ctr, big);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_big_kernel")) return rc;
        hipLaunchKernelGGL(raster_mark_kernel, dim3(blocks(npx)), dim3(kBlock), 0, st, keys, npx, triangles, slot,
                           ctr + 1, svert, l.cap);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_mark_kernel")) return rc;
        hipLaunchKernelGGL(raster_count_kernel, dim3(blocks(T)), dim3(kBlock), 0, st, triangles, (long long)T,
                           (long long)V, slot, cnt);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_count_kernel")) return rc;
        hipLaunchKernelGGL(raster_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, cnt, ctr + 1, l.cap, off);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_scan_kernel")) return rc;
        hipLaunchKernelGGL(raster_fill_kernel, dim3(blocks(T)), dim3(kBlock), 0, st, triangles, (long long)T,
                           (long long)V, slot, cnt, off, list);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_fill_kernel")) return rc;
        hipLaunchKernelGGL(raster_vnormal_kernel, dim3(blocks(l.cap)), dim3(kBlock), 0, st, vertices, triangles, ctr + 1,
                           l.cap, off, list, nrm);
        if (int rc = enarf::host::check_launch("enarf_raster_mesh: raster_vnormal_kernel")) return rc;
    }
    hipLaunchKernelGGL(raster_shade_kernel, dim3(blocks(npx)), dim3(kBlock), 0, st, keys, R, triangles, (long long)V,
                       vertices, pxy, pz, slot, nrm, image, pix_to_face, zbuf, bary, normals);
    return enarf::host::check_launch("enarf_raster_mesh: raster_shade_kernel");
}

}  // extern "C"
