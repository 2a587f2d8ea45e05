// enarf_mesh.hip - marching cubes over a device-resident fp32 volume (libenarf_mesh.so, include/enarf_mesh.h).
//
// Three launches, workspace O(X*Y):
//   mc_count_kernel  one wave per lattice row (i, j, .), 64 points a step (each lane loads its points k and k + 1): the row's owned crossing edges (0-3 per point)
//                    and the triangles of its cubes (i, j, k) from the case table; per-row int32 totals, and per-tile
//                    (16 rows, one block) int64 sums;
//   mc_scan_kernel   one block: exclusive scan of the tile sums into int64 tile offsets, and the grand totals (V, T);
//   mc_emit_kernel   the same walk; a wave scans four rows' crossing-edge counts (rows (i,j), (i+1,j), (i,j+1),
//                    (i+1,j+1), packed with the cube's triangle count into one 64-bit word) so it knows the vertex id of
//                    every edge its cubes use, writes the row's vertices and the cubes' triangles at the scanned offsets.
// A row's base offset is its tile's offset plus the int32 totals of the rows before it in the tile (at most 15).
// Blocks are dealt round-robin over the 8 XCDs; the block -> tile map gives each XCD a contiguous range of tiles, so the
// neighbouring rows a wave reads (i+1 and i+2 are Y rows further on) were mostly fetched into that XCD's L2 just before.
#include "enarf_mesh.h"
#include "enarf_host.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ENARF_MC_TABLE_SPACE __constant__
#include "enarf_mc_table.h"

namespace {

using enarf::host::align256;

constexpr int kWave = 64;
constexpr int kWaves = 4;                         // waves per block
constexpr int kRowsPerWave = 4;
constexpr int kTileRows = kWaves * kRowsPerWave;  // rows per block = one scan tile
constexpr int kScanThreads = 1024;

struct Layout {
    long long rows, tiles;
    size_t vcnt, tcnt, tsum_v, tsum_t, tot, bytes;
};

inline Layout layout(int X, int Y) {
    Layout l;
    l.rows = (long long)X * Y;
    l.tiles = (l.rows + kTileRows - 1) / kTileRows;
    l.vcnt = 0;
    l.tcnt = align256(l.vcnt + sizeof(int) * l.rows);
    l.tsum_v = align256(l.tcnt + sizeof(int) * l.rows);
    l.tsum_t = align256(l.tsum_v + sizeof(long long) * l.tiles);
    l.tot = align256(l.tsum_t + sizeof(long long) * l.tiles);
    l.bytes = l.tot + 256;
    return l;
}

// bijective XCD-grouping of the block index: the blocks the dispatcher deals to one XCD (b, b + 8, ...) get consecutive
// tiles. Placement only changes speed, never the result.
__device__ __forceinline__ long long tile_of_block(long long b, long long nb) {
    const long long q = nb / 8, r = nb % 8, x = b % 8, idx = b / 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + idx;
}

__device__ __forceinline__ int inside(float v, float iso) { return v > iso ? 1 : 0; }   // NaN: outside

__device__ __forceinline__ float ld(const float *__restrict__ vol, bool ok, size_t idx) {
    return ok ? vol[idx] : 0.0f;
}

__device__ __forceinline__ int bit(const float *__restrict__ vol, bool ok, size_t idx, float iso) {
    return ok ? inside(vol[idx], iso) : 0;
}

__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}

__global__ void __launch_bounds__(kWaves * kWave)
mc_count_kernel(const float *__restrict__ vol, int X, int Y, int Z, float iso, int *__restrict__ vcnt,
                int *__restrict__ tcnt, long long *__restrict__ tsum_v, long long *__restrict__ tsum_t, long long tiles) {
    __shared__ long long part[2][kWaves];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const long long tile = tile_of_block(blockIdx.x, gridDim.x);
    const long long rows = (long long)X * Y;
    long long tv = 0, tt = 0;
    for (int q = 0; q < kRowsPerWave; ++q) {
        const long long row = tile * kTileRows + w * kRowsPerWave + q;
        if (row >= rows) break;
        const int i = (int)(row / Y), j = (int)(row % Y);
        const bool hx = i + 1 < X, hy = j + 1 < Y;
        const size_t r00 = (size_t)row * Z, r10 = r00 + (size_t)Y * Z, r01 = r00 + Z, r11 = r10 + Z;
        int nv = 0, nt = 0;
        for (int k0 = 0; k0 < Z; k0 += kWave) {
            const int k = k0 + lane;
            const bool in = k < Z;
            const int m = bit(vol, in, r00 + k, iso) | bit(vol, in && hx, r10 + k, iso) << 1 |
                          bit(vol, in && hy, r01 + k, iso) << 2 | bit(vol, in && hx && hy, r11 + k, iso) << 3;
            // point k + 1: loaded by every lane next to point k (the same lines), so a step waits for one round trip
            const bool hz = k + 1 < Z;
            const int kk = k + 1;
            const int mn = bit(vol, hz, r00 + kk, iso) | bit(vol, hz && hx, r10 + kk, iso) << 1 |
                           bit(vol, hz && hy, r01 + kk, iso) << 2 | bit(vol, hz && hx && hy, r11 + kk, iso) << 3;
            if (in) {
                const int b = m & 1;
                nv += (hx & (b ^ ((m >> 1) & 1))) + (hy & (b ^ ((m >> 2) & 1))) + (hz & (b ^ (mn & 1)));
                if (hx && hy && hz) nt += ENARF_MC_NTRI[m | (mn << 4)];
            }
        }
        const long long sv = wave_sum(nv), st = wave_sum(nt);
        if (lane == 0) {
            vcnt[row] = (int)sv;
            tcnt[row] = (int)st;
        }
        tv += sv;
        tt += st;
    }
    if (lane == 0) {
        part[0][w] = tv;
        part[1][w] = tt;
    }
    __syncthreads();
    if (threadIdx.x == 0 && tile < tiles) {
        long long a = 0, b = 0;
        for (int q = 0; q < kWaves; ++q) {
            a += part[0][q];
            b += part[1][q];
        }
        tsum_v[tile] = a;
        tsum_t[tile] = b;
    }
}

// one block: tile sums -> exclusive tile offsets (in place), and the grand totals
__global__ void __launch_bounds__(kScanThreads)
mc_scan_kernel(long long *__restrict__ tsum_v, long long *__restrict__ tsum_t, long long tiles, int64_t *__restrict__ totals,
               long long *__restrict__ ws_totals) {
    __shared__ long long sv[kScanThreads], st[kScanThreads];
    const int t = threadIdx.x;
    const long long seg = (tiles + kScanThreads - 1) / kScanThreads;
    const long long s0 = t * seg, s1 = s0 + seg < tiles ? s0 + seg : tiles;
    long long a = 0, b = 0;
    for (long long s = s0; s < s1; ++s) {
        a += tsum_v[s];
        b += tsum_t[s];
    }
    sv[t] = a;
    st[t] = b;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {      // Hillis-Steele inclusive scan over the per-thread sums
        const long long xa = t >= o ? sv[t - o] : 0, xb = t >= o ? st[t - o] : 0;
        __syncthreads();
        sv[t] += xa;
        st[t] += xb;
        __syncthreads();
    }
    long long ca = sv[t] - a, cb = st[t] - b;
    for (long long s = s0; s < s1; ++s) {
        const long long va = tsum_v[s], vb = tsum_t[s];
        tsum_v[s] = ca;
        tsum_t[s] = cb;
        ca += va;
        cb += vb;
    }
    if (t == kScanThreads - 1) {
        totals[0] = ws_totals[0] = sv[t];
        totals[1] = ws_totals[1] = st[t];
    }
}

__device__ __forceinline__ long long sel4(int r, long long a, long long b, long long c, long long d) {
    return r == 0 ? a : r == 1 ? b : r == 2 ? c : d;
}

// vertex id of cube edge e: its base point lies in row rr = dx + 2 dy of the four, at k + dz, on axis a
struct EdgeIds {
    long long at0[4];   // id of the first owned edge of the row's point k
    int ex0[4], ey0[4]; // owned x / y crossings at k
    long long at1[4];   // id of the first owned edge of the row's point k + 1
    int ex1[4], ey1[4];
};

__device__ __forceinline__ long long edge_id(const EdgeIds &E, int e) {
    const int a = e >> 2, b0 = e & 1, b1 = (e >> 1) & 1;
    const int dx = a == 0 ? 0 : b0, dy = a == 0 ? b0 : (a == 1 ? 0 : b1), dz = a == 2 ? 0 : b1;
    const int rr = dx + 2 * dy;
    if (dz) {
        const long long base = sel4(rr, E.at1[0], E.at1[1], E.at1[2], E.at1[3]);
        const int ex = (int)sel4(rr, E.ex1[0], E.ex1[1], E.ex1[2], E.ex1[3]);
        const int ey = (int)sel4(rr, E.ey1[0], E.ey1[1], E.ey1[2], E.ey1[3]);
        return base + (a == 0 ? 0 : a == 1 ? ex : ex + ey);
    }
    const long long base = sel4(rr, E.at0[0], E.at0[1], E.at0[2], E.at0[3]);
    const int ex = (int)sel4(rr, E.ex0[0], E.ex0[1], E.ex0[2], E.ex0[3]);
    const int ey = (int)sel4(rr, E.ey0[0], E.ey0[1], E.ey0[2], E.ey0[3]);
    return base + (a == 0 ? 0 : a == 1 ? ex : ex + ey);
}

// base offset of a row: its tile's offset plus the rows before it in the tile
__device__ __forceinline__ long long row_base(const int *__restrict__ cnt, const long long *__restrict__ toff, long long row) {
    const long long t0 = (row / kTileRows) * kTileRows;
    long long s = toff[row / kTileRows];
    for (long long r = t0; r < row; ++r) s += cnt[r];
    return s;
}

__global__ void __launch_bounds__(kWaves * kWave)
mc_emit_kernel(const float *__restrict__ vol, int X, int Y, int Z, float iso, const int *__restrict__ vcnt,
               const int *__restrict__ tcnt, const long long *__restrict__ toff_v, const long long *__restrict__ toff_t,
               const long long *__restrict__ ws_totals, float *__restrict__ verts, int64_t *__restrict__ tris) {
    // the outputs were sized from these totals: no write goes past them, whatever the volume holds
    const long long nv = ws_totals[0], nt = ws_totals[1];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const long long tile = tile_of_block(blockIdx.x, gridDim.x);
    const long long rows = (long long)X * Y;
    const size_t YZ = (size_t)Y * Z;
    for (int q = 0; q < kRowsPerWave; ++q) {
        const long long row = tile * kTileRows + w * kRowsPerWave + q;
        if (row >= rows) break;
        const int i = (int)(row / Y), j = (int)(row % Y);
        // rows R0..R7: (i,j) (i+1,j) (i,j+1) (i+1,j+1) (i+2,j) (i,j+2) (i+2,j+1) (i+1,j+2)
        const bool x1 = i + 1 < X, x2 = i + 2 < X, y1 = j + 1 < Y, y2 = j + 2 < Y;
        const bool ok[8] = {true, x1, y1, x1 && y1, x2, y2, x2 && y1, x1 && y2};
        const size_t r0 = (size_t)row * Z;
        const size_t base[8] = {r0, r0 + YZ, r0 + Z, r0 + YZ + Z, r0 + 2 * YZ, r0 + 2 * (size_t)Z, r0 + 2 * YZ + Z,
                                r0 + YZ + 2 * (size_t)Z};
        // edge existence per row of the four: x-edge needs row a+1, y-edge row b+1 (and the row itself)
        const bool hx[4] = {x1, x2, x1 && y1, x2 && y1};
        const bool hy[4] = {y1, x1 && y1, y2, x1 && y2};
        // vertex bases of the four rows, triangle base of R0 (lanes 0-4 each fetch one, then broadcast)
        long long mine = 0;
        if (lane < 4 && ok[lane]) {
            const long long rr = row + (lane & 1) * Y + (lane >> 1);
            mine = row_base(vcnt, toff_v, rr);
        } else if (lane == 4) {
            mine = row_base(tcnt, toff_t, row);
        }
        long long bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = __shfl(mine, r, kWave);
        long long bt = __shfl(mine, 4, kWave);
        const bool cube_row = x1 && y1;
        for (int k0 = 0; k0 < Z; k0 += kWave) {
            const int k = k0 + lane;
            const bool in = k < Z, hz = k + 1 < Z;
            // points k and k + 1 of the eight rows, all loads issued together (k + 1 hits the lines of k)
            float f[8], g[8];
            int m = 0, mn = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                f[r] = ld(vol, in && ok[r], base[r] + k);
                g[r] = ld(vol, hz && ok[r], base[r] + k + 1);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                m |= (in && ok[r] ? inside(f[r], iso) : 0) << r;
                mn |= (hz && ok[r] ? inside(g[r], iso) : 0) << r;
            }
            const float fn = g[0];
            // per row of the four: owned crossings at k and at k + 1
            const int xn[4] = {1, 4, 3, 6}, yn[4] = {2, 3, 5, 7};
            int ex0[4], ey0[4], ez0[4], ex1[4], ey1[4], c[4];
            unsigned long long packed = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = (m >> r) & 1, bn = (mn >> r) & 1;
                ex0[r] = (in && hx[r]) ? b ^ ((m >> xn[r]) & 1) : 0;
                ey0[r] = (in && hy[r]) ? b ^ ((m >> yn[r]) & 1) : 0;
                ez0[r] = (in && hz && ok[r]) ? b ^ bn : 0;
                ex1[r] = (hz && hx[r]) ? bn ^ ((mn >> xn[r]) & 1) : 0;
                ey1[r] = (hz && hy[r]) ? bn ^ ((mn >> yn[r]) & 1) : 0;
                c[r] = ex0[r] + ey0[r] + ez0[r];
                packed |= (unsigned long long)c[r] << (12 * r);
            }
            const bool cube = cube_row && hz;
            const int cs = (m & 15) | ((mn & 15) << 4);
            const int ntri = cube ? ENARF_MC_NTRI[cs] : 0;
            packed |= (unsigned long long)ntri << 48;
            unsigned long long incl = packed;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const unsigned long long y = __shfl_up(incl, o, kWave);
                if (lane >= o) incl += y;
            }
            const unsigned long long excl = incl - packed, total = __shfl(incl, kWave - 1, kWave);
            EdgeIds E;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                E.at0[r] = bv[r] + (long long)((excl >> (12 * r)) & 0xFFF);
                E.at1[r] = E.at0[r] + c[r];
                E.ex0[r] = ex0[r];
                E.ey0[r] = ey0[r];
                E.ex1[r] = ex1[r];
                E.ey1[r] = ey1[r];
            }
            if (c[0] && E.at0[0] + c[0] <= nv) {           // the row's own vertices: x, y, z order at point k
                long long id = E.at0[0];
                const float fi = (float)i, fj = (float)j, fk = (float)k;
                if (ex0[0]) {
                    const float t = __fdiv_rn(__fsub_rn(iso, f[0]), __fsub_rn(f[1], f[0]));
                    float *o = verts + 3 * id++;
                    o[0] = __fadd_rn(fi, t), o[1] = fj, o[2] = fk;
                }
                if (ey0[0]) {
                    const float t = __fdiv_rn(__fsub_rn(iso, f[0]), __fsub_rn(f[2], f[0]));
                    float *o = verts + 3 * id++;
                    o[0] = fi, o[1] = __fadd_rn(fj, t), o[2] = fk;
                }
                if (ez0[0]) {
                    const float t = __fdiv_rn(__fsub_rn(iso, f[0]), __fsub_rn(fn, f[0]));
                    float *o = verts + 3 * id;
                    o[0] = fi, o[1] = fj, o[2] = __fadd_rn(fk, t);
                }
            }
            const long long t0 = bt + (long long)(excl >> 48);
            if (ntri && t0 + ntri <= nt) {
                const int4 tr = reinterpret_cast<const int4 *>(ENARF_MC_TRI)[cs];
                const int word[4] = {tr.x, tr.y, tr.z, tr.w};
                int64_t *o = tris + 3 * t0;
#pragma unroll
                for (int n = 0; n < ENARF_MC_MAX_TRI; ++n) {
                    if (n < ntri) {
#pragma unroll
                        for (int v = 0; v < 3; ++v) {
                            const int s = 3 * n + v;
                            const int e = (int)(signed char)((word[s >> 2] >> (8 * (s & 3))) & 0xFF);
                            const long long id = edge_id(E, e);
                            o[s] = id >= 0 && id < nv ? id : -1;
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[r] += (long long)((total >> (12 * r)) & 0xFFF);
            bt += (long long)(total >> 48);
        }
    }
}

int check_sizes(const char *who, int X, int Y, int Z) {
    if (X < 2 || Y < 2 || Z < 2)
        return enarf::host::fail(ENARF_ERR_ARG, "%s: volume (%d, %d, %d): every extent must be >= 2", who, X, Y, Z);
    if ((long long)X * Y * Z >= (1LL << 31))
        return enarf::host::fail(ENARF_ERR_UNSUPPORTED, "%s: volume (%d, %d, %d) has >= 2^31 points", who, X, Y, Z);
    return 0;
}

}  // namespace

extern "C" {

int enarf_mesh_abi_version(void) { return ENARF_MESH_ABI_VERSION; }

const char *enarf_mesh_last_error(void) { return enarf::host::last_error(); }

size_t enarf_mesh_workspace_bytes(int X, int Y, int Z) {
    if (X < 2 || Y < 2 || Z < 2 || (long long)X * Y * Z >= (1LL << 31)) return 0;
    return layout(X, Y).bytes;
}

int enarf_mesh_count(const float *volume, int X, int Y, int Z, float iso, void *workspace, int64_t *totals, void *stream) {
    if (int rc = check_sizes("enarf_mesh_count", X, Y, Z)) return rc;
    if (!volume || !workspace || !totals)
        return enarf::host::fail(ENARF_ERR_ARG, "enarf_mesh_count: null volume, workspace or totals");
    const Layout l = layout(X, Y);
    char *ws = static_cast<char *>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)l.tiles), dim3(kWaves * kWave), 0, s, volume, X, Y, Z, iso,
                       reinterpret_cast<int *>(ws + l.vcnt), reinterpret_cast<int *>(ws + l.tcnt),
                       reinterpret_cast<long long *>(ws + l.tsum_v), reinterpret_cast<long long *>(ws + l.tsum_t), l.tiles);
    if (int rc = enarf::host::check_launch("enarf_mesh_count: mc_count_kernel")) return rc;
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, reinterpret_cast<long long *>(ws + l.tsum_v),
                       reinterpret_cast<long long *>(ws + l.tsum_t), l.tiles, totals, reinterpret_cast<long long *>(ws + l.tot));
    return enarf::host::check_launch("enarf_mesh_count: mc_scan_kernel");
}

int enarf_mesh_emit(const float *volume, int X, int Y, int Z, float iso, const void *workspace, float *vertices,
                    int64_t *triangles, void *stream) {
    if (int rc = check_sizes("enarf_mesh_emit", X, Y, Z)) return rc;
    if (!volume || !workspace || !vertices || !triangles)
        return enarf::host::fail(ENARF_ERR_ARG, "enarf_mesh_emit: null volume, workspace or output");
    const Layout l = layout(X, Y);
    const char *ws = static_cast<const char *>(workspace);
    hipLaunchKernelGGL(mc_emit_kernel, dim3((unsigned)l.tiles), dim3(kWaves * kWave), 0, static_cast<hipStream_t>(stream),
                       volume, X, Y, Z, iso, reinterpret_cast<const int *>(ws + l.vcnt),
                       reinterpret_cast<const int *>(ws + l.tcnt), reinterpret_cast<const long long *>(ws + l.tsum_v),
                       reinterpret_cast<const long long *>(ws + l.tsum_t), reinterpret_cast<const long long *>(ws + l.tot),
                       vertices, triangles);
    return enarf::host::check_launch("enarf_mesh_emit: mc_emit_kernel");
}

}  // extern "C"
