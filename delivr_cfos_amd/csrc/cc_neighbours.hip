// cc_neighbours.hip - the neighbour table of a label volume on the device (dlv_cc_neighbours_count_dev, dlv_cc_neighbours_dev): every
// pair of labels a < b whose cells come within a radius of each other, with the exact smallest squared distance between a voxel of
// one and a voxel of the other - what count_blobs' neighbour_stats turns into degrees, nearest cells and clusters.  The reference
// has no counterpart.  A voxel takes part when 1 <= L(v) <= n; the background and labels above n contribute nothing and block
// nothing.  With the integer spacings wz, wy, wx (1..64)
//     gap2(a, b) = min over L(v) = a, L(u) = b of (wz (vz - uz))^2 + (wy (vy - uy))^2 + (wx (vx - ux))^2,
// and the table holds every a < b with gap2(a, b) <= R2.  gap2 >= 1, the key of a pair is (a << 32) | b, never 0.  The per-axis
// reach is rho_a = floor(sqrt(R2) / w_a) <= NB_MAX_REACH; tests/helpers/neighbour_reference.py is the numpy statement of the result.
//
// Two exact prunings of the voxel pairs that are looked at:
//  1. POSITIVE HALF-SPACE.  An unordered voxel pair {v, u} is visited once, from its raster-earlier voxel v, over the offsets
//     u - v with dz > 0, or dz == 0 and dy > 0, or dz == dy == 0 and dx > 0, and recorded under (min(a, b), max(a, b)): the metric
//     is symmetric, so nothing is lost.
//  2. SURFACE SOURCES, PER DIRECTION.  Let (v, u) be a pair that attains gap2(a, b), v the earlier voxel, and step one voxel from v
//     towards u along the first axis of z, y, x on which the two differ - by the half-space that step is +z when dz > 0, +y when
//     dz == 0 and dy > 0, +x otherwise.  The voxel v' reached lies between v and u on that axis, so it is inside the volume, and it
//     is strictly closer to u (the spacings are >= 1).  Were L(v') = L(v), (v', u) would be a closer pair of the same two cells:
//     so L(v') != L(v).  A source voxel therefore scans the rows with dz > 0 only when its +z neighbour holds another label, the
//     rows dz == 0, dy > 0 only when its +y neighbour does, and the row dz == dy == 0 only when its +x neighbour does; a voxel with
//     none of the three scans nothing.  (This is the issue's "voxels with a face neighbour of a different label", narrowed to the
//     one face the argument uses.  A label above n counts as background on both sides of the comparison, which changes nothing for
//     a source that takes part.)
//
// One kernel, built twice (count / table), so that both passes make the same traversal.  A workgroup of 256 threads owns a tile of
// 8 x 8 x 32 voxels.  It first looks at its own voxels and returns at once when none takes part (as cc_shell).  Else it stages the
// tile with its halo in LDS - rho_z planes on the far side only, rho_y / rho_x on both sides; labels above n and voxels outside the
// volume as 0 -, (8 + 8) x (8 + 16) x (32 + 16) words = 72 KiB whatever the reach (below 80 KiB with the lists: two workgroups per CU).  The surface voxels of the tile are listed in
// LDS in raster order (a block-wide scan, no atomic: the list, and with it S, does not depend on scheduling), and the threads take
// (row offset (dz, dy), surface voxel) items, row-major, so that the lanes of a wave mostly walk rows of one length.  The rows
// with (wz dz)^2 + (wy dy)^2 <= R2 and the x reach of each, cut to the ellipsoid, are tabulated on the host (at most 145 rows).
// A thread keeps a carry (a, b, min d2) over consecutive hits of one pair - across its items too - and flushes it when the pair
// changes and at its end; a flush is a "segment": the count adds them up (S >= P), the table pass puts them into an open-addressed
// table in HBM - cc_pair_table.h: cc_overlap.hip's hash (splitmix64's finaliser), linear probe and compaction, with a minimum in place of the sum:
// a slot is {uint64 key, uint64 2^32 - 1 - d2} under an atomic maximum, so that the zero-cleared table needs no second
// initialisation.  Every loop is bounded: a probe visits at most cap slots, a write goes below out_cap, and either overflow sets
// a word that the host turns into DLV_ESTATE.  No wave waits for another or spins on memory.  Integer work only, minimum and
// maximum commute: the table is exact and independent of scheduling.
// Deviations from the issue's sketch: pruning 2 per direction (above); the staging does not go through cc_tile.h, whose tile has
// a one-voxel halo on every side; no LDS-level pair cache.  Not measured yet: profiles/README.md, "cc_neighbours".
#include "common.h"
#include "cc_check.h"
#include "cc_pair_table.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int NB_MAX_REACH = 8;  // the largest per-axis reach in voxels: the halo of the LDS tile
constexpr int R = NB_MAX_REACH;
constexpr int NT = 256;                  // threads per workgroup
constexpr int NTX = 32, NTY = 8, NTZ = 8;  // the voxels of a workgroup's tile: 8 per thread, 4 threads per row
constexpr int LX = NTX + 2 * R, LY = NTY + 2 * R, LZ = NTZ + R;  // the LDS image: own voxel (oz, oy, ox) at (oz, oy + R, ox + R)
constexpr int TILE_VOX = NTX * NTY * NTZ;
constexpr int NR_MAX = R * (2 * R + 1) + R + 1;  // row offsets (dz, dy) of the positive half-space: 145
constexpr int MAX_X = 1 << 30;                   // (x0 + the halo stays an int)

// the rows a source voxel scans: row[i] = dz | (dy + R) << 4 | xr << 9, xr the largest |dx| with the offset inside the ellipsoid
struct NbRows {
    int n;
    u32 row[NR_MAX];
};

// d2 of `key` into its slot, the smallest wins (cc_pair_table.h: at most cap probes, the overflow word where no slot is left)
__device__ __forceinline__ void table_min(u64* __restrict__ table, u64 cap, u64 key, u32 d2, u64* __restrict__ words) {
    if (u64* at = pair_slot(table, cap, key, words)) atomicMax(at, (u64)(0xffffffffu - d2));
}

__device__ __forceinline__ int lds_at(int oz, int oy, int ox) { return (oz * LY + oy + R) * LX + ox + R; }

// TABLE = false: words[W_COUNT] += the segments of the volume; TABLE = true: the segments go into the table
template <bool TABLE>
__global__ void __launch_bounds__(NT) cc_neighbours_kernel(const u32* __restrict__ labels, int Z, int Y, int X, u32 n, u32 wz2, u32 wy2,
                                                           u32 wx2, int rz, int ry, int rx, NbRows rows, u64* __restrict__ table, u64 cap,
                                                           u64* __restrict__ words) {
    __shared__ u32 lab[LZ * LY * LX];
    __shared__ unsigned short list[TILE_VOX];  // a surface voxel: its index in the tile | the faces that differ (bit 11: +z, 12: +y, 13: +x)
    __shared__ u32 rowtab[NR_MAX];
    __shared__ u32 wsum[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z0 = blockIdx.z * NTZ, y0 = blockIdx.y * NTY, x0 = blockIdx.x * NTX;
    // this thread's eight voxels of the tile: row (oz, oy), x from ox0
    const int oz = tid >> 5, oy = (tid >> 2) & 7, ox0 = (tid & 3) * 8;

    // ---- a tile without a voxel that takes part has nothing to scan from -----------------------------------------------------
    {
        bool any = false;
        const int z = z0 + oz, y = y0 + oy;
        if (z < Z && y < Y) {
            const u32* p = labels + ((u64)z * Y + y) * (u64)X;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int x = x0 + ox0 + k;
                if (x < X) any |= p[x] - 1u < n;  // (false for 0 and for a label above n, n <= 2^32 - 2)
            }
        }
        if (!__syncthreads_or(any)) return;
    }

    // ---- the tile and its halo --------------------------------------------------------------------------------------------------
    {
        const int SX = NTX + 2 * rx, SY = NTY + 2 * ry, SZ = NTZ + rz;
        for (int i = tid; i < SZ * SY * SX; i += NT) {
            const int lx = i % SX, t = i / SX, ly = t % SY, lz = t / SY;
            const int z = z0 + lz, y = y0 + ly - ry, x = x0 + lx - rx;
            u32 v = 0;
            if (z < Z && y >= 0 && y < Y && x >= 0 && x < X) {
                const u32 l = labels[((u64)z * Y + y) * (u64)X + x];
                v = l - 1u < n ? l : 0u;
            }
            lab[lds_at(lz, ly - ry, lx - rx)] = v;
        }
        if (tid < rows.n) rowtab[tid] = rows.row[tid];
    }
    __syncthreads();

    // ---- the surface voxels, in raster order ------------------------------------------------------------------------------------
    u32 face[8];
    u32 cnt = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int p = lds_at(oz, oy, ox0 + k);
        const u32 a = lab[p];
        u32 f = 0;
        if (a != 0) {
            if (rz > 0 && lab[p + LY * LX] != a) f |= 1u;
            if (ry > 0 && lab[p + LX] != a) f |= 2u;
            if (rx > 0 && lab[p + 1] != a) f |= 4u;
        }
        face[k] = f;
        cnt += f != 0 ? 1u : 0u;
    }
    u32 incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    u32 at = incl - cnt, nsurf = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        at += w < wave ? wsum[w] : 0u;
        nsurf += wsum[w];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (face[k] != 0) list[at++] = (unsigned short)((u32)(tid * 8 + k) | (face[k] << 11));  // (tid * 8 + k = (oz * 8 + oy) * 32 + ox)
    __syncthreads();

    // ---- the items (row, surface voxel), row-major --------------------------------------------------------------------------------
    u32 ca = 0, cb = 0, cd = 0;  // the carry: the pair ca < cb (ca == 0: none) and its smallest d2 so far
    u32 segments = 0;  // (a thread flushes at most once per voxel it reads: below 2^32 for the workgroup)
    auto flush = [&]() {
        if (ca == 0) return;
        if (TABLE) table_min(table, cap, ((u64)ca << 32) | cb, cd, words);
        else ++segments;
    };
    const u32 total = nsurf * (u32)rows.n;  // (at most 2048 * 145)
    for (u32 item = tid; item < total; item += NT) {
        const u32 r = item / nsurf, s = item - r * nsurf;
        const u32 e = list[s], row = rowtab[r];
        const int dz = (int)(row & 15u), dy = (int)((row >> 4) & 31u) - R, xr = (int)((row >> 9) & 15u);
        const u32 needs = dz > 0 ? 1u : dy > 0 ? 2u : 4u;
        if (!((e >> 11) & needs)) continue;
        const int p = lds_at((int)((e >> 8) & 7u), (int)((e >> 5) & 7u), (int)(e & 31u));
        const u32 a = lab[p];
        const u32 base = wz2 * (u32)(dz * dz) + wy2 * (u32)(dy * dy);
        const int q = p + (dz * LY + dy) * LX;
        for (int dx = (dz == 0 && dy == 0) ? 1 : -xr; dx <= xr; ++dx) {
            const u32 b = lab[q + dx];
            if (b != 0 && b != a) {
                const u32 d = base + wx2 * (u32)(dx * dx);
                const u32 lo = min(a, b), hi = max(a, b);
                if (lo == ca && hi == cb) {
                    cd = min(cd, d);
                } else {
                    flush();
                    ca = lo; cb = hi; cd = d;
                }
            }
        }
    }
    flush();
    if (!TABLE) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) segments += __shfl_xor(segments, o);
        if (lane == 0 && segments) atomicAdd(words + W_COUNT, (u64)segments);
    }
}

// the largest k with (k w)^2 <= r2, that is floor(sqrt(r2) / w), in integers
u64 reach_of(u64 r2, int w) {
    u64 s = (u64)std::sqrt((long double)r2);
    while (s * s > r2) --s;
    while ((s + 1) * (s + 1) <= r2) ++s;
    return s / (u64)w;
}

// what both entries check before anything is launched; the rows of the scan
int neighbours_args(dlv_ctx* ctx, const char* what, const void* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                    uint64_t r2, int (&rho)[3], NbRows& rows) {
    DLV_TRY(check_volume(ctx, what, Z, Y, X));
    DLV_TRY(check_label_count(ctx, what, n));
    if ((uintptr_t)labels_dev & 3) return dlv_fail(ctx, DLV_EINVAL, "%s: the label volume must be 4-byte aligned", what);
    DLV_TRY(check_spacing(ctx, what, "z", wz));
    DLV_TRY(check_spacing(ctx, what, "y", wy));
    DLV_TRY(check_spacing(ctx, what, "x", wx));
    if (r2 < 1) return dlv_fail(ctx, DLV_EINVAL, "%s: r2 = 0: the squared radius must be at least 1", what);
    const int w[3] = {wz, wy, wx};
    const char* axis[3] = {"z", "y", "x"};
    for (int a = 0; a < 3; ++a) {
        const u64 reach = reach_of(r2, w[a]);
        if (reach > (u64)NB_MAX_REACH)
            return dlv_fail(ctx, DLV_EUNSUP, "%s: axis %s: r2 = %llu over a spacing of %d reaches %llu voxels, this version supports a "
                            "reach of at most %d", what, axis[a], (unsigned long long)r2, w[a], (unsigned long long)reach, NB_MAX_REACH);
        rho[a] = (int)reach;
    }
    if (X > MAX_X) return dlv_fail(ctx, DLV_EUNSUP, "%s: X = %d exceeds %d", what, X, MAX_X);
    DLV_TRY(check_tile_grid(ctx, what, dim3((X + NTX - 1) / NTX, (Y + NTY - 1) / NTY, (Z + NTZ - 1) / NTZ), Z, Y, X));
    rows.n = 0;
    for (int dz = 0; dz <= rho[0]; ++dz)
        for (int dy = dz > 0 ? -rho[1] : 0; dy <= rho[1]; ++dy) {
            const u64 base = (u64)(wz * dz) * (wz * dz) + (u64)(wy * dy) * (wy * dy);
            if (base > r2) continue;
            const int xr = (int)std::min<u64>(reach_of(r2 - base, wx), (u64)rho[2]);  // (r2 - base = 0: 0)
            if (dz == 0 && dy == 0 && xr == 0) continue;                           // (the voxel itself)
            rows.row[rows.n++] = (u32)dz | (u32)(dy + R) << 4 | (u32)xr << 9;
        }
    return DLV_OK;
}

template <bool TABLE>
void launch_scan(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx, const int (&rho)[3],
                 const NbRows& rows, u64* table, u64 cap, u64* words) {
    const dim3 grid((X + NTX - 1) / NTX, (Y + NTY - 1) / NTY, (Z + NTZ - 1) / NTZ);
    hipLaunchKernelGGL(cc_neighbours_kernel<TABLE>, grid, dim3(NT), 0, ctx->stream, labels_dev, Z, Y, X, (u32)n, (u32)(wz * wz), (u32)(wy * wy),
                       (u32)(wx * wx), rho[0], rho[1], rho[2], rows, table, cap, words);
}

}  // namespace

extern "C" {

int dlv_cc_neighbours_count_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                                uint64_t r2, uint64_t* n_segments) {
    if (!ctx || !labels_dev || !n_segments) return DLV_EINVAL;
    int rho[3];
    NbRows rows;
    DLV_TRY(neighbours_args(ctx, "cc_neighbours_count", labels_dev, Z, Y, X, n, wz, wy, wx, r2, rho, rows));
    if (rows.n == 0 || n < 2) {  // (no offset lies inside the radius, or no two labels: no pair)
        *n_segments = 0;
        return DLV_OK;
    }
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    u64* words;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, W_WORDS * 8, (void**)&words));
    DLV_HIP(ctx, hipMemsetAsync(words, 0, W_WORDS * 8, ctx->stream));
    DlvProf pr(ctx, "cc_neighbours_count", 0.0, (double)Z * Y * X * 4);
    launch_scan<false>(ctx, labels_dev, Z, Y, X, n, wz, wy, wx, rho, rows, nullptr, 0, words);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_neighbours_kernel<count>");
    u64 s = 0;
    DLV_HIP(ctx, hipMemcpyAsync(&s, words + W_COUNT, 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_segments = s;
    return DLV_OK;
}

int dlv_cc_neighbours_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx, uint64_t r2,
                          uint64_t n_segments, uint64_t* table_dev, uint64_t cap, uint64_t* keys_out_dev, uint32_t* gap2_out_dev,
                          uint64_t out_cap, uint64_t* n_pairs) {
    if (!ctx || !labels_dev || !table_dev || !keys_out_dev || !gap2_out_dev || !n_pairs) return DLV_EINVAL;
    int rho[3];
    NbRows rows;
    DLV_TRY(neighbours_args(ctx, "cc_neighbours", labels_dev, Z, Y, X, n, wz, wy, wx, r2, rho, rows));
    if (((uintptr_t)table_dev & 15) || ((uintptr_t)keys_out_dev & 7) || ((uintptr_t)gap2_out_dev & 3))
        return dlv_fail(ctx, DLV_EINVAL, "cc_neighbours: the table must be 16-byte, the keys 8-byte, the gaps 4-byte aligned");
    // P <= min(S, n (n - 1) / 2)
    const u64 all_pairs = n < 2 ? 0 : (n % 2 ? n * ((n - 1) / 2) : (n / 2) * (n - 1));  // (n < 2^32: the product fits)
    const u64 bound = std::min<u64>(n_segments, all_pairs);
    if (bound > (1ull << 62))
        return dlv_fail(ctx, DLV_EINVAL, "cc_neighbours: %llu segments are beyond any table", (unsigned long long)n_segments);
    if (cap == 0 || (cap & (cap - 1)) || cap < 2 * bound)
        return dlv_fail(ctx, DLV_EINVAL, "cc_neighbours: a table of %llu slots; expected a power of two >= 2 * min(segments, n (n - 1) / 2) = %llu",
                        (unsigned long long)cap, (unsigned long long)(2 * bound));
    if (out_cap < bound)
        return dlv_fail(ctx, DLV_EINVAL, "cc_neighbours: outputs of %llu entries; min(segments, n (n - 1) / 2) = %llu",
                        (unsigned long long)out_cap, (unsigned long long)bound);
    if (bound == 0 || rows.n == 0) {  // no pair: nothing to launch
        *n_pairs = 0;
        return DLV_OK;
    }
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    u64* words;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, W_WORDS * 8, (void**)&words));
    DLV_HIP(ctx, hipMemsetAsync(words, 0, W_WORDS * 8, ctx->stream));
    {
        DlvProf pr(ctx, "cc_neighbours_table", 0.0, (double)Z * Y * X * 4 + (double)cap * 16);
        DLV_HIP(ctx, hipMemsetAsync(table_dev, 0, (size_t)cap * 16, ctx->stream));
        launch_scan<true>(ctx, labels_dev, Z, Y, X, n, wz, wy, wx, rho, rows, (u64*)table_dev, (u64)cap, words);
        pr.end();
    }
    DLV_LAUNCH_CHECK(ctx, "cc_neighbours_kernel<table>");
    {
        DlvProf pr(ctx, "cc_neighbours_compact", 0.0, (double)cap * 16);
        hipLaunchKernelGGL(pair_table_compact_kernel<u32>, dim3(pair_table_compact_grid(cap)), dim3(PT_CT), 0, ctx->stream, (const u64*)table_dev,
                           (u64)cap, (u64*)keys_out_dev, (u32*)gap2_out_dev, (u64)out_cap, words);
        pr.end();
    }
    DLV_LAUNCH_CHECK(ctx, "pair_table_compact_kernel");
    u64 host[W_WORDS] = {0, 0};
    DLV_HIP(ctx, hipMemcpyAsync(host, words, W_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (host[W_OVERFLOW])
        return dlv_fail(ctx, DLV_ESTATE, "cc_neighbours: the pair table of %llu slots (outputs of %llu entries) overflowed: %llu segments is "
                        "not the count of this volume", (unsigned long long)cap, (unsigned long long)out_cap, (unsigned long long)n_segments);
    *n_pairs = host[W_COUNT];
    return DLV_OK;
}

}  // extern "C"
