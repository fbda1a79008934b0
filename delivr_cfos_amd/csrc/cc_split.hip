// cc_split.hip - fused cells split by their erosion cores (dlv_cc_split_dev): two nuclei that touch in the mask are one
// 26-connected component and one row of the cell table.  The labels are eroded `depth` times with the 6 face neighbours, what is
// left of a label are its cores; a label with two or more cores is divided among them by growing the cores back through the
// label, every voxel going to the core nearest to it in 26-steps inside its own label (the smallest core label on a tie).  The
// reference has no counterpart; its users run a watershed on the host from the label file.
//
//   C_0 = L != 0;  C_{k+1}(v) = C_k(v) and C_k(u) for the 6 face neighbours u (outside the volume: background);  C = C_depth.
//   Q = the 26-connected components of C (dlv_ccl26_dev; min_core > 1: dlv_cc_size_filter_dev drops the smaller ones), 1..M.
//   G_0 = Q;  G_{k+1}(v) = G_k(v) where that is not 0, else where L(v) != 0 the smallest non-zero G_k(u) over the 26 neighbours u
//   with L(u) == L(v) (0 without one);  G = the fixed point.
//   key(v) = 0 where L(v) == 0, G(v) where L(v) holds two or more cores and G(v) != 0, M + L(v) otherwise; the distinct keys are
//   the pieces, numbered in raster order of their first voxel.
//
// Only labels with two or more cores are grown: G_0 holds their cores alone, the voxels of every other label hold SKIP and are
// never pending.  Integer work only; one writer per voxel in the sweeps, and the tables are written with atomicMin / atomicAdd
// or by writers that agree: the result is exact and independent of scheduling.
//
// dlv_cc_split_depth_dev is the same split with other cores, for stacks whose voxels are not cubes (one erosion step takes a
// whole plane off a cell that is two planes thick): C(v) = D2(v) >= T(L(v)), with D2 the exact label-wise distance map of
// cc_depth.hip in integer spacings and T(l) = max(core_d2, ceil(core_pct^2 m(l) / 10000), 1) from the largest D2 of the label - a
// Euclidean erosion in physical units.  D2 lies in work_a, the byte mask goes to work_b, and from Q on both entries run
// split_from_cores.  The threshold cannot be folded into the z pass of the map: m(l) is known only when that pass has ended.
#include "common.h"
#include "cc_check.h"
#include "cc_tile.h"  // (the tile of the growth)

#include <algorithm>

namespace {

constexpr u32 NONE = 0xffffffffu;          // "no core reaches" while the minimum is taken
constexpr u32 SKIP = 0xffffffffu;          // G of a voxel whose label is not split: never pending, never a neighbour of a pending voxel
constexpr int BATCH = 8;                   // growth steps between two read-backs of the change flags

// tile states of the growth (one word per tile, read and written by the tile's own workgroup only)
constexpr u32 T_DONE = 0;     // nothing pending, both buffers hold the tile
constexpr u32 T_PENDING = 1;  // holds a voxel with L != 0 and G == 0 (or has not been looked at yet)
constexpr u32 T_CARRY = 2;    // completed by the last step: the step's destination holds it, the other buffer not yet

// bit j: p[j] != 0, for j < valid (<= 4); one 4- or 16-byte load where the four are whole and aligned
__device__ __forceinline__ unsigned nz4(const uint8_t* __restrict__ p, int valid) {
    if (valid == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const u32 w = *reinterpret_cast<const u32*>(p);
        return ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
    }
    unsigned b = 0;
    for (int j = 0; j < valid; ++j) b |= (p[j] ? 1u : 0u) << j;
    return b;
}
__device__ __forceinline__ unsigned nz4(const u32* __restrict__ p, int valid) {
    if (valid == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const u32x4_t w = *reinterpret_cast<const u32x4_t*>(p);
        return (w.x ? 1u : 0u) | (w.y ? 2u : 0u) | (w.z ? 4u : 0u) | (w.w ? 8u : 0u);
    }
    unsigned b = 0;
    for (int j = 0; j < valid; ++j) b |= (p[j] ? 1u : 0u) << j;
    return b;
}

// p[j] = bit j of c, for j < valid (<= 4): one 4-byte store where the four are whole and aligned
__device__ __forceinline__ void store_mask4(uint8_t* __restrict__ p, int valid, unsigned c) {
    if (valid == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<u32*>(p) = (c & 1u) | ((c & 2u) << 7) | ((c & 4u) << 14) | ((c & 8u) << 21);
    } else {
        for (int j = 0; j < valid; ++j) p[j] = (uint8_t)((c >> j) & 1u);
    }
}

// One erosion step: dst = C_{k+1} of src = C_k (a byte mask), or of the labels for the first step.  A thread takes four voxels
// along x; the neighbour rows are read only where the four and their x neighbours left something (cells: < 1 % foreground).
template <typename T>
__global__ void __launch_bounds__(256) split_erode_kernel(const T* __restrict__ src, int Z, int Y, int X, uint8_t* __restrict__ dst) {
    const int qx = (X + 3) / 4;
    const u64 total = (u64)Z * Y * qx;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) {
        const int x = (int)(t % (u64)qx) * 4;
        const u64 row = t / (u64)qx;
        const int y = (int)(row % (u64)Y), z = (int)(row / (u64)Y);
        const int valid = min(4, X - x);
        const u64 at = row * (u64)X + x;
        unsigned c = nz4(src + at, valid);
        if (c) {
            unsigned wide = c << 1;  // bit j + 1: voxel x + j; bits 0 and 5: the voxels left and right of the four
            if (x > 0 && src[at - 1] != 0) wide |= 1u;
            if (x + 4 < X && src[at + 4] != 0) wide |= 1u << 5;
            c &= wide & (wide >> 2);
            if (c) c &= y > 0 ? nz4(src + at - (u64)X, valid) : 0u;
            if (c) c &= y + 1 < Y ? nz4(src + at + (u64)X, valid) : 0u;
            if (c) c &= z > 0 ? nz4(src + at - (u64)Y * X, valid) : 0u;
            if (c) c &= z + 1 < Z ? nz4(src + at + (u64)Y * X, valid) : 0u;
        }
        store_mask4(dst + at, valid, c);
    }
}

// T(l) of dlv_cc_split_depth_dev for the rows 0..n: key[l] >> 32 is m(l), the largest D2 of label l (cc_depth.hip's peak keys)
__global__ void __launch_bounds__(256) split_depth_threshold_kernel(const u64* __restrict__ key, u64 N, u32 core_d2, u32 core_pct,
                                                                    u32* __restrict__ T) {
    for (u64 l = (u64)blockIdx.x * blockDim.x + threadIdx.x; l <= N; l += (u64)gridDim.x * blockDim.x) {
        const u64 m = key[l] >> 32;
        const u64 part = ((u64)core_pct * core_pct * m + 9999u) / 10000u;  // (< 2^14 * 2^32; <= m)
        T[l] = (u32)max(max((u64)core_d2, part), (u64)1);
    }
}

// The cores of dlv_cc_split_depth_dev: dst(v) = 1 where 1 <= L(v) <= n and D2(v) >= T(L(v)), else 0.  A thread takes four voxels
// along x, as split_erode_kernel: one 16-byte load of the labels and one of the map where the four are whole and aligned, and T is
// read only under a voxel the map measured (D2 != 0: a label 1..n; cells: < 1 % of the voxels).
__global__ void __launch_bounds__(256) split_depth_cores_kernel(const u32* __restrict__ L, const u32* __restrict__ D2,
                                                                const u32* __restrict__ T, u32 n, int Z, int Y, int X,
                                                                uint8_t* __restrict__ dst) {
    const int qx = (X + 3) / 4;
    const u64 total = (u64)Z * Y * qx;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) {
        const int x = (int)(t % (u64)qx) * 4;
        const u64 at = (t / (u64)qx) * (u64)X + x;
        const int valid = min(4, X - x);
        u32 l[4] = {0, 0, 0, 0}, d[4] = {0, 0, 0, 0};
        if (valid == 4 && ((reinterpret_cast<uintptr_t>(L + at) | reinterpret_cast<uintptr_t>(D2 + at)) & 15) == 0) {
            const u32x4_t lq = *reinterpret_cast<const u32x4_t*>(L + at), dq = *reinterpret_cast<const u32x4_t*>(D2 + at);
            l[0] = lq.x; l[1] = lq.y; l[2] = lq.z; l[3] = lq.w;
            d[0] = dq.x; d[1] = dq.y; d[2] = dq.z; d[3] = dq.w;
        } else {
            for (int j = 0; j < valid; ++j) {
                l[j] = L[at + j];
                d[j] = D2[at + j];
            }
        }
        unsigned c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d[j] != 0 && l[j] >= 1 && l[j] <= n && d[j] >= T[l[j]]) c |= 1u << j;
        store_mask4(dst + at, valid, c);
    }
}

// comp[q] = the label of core q's voxels (a core lies inside one label: every writer stores the same value); one store per run
__global__ void __launch_bounds__(256) split_comp_kernel(const u32* __restrict__ Q, const u32* __restrict__ L, u64 n, int X,
                                                         u32* __restrict__ comp) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 q = Q[i];
        if (q && (i % (u64)X == 0 || Q[i - 1] != q)) comp[q] = L[i];
    }
}

// cores[l] = the number of cores in label l; a core whose label lies above n (refused by split_seed_kernel) is not counted
__global__ void __launch_bounds__(256) split_cores_kernel(const u32* __restrict__ comp, u64 M, u64 N, u32* __restrict__ cores) {
    for (u64 q = 1 + (u64)blockIdx.x * blockDim.x + threadIdx.x; q <= M; q += (u64)gridDim.x * blockDim.x) {
        const u32 l = comp[q];
        if (l >= 1 && l <= N) atomicAdd(cores + l, 1u);
    }
}

// word[0] = the number of labels with two or more cores
__global__ void __launch_bounds__(256) split_count_kernel(const u32* __restrict__ cores, u64 N, u32* __restrict__ word) {
    u32 c = 0;
    for (u64 l = 1 + (u64)blockIdx.x * blockDim.x + threadIdx.x; l <= N; l += (u64)gridDim.x * blockDim.x) c += cores[l] >= 2 ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(word, c);
}

// G_0 into both buffers of the growth (a holds Q): the core label where the voxel's label is split, SKIP on the rest of the
// foreground, 0 on the background and on the voxels a core has to reach.  word[1] is raised by a label above n.
__global__ void __launch_bounds__(256) split_seed_kernel(const u32* __restrict__ L, u64 n, u64 N, const u32* __restrict__ cores,
                                                         u32* a, u32* __restrict__ b, u32* __restrict__ word) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 l = L[i];
        u32 g = 0;
        if (l) {
            if (l > N) {
                word[1] = 1u;
                g = SKIP;
            } else {
                g = cores[l] >= 2 ? a[i] : SKIP;
            }
        }
        a[i] = g;
        b[i] = g;
    }
}

// One growth step: dst = G_{k+1} of src = G_k on the tiles that still hold a pending voxel (L != 0, G == 0).  A workgroup of 256
// threads owns the TZ x TY x TX voxels at (blockIdx.z, .y, .x) and their state word.  T_DONE: nothing is read.  T_CARRY: the
// tile is copied from src to dst, which lacks the last step's result, and is T_DONE from then on.  T_PENDING: the tile's own
// voxels of G_k and of the labels are staged in LDS; without a pending voxel among them (the first look at a tile: both buffers
// hold G_0) the tile is T_DONE and its neighbourhood is never read.  Otherwise the one-voxel halo follows (outside the volume:
// label 0, which no pending voxel has), every pending voxel takes the smallest G_k among its 26 neighbours of its own label, and
// the whole tile is written to dst - the assigned voxels are carried forward, so dst holds all of G_{k+1} on it.  A step that
// assigns a voxel raises *changed; a tile that has no pending voxel left becomes T_CARRY.
__global__ void __launch_bounds__(256) split_grow_kernel(const u32* __restrict__ labels, const u32* __restrict__ src, u32* __restrict__ dst,
                                                         int Z, int Y, int X, u32* __restrict__ state, u32* __restrict__ changed, int first_step) {
    __shared__ __attribute__((aligned(16))) u32 gt[ROWS * PITCH];
    __shared__ __attribute__((aligned(16))) u32 lt[ROWS * PITCH];
    const u64 tile = ((u64)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const u32 st = state[tile];  // (workgroup-uniform: written by this tile's workgroup of the step before)
    if (st == T_DONE) return;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = blockIdx.z * TZ;
    const TileAt t(Z, Y, X);
    auto quad_of = [&](const u32* __restrict__ vol, int row, int q) -> u32x4_t { return tile_quad_of(vol, t, row, q); };
    auto store_quad = [&](u32* p, int x, u32x4_t v) { tile_store_quad(p, x, X, v); };
    auto carry = [&]() {  // dst = src on the tile's own voxels
        for (int i = threadIdx.x; i < TZ * TY * QX; i += 256) {
            const int q = i % QX, oy = (i / QX) % TY, oz = i / (QX * TY);
            const int z = z0 + oz, y = y0 + oy, x = x0 + 4 * q;
            if (z >= Z || y >= Y || x >= X) continue;
            store_quad(dst + ((u64)z * Y + y) * (u64)X + x, x, quad_of(src, (oz + 1) * (TY + 2) + oy + 1, q));
        }
    };
    if (st == T_CARRY) {
        carry();
        if (threadIdx.x == 0) state[tile] = T_DONE;
        return;
    }

    bool pending = false;
    for (int i = threadIdx.x; i < TZ * TY * QX; i += 256) {  // the tile's own voxels
        const int q = i % QX, row = (i / (QX * TY) + 1) * (TY + 2) + (i / QX) % TY + 1;
        const u32x4_t g = quad_of(src, row, q), l = quad_of(labels, row, q);
        pending = pending || (l.x && !g.x) || (l.y && !g.y) || (l.z && !g.z) || (l.w && !g.w);
        *reinterpret_cast<u32x4_t*>(gt + row * PITCH + 4 + 4 * q) = g;
        *reinterpret_cast<u32x4_t*>(lt + row * PITCH + 4 + 4 * q) = l;
    }
    if (!__syncthreads_or(pending)) {  // (workgroup-uniform)
        if (!first_step) carry();  // (the first step finds dst equal to src: both hold G_0; a later one must not rely on that)
        if (threadIdx.x == 0) state[tile] = T_DONE;
        return;
    }
    for (int i = threadIdx.x; i < ROWS * QX; i += 256) {  // the halo rows
        const int row = i / QX, q = i % QX;
        const int rz = row / (TY + 2), ry = row % (TY + 2);
        if (rz >= 1 && rz <= TZ && ry >= 1 && ry <= TY) continue;
        *reinterpret_cast<u32x4_t*>(gt + row * PITCH + 4 + 4 * q) = quad_of(src, row, q);
        *reinterpret_cast<u32x4_t*>(lt + row * PITCH + 4 + 4 * q) = quad_of(labels, row, q);
    }
    for (int i = threadIdx.x; i < ROWS * 2; i += 256) {  // the voxels left and right of every row
        const int row = i >> 1, right = i & 1;
        const int z = z0 - 1 + row / (TY + 2), y = y0 - 1 + row % (TY + 2), x = right ? x0 + TX : x0 - 1;
        u32 g = 0, l = 0;
        if (z >= 0 && z < Z && y >= 0 && y < Y && x >= 0 && x < X) {
            const u64 at = ((u64)z * Y + y) * (u64)X + x;
            g = src[at];
            l = labels[at];
        }
        gt[row * PITCH + (right ? 4 + TX : 3)] = g;
        lt[row * PITCH + (right ? 4 + TX : 3)] = l;
    }
    __syncthreads();

    bool grew = false, left = false;
    for (int i = threadIdx.x; i < TZ * TY * QX; i += 256) {
        const int q = i % QX, oy = (i / QX) % TY, oz = i / (QX * TY);
        const int z = z0 + oz, y = y0 + oy, x = x0 + 4 * q;
        if (z >= Z || y >= Y || x >= X) continue;
        const int centre = ((oz + 1) * (TY + 2) + oy + 1) * PITCH + 4 + 4 * q;
        const u32x4_t gq = *reinterpret_cast<const u32x4_t*>(gt + centre), lq = *reinterpret_cast<const u32x4_t*>(lt + centre);
        u32 g[4] = {gq.x, gq.y, gq.z, gq.w};
        const u32 l[4] = {lq.x, lq.y, lq.z, lq.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (g[j] != 0 || l[j] == 0) continue;  // (a voxel beyond the end of the row was staged as label 0)
            u32 m = NONE;
            for (int dz = 0; dz < 3; ++dz)
                for (int dy = 0; dy < 3; ++dy) {
                    const int r = ((oz + dz) * (TY + 2) + oy + dy) * PITCH + 3 + 4 * q + j;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const u32 gu = gt[r + dx];
                        if (lt[r + dx] == l[j] && gu != 0 && gu < m) m = gu;  // (the voxel itself: gu == 0)
                    }
                }
            if (m != NONE) {
                g[j] = m;
                grew = true;
            } else {
                left = true;
            }
        }
        store_quad(dst + ((u64)z * Y + y) * (u64)X + x, x, u32x4_t{g[0], g[1], g[2], g[3]});
    }
    const int any_grew = __syncthreads_or(grew), any_left = __syncthreads_or(left);
    if (threadIdx.x == 0) {
        if (any_grew) *changed = 1u;
        state[tile] = any_left ? T_PENDING : T_CARRY;
    }
}

__device__ __forceinline__ u32 key_of(u32 l, u32 g, u32 M) { return (g != 0 && g != SKIP) ? g : M + l; }

// first[key] = the smallest linear index of the piece (first is preset to 0xffffffff); one atomicMin per run of a key in a row
__global__ void __launch_bounds__(256) split_first_kernel(const u32* __restrict__ L, const u32* __restrict__ G, u64 n, int X, u32 M,
                                                          u32* __restrict__ first) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 l = L[i];
        if (!l) continue;
        const u32 key = key_of(l, G[i], M);
        if (i % (u64)X != 0 && L[i - 1] != 0 && key_of(L[i - 1], G[i - 1], M) == key) continue;
        atomicMin(first + key, (u32)i);
    }
}

// the pieces as a forest for dlv_ccl_number_forest: every foreground voxel holds the index of its piece's first voxel
__global__ void __launch_bounds__(256) split_forest_kernel(const u32* __restrict__ L, const u32* __restrict__ G, u64 n, u32 M,
                                                           const u32* __restrict__ first, u32* __restrict__ forest) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 l = L[i];
        forest[i] = l ? first[key_of(l, G[i], M)] : 0u;
    }
}

// labels = the pieces, parent[piece] = the label it was cut from (every writer of a row stores the same value; one per run)
__global__ void __launch_bounds__(256) split_apply_kernel(u32* __restrict__ L, const u32* __restrict__ pieces, u64 n, int X,
                                                          u32* __restrict__ parent) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 l = L[i];
        if (!l) continue;
        const u32 p = pieces[i];
        if (i % (u64)X == 0 || pieces[i - 1] != p) parent[p] = l;
        L[i] = p;
    }
}

// the checks the two entries share, in two parts with an entry's own checks between them: the pointers and the shape ...
int split_check_pointers(dlv_ctx* ctx, const char* what, const uint32_t* labels_dev, int Z, int Y, int X, const uint32_t* work_a_dev,
                         const uint32_t* work_b_dev, const uint64_t* n_out, const uint64_t* n_split_out, const uint32_t* parent_dev) {
    if (!labels_dev || !work_a_dev || !work_b_dev) return dlv_fail(ctx, DLV_EINVAL, "%s: labels_dev, work_a_dev or work_b_dev is NULL", what);
    if (!n_out || !n_split_out || !parent_dev) return dlv_fail(ctx, DLV_EINVAL, "%s: n_out, n_split_out or parent_dev is NULL", what);
    return check_volume(ctx, what, Z, Y, X);
}
// ... and min_core, the alignment, the tile grid of the growth, the 32-bit indices and labels, the three volumes apart
int split_check_volumes(dlv_ctx* ctx, const char* what, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int64_t min_core,
                        const uint32_t* work_a_dev, const uint32_t* work_b_dev, const uint32_t* parent_dev) {
    if (min_core < 1) return dlv_fail(ctx, DLV_EINVAL, "%s: min_core %lld is below 1", what, (long long)min_core);
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)work_a_dev & 3) || ((uintptr_t)work_b_dev & 3) || ((uintptr_t)parent_dev & 3))
        return dlv_fail(ctx, DLV_EINVAL, "%s: labels, work_a, work_b and parent must be 4-byte aligned", what);
    DLV_TRY(check_tile_grid(ctx, what, tile_grid(Z, Y, X), Z, Y, X));
    const u64 nvox = (u64)Z * Y * X;
    if (nvox > ((u64)1 << 32)) return dlv_fail(ctx, DLV_EUNSUP, "%s: volumes above 2^32 voxels need 64-bit labels", what);
    DLV_TRY(check_label_count(ctx, what, n));
    const size_t bytes = (size_t)nvox * 4;
    if (ranges_overlap(work_a_dev, labels_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "%s: work_a_dev overlaps labels_dev", what);
    if (ranges_overlap(work_b_dev, labels_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "%s: work_b_dev overlaps labels_dev", what);
    if (ranges_overlap(work_b_dev, work_a_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "%s: work_b_dev overlaps work_a_dev", what);
    return DLV_OK;
}

// Steps (2) - (4) of the two entries, for checked arguments: `core_mask` is the byte mask C of the cores, somewhere in work_b_dev;
// work_a_dev holds nothing that is still needed.  Synchronous.
int split_from_cores(dlv_ctx* ctx, const char* what, uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int64_t min_core,
                     const uint8_t* core_mask, uint32_t* work_a_dev, uint32_t* work_b_dev, uint64_t* n_out, uint64_t* n_split_out,
                     uint32_t* parent_dev, uint64_t parent_cap) {
    const dim3 grid = tile_grid(Z, Y, X);
    const u64 nvox = (u64)Z * Y * X;
    const int flat = (int)std::min<u64>((nvox + 255) / 256, (u64)256 * 64);  // the grid-stride kernels over the voxels
    auto rows_grid = [](u64 rows) { return dim3((unsigned)std::min<u64>(std::max<u64>((rows + 255) / 256, 1), (u64)256 * 32)); };
    // (2) the labels Q of the cores in work_a, 1..M
    uint64_t M = 0;
    DLV_TRY(dlv_ccl26_dev(ctx, core_mask, Z, Y, X, work_a_dev, &M));
    if (min_core > 1 && M > 0) {
        u32* sizes;  // (the labelling has returned: its scratch slot is free, and the filter does not touch it)
        DLV_TRY(dlv_ws_get(ctx, WS_CCL, ((size_t)M + 1) * 4, (void**)&sizes));
        DLV_TRY(dlv_cc_counts_dev(ctx, work_a_dev, nvox, M, sizes));
        DLV_TRY(dlv_cc_size_filter_dev(ctx, work_a_dev, nvox, M, sizes, min_core, -1, &M));
    }
    if (M + n >= 0xffffffffull)
        return dlv_fail(ctx, DLV_EINVAL, "%s: %llu cores and n = %llu do not fit the uint32 keys", what, (unsigned long long)M, (unsigned long long)n);

    // tables: comp (M + 1), cores (n + 1), first (M + n + 1), the tile states, the change flags of a batch, two words
    // (the labels that are split, "a label above n")
    const u64 ntiles = (u64)grid.x * grid.y * grid.z;
    WsCarve c;
    const size_t comp_off = c.take(((size_t)M + 1) * 4), cores_off = c.take(((size_t)n + 1) * 4), first_off = c.take(((size_t)M + n + 1) * 4);
    const size_t state_off = c.take((size_t)ntiles * 4), flags_off = c.take(BATCH * 4), word_off = c.take(256);
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, c.end, (void**)&ws));
    u32 *comp = (u32*)(ws + comp_off), *cores = (u32*)(ws + cores_off), *first = (u32*)(ws + first_off);
    u32 *state = (u32*)(ws + state_off), *flags = (u32*)(ws + flags_off), *word = (u32*)(ws + word_off);
    DLV_HIP(ctx, hipMemsetAsync(ws, 0, first_off, ctx->stream));                              // comp, cores
    DLV_HIP(ctx, hipMemsetAsync(first, 0xff, ((size_t)M + n + 1) * 4, ctx->stream));
    DLV_HIP(ctx, hipMemsetAsync(word, 0, 8, ctx->stream));
    if (M > 0) {
        hipLaunchKernelGGL(split_comp_kernel, dim3(flat), dim3(256), 0, ctx->stream, (const u32*)work_a_dev, (const u32*)labels_dev, nvox, X, comp);
        hipLaunchKernelGGL(split_cores_kernel, rows_grid(M), dim3(256), 0, ctx->stream, (const u32*)comp, (u64)M, (u64)n, cores);
        hipLaunchKernelGGL(split_count_kernel, rows_grid(n), dim3(256), 0, ctx->stream, (const u32*)cores, (u64)n, word);
        DLV_LAUNCH_CHECK(ctx, "split_cores_kernel");
    }
    hipLaunchKernelGGL(split_seed_kernel, dim3(flat), dim3(256), 0, ctx->stream, (const u32*)labels_dev, nvox, (u64)n, (const u32*)cores,
                       work_a_dev, work_b_dev, word);
    DLV_LAUNCH_CHECK(ctx, "split_seed_kernel");
    u32 host_word[2] = {0, 0};
    DLV_HIP(ctx, hipMemcpyAsync(host_word, word, 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (host_word[1]) return dlv_fail(ctx, DLV_EINVAL, "%s: the volume holds a label above n = %llu", what, (unsigned long long)n);

    // (3) the growth, only with something to split: a step reads one buffer and writes the other; the flags of BATCH steps are
    // read back together, and the loop ends with the first step that assigned nothing - from that step on a step changes
    // nothing, and after it both buffers hold G on every tile (the kernel's note), so the steps a batch ran beyond it are harmless
    u32* G = work_a_dev;
    if (host_word[0]) {
        DlvProf p3(ctx, "cc_split_grow", 0.0, 0.0);
        DLV_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)state, (int)T_PENDING, (size_t)ntiles, ctx->stream));
        u32 *src = work_a_dev, *dst = work_b_dev;
        int first_step = 1;
        for (bool done = false; !done;) {
            DLV_HIP(ctx, hipMemsetAsync(flags, 0, BATCH * 4, ctx->stream));
            for (int k = 0; k < BATCH; ++k) {
                hipLaunchKernelGGL(split_grow_kernel, grid, dim3(256), 0, ctx->stream, (const u32*)labels_dev, (const u32*)src, dst, Z, Y, X, state,
                                   flags + k, first_step);
                first_step = 0;
                std::swap(src, dst);
            }
            DLV_LAUNCH_CHECK(ctx, "split_grow_kernel");
            u32 host_flags[BATCH];
            DLV_HIP(ctx, hipMemcpyAsync(host_flags, flags, BATCH * 4, hipMemcpyDeviceToHost, ctx->stream));
            DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            for (int k = 0; k < BATCH; ++k) done = done || host_flags[k] == 0;
        }
        p3.end();
        G = src;
    }
    u32* pieces = G == work_a_dev ? work_b_dev : work_a_dev;

    // (4) the pieces: first voxel per key, the forest of those first voxels, dlv_ccl26_dev's renumbering, the relabel pass
    DlvProf p4(ctx, "cc_split_number", 0.0, (double)nvox * 36.0);
    hipLaunchKernelGGL(split_first_kernel, dim3(flat), dim3(256), 0, ctx->stream, (const u32*)labels_dev, (const u32*)G, nvox, X, (u32)M, first);
    hipLaunchKernelGGL(split_forest_kernel, dim3(flat), dim3(256), 0, ctx->stream, (const u32*)labels_dev, (const u32*)G, nvox, (u32)M,
                       (const u32*)first, pieces);
    DLV_LAUNCH_CHECK(ctx, "split_forest_kernel");
    uint64_t K = 0;
    DLV_TRY(dlv_ccl_number_forest(ctx, labels_dev, pieces, nvox, &K));
    *n_out = K;
    *n_split_out = host_word[0];
    if (parent_cap < K + 1)
        return dlv_fail(ctx, DLV_EINVAL, "%s: parent_dev of %llu rows does not hold the %llu pieces and row 0", what, (unsigned long long)parent_cap,
                        (unsigned long long)K);
    DLV_HIP(ctx, hipMemsetAsync(parent_dev, 0, ((size_t)K + 1) * 4, ctx->stream));
    hipLaunchKernelGGL(split_apply_kernel, dim3(flat), dim3(256), 0, ctx->stream, labels_dev, (const u32*)pieces, nvox, X, parent_dev);
    DLV_LAUNCH_CHECK(ctx, "split_apply_kernel");
    p4.end();
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DLV_OK;
}

}  // namespace

extern "C" int dlv_cc_split_dev(dlv_ctx* ctx, uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int depth, int64_t min_core,
                                uint32_t* work_a_dev, uint32_t* work_b_dev, uint64_t* n_out, uint64_t* n_split_out,
                                uint32_t* parent_dev, uint64_t parent_cap) {
    if (!ctx) return DLV_EINVAL;
    DLV_TRY(split_check_pointers(ctx, "cc_split", labels_dev, Z, Y, X, work_a_dev, work_b_dev, n_out, n_split_out, parent_dev));
    if (depth < 1 || depth > 16) return dlv_fail(ctx, DLV_EINVAL, "cc_split: depth %d is outside 1..16", depth);
    DLV_TRY(split_check_volumes(ctx, "cc_split", labels_dev, Z, Y, X, n, min_core, work_a_dev, work_b_dev, parent_dev));
    const u64 nvox = (u64)Z * Y * X;
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    DlvProf pr(ctx, "cc_split", 0.0, 0.0);

    // (1) the cores: `depth` erosion steps between two byte masks that live in work_b until the cores are labelled
    uint8_t* mask[2] = {(uint8_t*)work_b_dev, (uint8_t*)work_b_dev + (nvox >= 16 ? (nvox + 15) / 16 * 16 : nvox)};
    {
        DlvProf p1(ctx, "cc_split_erode", 0.0, (double)nvox * (5.0 + 2.0 * (depth - 1)));
        const int ge = (int)std::min<u64>(((u64)Z * Y * ((X + 3) / 4) + 255) / 256, (u64)256 * 64);
        for (int i = 1; i <= depth; ++i) {
            if (i == 1)
                hipLaunchKernelGGL(split_erode_kernel<u32>, dim3(ge), dim3(256), 0, ctx->stream, (const u32*)labels_dev, Z, Y, X, mask[1]);
            else
                hipLaunchKernelGGL(split_erode_kernel<uint8_t>, dim3(ge), dim3(256), 0, ctx->stream, (const uint8_t*)mask[(i - 1) & 1], Z, Y, X,
                                   mask[i & 1]);
        }
        p1.end();
        DLV_LAUNCH_CHECK(ctx, "split_erode_kernel");
    }
    DLV_TRY(split_from_cores(ctx, "cc_split", labels_dev, Z, Y, X, n, min_core, mask[depth & 1], work_a_dev, work_b_dev, n_out, n_split_out,
                             parent_dev, parent_cap));
    pr.end();
    return DLV_OK;
}

extern "C" int dlv_cc_split_depth_dev(dlv_ctx* ctx, uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                                      uint32_t core_d2, int core_pct, int64_t min_core, uint32_t* work_a_dev, uint32_t* work_b_dev,
                                      uint64_t* n_out, uint64_t* n_split_out, uint32_t* parent_dev, uint64_t parent_cap) {
    const char* what = "cc_split_depth";
    if (!ctx) return DLV_EINVAL;
    DLV_TRY(split_check_pointers(ctx, what, labels_dev, Z, Y, X, work_a_dev, work_b_dev, n_out, n_split_out, parent_dev));
    DLV_TRY(check_spacing(ctx, what, "z", wz));
    DLV_TRY(check_spacing(ctx, what, "y", wy));
    DLV_TRY(check_spacing(ctx, what, "x", wx));
    if (core_pct < 0 || core_pct > 99) return dlv_fail(ctx, DLV_EINVAL, "%s: core_pct %d is outside 0..99", what, core_pct);
    if (core_d2 == 0 && core_pct == 0) return dlv_fail(ctx, DLV_EINVAL, "%s: core_d2 and core_pct are both 0: no core is defined", what);
    DLV_TRY(check_reach(ctx, what, "z", wz, Z));  // (each dimension is below 2^17 from here on: no wrap of Z * Y * X)
    DLV_TRY(check_reach(ctx, what, "y", wy, Y));
    DLV_TRY(check_reach(ctx, what, "x", wx, X));
    DLV_TRY(split_check_volumes(ctx, what, labels_dev, Z, Y, X, n, min_core, work_a_dev, work_b_dev, parent_dev));
    const u64 nvox = (u64)Z * Y * X;
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    DlvProf pr(ctx, "cc_split_depth", 0.0, 0.0);

    // (1) D2 in work_a and the peak keys of the labels; (2) T(l) from the keys, then the cores as a byte mask at the start of
    // work_b: work_b's values of the y pass are dead since the z pass, and D2 is dead once this kernel has read it
    DlvDepthTables t;
    DLV_TRY(dlv_cc_depth_passes(ctx, labels_dev, Z, Y, X, n, wz, wy, wx, work_a_dev, work_b_dev, ((size_t)n + 1) * 4, &t));
    {
        DlvProf p2(ctx, "cc_split_depth_cores", 0.0, (double)nvox * 9.0);
        const int gt = (int)std::min<u64>((n + 1 + 255) / 256, (u64)256 * 32);
        const int gc = (int)std::min<u64>(((u64)Z * Y * ((X + 3) / 4) + 255) / 256, (u64)256 * 64);
        hipLaunchKernelGGL(split_depth_threshold_kernel, dim3(gt), dim3(256), 0, ctx->stream, (const u64*)t.key, (u64)n, (u32)core_d2,
                           (u32)core_pct, (u32*)t.extra);
        hipLaunchKernelGGL(split_depth_cores_kernel, dim3(gc), dim3(256), 0, ctx->stream, (const u32*)labels_dev, (const u32*)work_a_dev,
                           (const u32*)t.extra, (u32)n, Z, Y, X, (uint8_t*)work_b_dev);
        p2.end();
        DLV_LAUNCH_CHECK(ctx, "split_depth_cores_kernel");
    }
    // (the tables of the distance map are read by launches queued before split_from_cores asks for their scratch slot again)
    DLV_TRY(split_from_cores(ctx, what, labels_dev, Z, Y, X, n, min_core, (const uint8_t*)work_b_dev, work_a_dev, work_b_dev, n_out,
                             n_split_out, parent_dev, parent_cap));
    pr.end();
    return DLV_OK;
}
