// fill_holes.hip - exact hole filling of a byte mask on the device, in place (dlv_fill_holes_u8_dev), and the count of marked
// voxels per label that tells afterwards which cell the fill gave how many voxels (dlv_cc_count_marked_dev).  The reference has no
// counterpart: its users call scipy.ndimage.binary_fill_holes(mask != 0) on the host, and that function (default structure) is what
// this computes.
//
// Definition.  The foreground is every voxel that is not 0.  Two background voxels are connected when they share a face; the
// voxels outside the volume count as background and are all connected to each other.  A hole is a background component with no
// voxel on any of the six faces of the volume, and filling writes fill_value over every voxel of every hole.  So:
//   - background that reaches the rest only over an edge or a corner is sealed (6-connected background is the dual of the
//     26-connected foreground dlv_ccl26_dev labels);
//   - a cavity open to a face of the volume is not a hole;
//   - a cell that lies inside the cavity of another cell is swallowed: after the fill both are one component;
//   - a hole never holds the first voxel (in raster order) of the component around it, so the labelling of the filled mask numbers
//     the surviving components in the order they had before.
//
// Algorithm.  Every hole voxel lies in a GAP: a maximal background stretch of a row (z, y) with foreground on both sides in that
// row - the background left of a row's first and right of its last foreground voxel reaches an x face.  The work after the first
// scan is proportional to the gaps of the mask, not to its background.
//   1. count: a wave per row reads the bytes 16 per lane and records the row's foreground extent [first, last] and its number of
//      gaps (its foreground runs - 1), and whether any byte equals fill_value; the counts are scanned into row_start.
//   2. emit: the rows that have gaps are read again; gap k of a row gets x0, x1 (uint16, inclusive) and its row at row_start + k.
//      Runs and gaps alternate, so with S(x) = the run starts at or before x, the background voxel x behind a run opens gap
//      S(x) - 1 and the run start x closes gap S(x) - 2.
//   3. union-find over the gaps with atomicMin links, as ccl.hip; node 0 is "outside" and gap g is node g + 1, so that the outside
//      is the root of everything it touches.  For each of the four rows (z +- 1, y), (z, y +- 1) of a gap: a row outside the volume,
//      or one whose extent does not cover [x0, x1], joins the gap to 0; the gaps of the two rows that precede in raster order whose
//      intervals overlap [x0, x1] - found by bisection in the row's slice of the gap table - are joined to it (overlap is
//      symmetric: the other two rows join from their side).
//   4. fill: a gap whose root is not 0 is part of a hole: its interval is written, its length added to voxels_filled, and the roots
//      other than 0 are the holes.
// Integer work only; what is written does not depend on the order of the unions: results are exact and independent of scheduling.
// No overflow: a volume has at most 2^32 voxels (checked), so at most 2^31 gaps: row_start and the node numbers fit 32 bits.
//
// Measured once on an MI355X (profiles/README.md, "fill_holes"): 1024 x 2048 x 2048, the bench's cell mask (0.22 % foreground, 4121
// holes) 2.5 ms beside 8.2 ms of dlv_ccl26_dev on the same mask; the same mask with every cell hollowed (494 764 holes) 3.1 ms.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"
#include "dev_scan.h"

#include <algorithm>

namespace {

constexpr int FT = 64;                 // threads per workgroup of the row kernels: one wave, one row at a time
constexpr u64 FILL_MAX_WG = 256 * 32;  // workgroups per launch; rows beyond that are walked grid-stride
constexpr u32 EXT_NONE = 1u;           // the extent (first | last << 16) of a row without foreground: first 1 > last 0 covers nothing

__device__ __forceinline__ u32 fh_find(const u32* __restrict__ P, u32 i) {
    u32 p;
    while ((p = __hip_atomic_load(P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != i) i = p;
    return i;
}

__device__ __forceinline__ void fh_union(u32* P, u32 a, u32 b) {
    bool done = false;
    while (!done) {
        a = fh_find(P, a);
        b = fh_find(P, b);
        if (a < b) {
            const u32 old = atomicMin(P + b, a);
            done = (old == b);
            b = old;
        } else if (b < a) {
            const u32 old = atomicMin(P + a, b);
            done = (old == a);
            a = old;
        } else {
            done = true;
        }
    }
}

// foreground bits of the 16 voxels [x, x + 16) of a row (bit k = voxel x + k, 0 past the row's end): one 16-byte load where the
// row starts on a 16-byte boundary (x is a multiple of 16) and the chunk is whole.  bad: a byte equals fv (fv != 0)
__device__ __forceinline__ unsigned row_bits16(const uint8_t* __restrict__ row, u32 x, u32 X, bool vec, u32 fv, bool& bad) {
    unsigned bits = 0;
    if (x >= X) return 0u;
    if (vec && x + 16u <= X) {
        const uint4 u = *reinterpret_cast<const uint4*>(row + x);
        if ((u.x | u.y | u.z | u.w) == 0u) return 0u;
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned v = (w[q] >> (8 * b)) & 0xffu;
                bits |= (v ? 1u : 0u) << (4 * q + b);
                bad |= v == fv;
            }
    } else {
        for (u32 k = 0; k < 16u && x + k < X; ++k) {
            const unsigned v = row[x + k];
            bits |= (v ? 1u : 0u) << k;
            bad |= v == fv;
        }
    }
    return bits;
}

__device__ __forceinline__ int fill_sweeps(int X) { return (X + FT * 16 - 1) / (FT * 16); }

// ---- count: counts[row] = the gaps of the row, ext[row] = its foreground extent; *bad_flag = 1 where a byte equals fv ----------
__global__ void __launch_bounds__(FT) fill_count_kernel(const uint8_t* __restrict__ mask, u64 nrows, int X, u32 fv, u32* __restrict__ counts,
                                                        u32* __restrict__ ext, u32* __restrict__ bad_flag) {
    const int lane = threadIdx.x & 63;
    const int sweeps = fill_sweeps(X);
    bool bad = false;
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const uint8_t* row = mask + r * (u64)X;
        const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
        u32 c = 0, first = NO_VOXEL, last = 0;
        unsigned carrybit = 0;  // the last voxel of the sweep before is foreground
        for (int sw = 0; sw < sweeps; ++sw) {
            const u32 x = (u32)sw * (FT * 16) + 16u * lane;
            const unsigned bits = row_bits16(row, x, (u32)X, vec, fv, bad);
            if (!__any(bits != 0)) {  // (wave-uniform) nothing but background in these 1024 voxels
                carrybit = 0;
                continue;
            }
            const unsigned up = __shfl_up(bits, 1, 64);
            const unsigned leftbit = lane == 0 ? carrybit : (up >> 15) & 1u;
            const unsigned starts = bits & ~((bits << 1) | leftbit) & 0xffffu;
            c += (u32)__popc(starts);
            if (bits) {
                first = min(first, x + (u32)(__ffs((int)bits) - 1));
                last = max(last, x + (u32)(31 - __clz((int)bits)));
            }
            carrybit = (__shfl(bits, 63, 64) >> 15) & 1u;
        }
        for (int o = 32; o > 0; o >>= 1) {
            xor_add(c, o);
            xor_min(first, o);
            xor_max(last, o);
        }
        if (lane == 0) {
            counts[r] = c ? c - 1u : 0u;
            ext[r] = c ? (first | (last << 16)) : EXT_NONE;
        }
    }
    if (__any(bad) && lane == 0) *bad_flag = 1u;
}

// ---- emit: x0 / x1 / row of every gap at row_start[row] + its rank in the row; parent[node] = node ------------------------------
__global__ void __launch_bounds__(FT) fill_emit_kernel(const uint8_t* __restrict__ mask, u64 nrows, int X, const u32* __restrict__ row_start,
                                                       u32 n_gaps, unsigned short* __restrict__ x0, unsigned short* __restrict__ x1,
                                                       u32* __restrict__ grow) {
    const int lane = threadIdx.x & 63;
    const int sweeps = fill_sweeps(X);
    bool bad = false;  // (not used here: the count has looked)
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u32 g0 = row_start[r], ng = row_start[r + 1] - g0;
        if (ng == 0) continue;  // (wave-uniform) a row without a gap
        const uint8_t* row = mask + r * (u64)X;
        const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
        u32 carry = 0;          // the run starts of the sweeps before this one (<= X)
        unsigned carrybit = 0;  // the last voxel of the sweep before is foreground
        for (int sw = 0; sw < sweeps; ++sw) {
            const u32 x = (u32)sw * (FT * 16) + 16u * lane;
            const unsigned bits = row_bits16(row, x, (u32)X, vec, 0x100u, bad);
            const unsigned valid = x >= (u32)X ? 0u : ((u32)X - x >= 16u ? 0xffffu : (1u << ((u32)X - x)) - 1u);
            const unsigned up = __shfl_up(bits, 1, 64);
            const unsigned leftbit = lane == 0 ? carrybit : (up >> 15) & 1u;
            const unsigned left = (bits << 1) | leftbit;
            const unsigned starts = bits & ~left & 0xffffu;  // foreground behind background (or the row's start)
            const unsigned opens = ~bits & left & valid;     // background behind foreground
            const u32 own = (u32)__popc(starts);
            u32 incl = own;
            for (int o = 1; o < 64; o <<= 1) {
                const u32 t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            const u32 total = __shfl(incl, 63, 64), before = carry + incl - own;
            unsigned m = starts | opens;
            while (m) {
                const int k = __ffs((int)m) - 1;
                m &= m - 1;
                const u32 S = before + (u32)__popc(starts & ((2u << k) - 1u));  // the run starts at or before x + k
                if ((starts >> k) & 1u) {
                    if (S >= 2u && S - 2u < ng && g0 + (S - 2u) < n_gaps) x1[g0 + (S - 2u)] = (unsigned short)(x + k - 1u);
                } else if (S >= 1u && S - 1u < ng && g0 + (S - 1u) < n_gaps) {  // (behind the row's last run: S - 1 == ng, no gap)
                    x0[g0 + (S - 1u)] = (unsigned short)(x + k);
                    grow[g0 + (S - 1u)] = (u32)r;
                }
            }
            carry += total;
            carrybit = (__shfl(bits, 63, 64) >> 15) & 1u;
        }
    }
}

__global__ void __launch_bounds__(256) fill_iota_kernel(u32* __restrict__ parent, u64 n) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) parent[i] = (u32)i;
}

// ---- union: one thread per gap ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fill_union_kernel(int Z, int Y, const u32* __restrict__ row_start, const u32* __restrict__ ext,
                                                         u32 n_gaps, const unsigned short* __restrict__ x0,
                                                         const unsigned short* __restrict__ x1, const u32* __restrict__ grow, u32* parent) {
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < n_gaps; g += (u64)gridDim.x * blockDim.x) {
        const u32 r = grow[g], a = x0[g], b = x1[g];
        if ((u64)r >= (u64)Z * Y) continue;  // (cannot happen: the emit has written every gap's row)
        const int z = (int)(r / (u32)Y), y = (int)(r % (u32)Y);
        const int dzs[4] = {-1, 0, 0, 1}, dys[4] = {0, -1, 1, 0};
        bool outside = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int zz = z + dzs[k], yy = y + dys[k];
            if (zz < 0 || zz >= Z || yy < 0 || yy >= Y) {
                outside = true;
                continue;
            }
            const u64 nr = (u64)zz * Y + yy;
            const u32 e = ext[nr];
            if (!((e & 0xffffu) <= a && b <= (e >> 16))) outside = true;  // a background voxel of that row reaches an x face
            if (k >= 2) continue;  // (the rows behind this one join from their side)
            u32 lo = row_start[nr], hi = row_start[nr + 1];
            const u32 end = min(hi, n_gaps);
            while (lo < hi) {  // the first gap of the row that ends at or behind a
                const u32 mid = lo + ((hi - lo) >> 1);
                if ((u32)x1[mid] < a) lo = mid + 1;
                else hi = mid;
            }
            for (u32 j = lo; j < end && (u32)x0[j] <= b; ++j) fh_union(parent, (u32)g + 1u, j + 1u);
        }
        if (outside) fh_union(parent, (u32)g + 1u, 0u);
    }
}

// ---- fill: the gaps whose root is not the outside -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fill_write_kernel(uint8_t* __restrict__ mask, u64 nrows, int X, u32 n_gaps, const unsigned short* __restrict__ x0,
                                                         const unsigned short* __restrict__ x1, const u32* __restrict__ grow,
                                                         const u32* __restrict__ parent, uint8_t fv, u64* __restrict__ voxels,
                                                         u32* __restrict__ holes) {
    u64 nv = 0;
    u32 nh = 0;
    const u64 span = ((u64)n_gaps + blockDim.x - 1) / blockDim.x * blockDim.x;  // (workgroup-uniform trip count)
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < span; g += (u64)gridDim.x * blockDim.x) {
        if (g >= n_gaps) continue;
        u32 root = (u32)g + 1u, p;
        while ((p = parent[root]) != root) root = p;  // (nobody writes parent any more)
        if (root == 0u) continue;
        const u32 a = x0[g], b = x1[g];
        const u64 r = grow[g];
        if (b < a || b >= (u32)X || r >= nrows) continue;  // (cannot happen: the write stays inside the volume whatever the table holds)
        uint8_t* row = mask + r * (u64)X;
        for (u32 x = a; x <= b; ++x) row[x] = fv;
        nv += b - a + 1u;
        nh += root == (u32)g + 1u ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        xor_add(nv, o);
        xor_add(nh, o);
    }
    if ((threadIdx.x & 63) == 0 && nv) {
        atomicAdd(voxels, nv);
        if (nh) atomicAdd(holes, nh);
    }
}

// ---- marked voxels per label --------------------------------------------------------------------------------------------------
// cc_counts_kernel's flat tiles of 2048 voxels (cc_stats.hip) with the mask read first: a wave whose 512 voxels hold no marked
// byte - nearly all of them - never loads its labels.  One atomic per (wave, label), folded as cc_fold.h describes.
constexpr int MTILE = 256 * VPT;

struct MarkAcc {
    u32 c;
    static __device__ __forceinline__ MarkAcc none() { return {0u}; }
    __device__ __forceinline__ void combine(int o) { xor_add(c, o); }
};

__device__ __forceinline__ void marked_fold(const u32 (&l)[VPT], unsigned marked, u32 n, u32* __restrict__ counts, u32& nbg) {
#pragma unroll
    for (int k = 0; k < VPT; ++k) nbg += (((marked >> k) & 1u) && l[k] == 0) ? 1u : 0u;
    unsigned todo = marked & fg_mask(l, n);
    while (__any(todo != 0)) {  // one pass per distinct label of the thread
        const bool have = todo != 0;
        const u32 lab = first_label(l, todo);
        MarkAcc own = MarkAcc::none();
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const bool in = ((todo >> k) & 1u) && l[k] == lab;
            own.c += in ? 1u : 0u;
            todo &= ~((in ? 1u : 0u) << k);
        }
        wave_fold_by_label<true>(lab, have, own, [&](u32 L, const MarkAcc& w) { atomicAdd(counts + L, w.c); });
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) cc_count_marked_kernel(const u32* __restrict__ labels, const uint8_t* __restrict__ mask, u64 nvox,
                                                              u32 n, u32 value, u32* __restrict__ counts) {
    const u64 ntiles = nvox / MTILE;
    u32 nbg = 0;
    u32 l[VPT];
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (workgroup-uniform trip count: the shuffles are convergent)
        const u64 base = tile * MTILE + 4u * threadIdx.x;
        unsigned marked = 0;
        if (VEC) {
            const u32 m0 = __builtin_nontemporal_load(reinterpret_cast<const u32*>(mask + base));
            const u32 m1 = __builtin_nontemporal_load(reinterpret_cast<const u32*>(mask + base + MTILE / 2));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                marked |= (((m0 >> (8 * k)) & 0xffu) == value ? 1u : 0u) << k;
                marked |= (((m1 >> (8 * k)) & 0xffu) == value ? 1u : 0u) << (4 + k);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                marked |= (mask[base + k] == value ? 1u : 0u) << k;
                marked |= (mask[base + MTILE / 2 + k] == value ? 1u : 0u) << (4 + k);
            }
        }
        if (!__any(marked != 0)) continue;  // (wave-uniform)
        if (VEC) {
            const u32x4_t u0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(labels + base));
            const u32x4_t u1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(labels + base + MTILE / 2));
            l[0] = u0.x; l[1] = u0.y; l[2] = u0.z; l[3] = u0.w;
            l[4] = u1.x; l[5] = u1.y; l[6] = u1.z; l[7] = u1.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                l[k] = labels[base + k];
                l[4 + k] = labels[base + MTILE / 2 + k];
            }
        }
        marked_fold(l, marked, n, counts, nbg);
    }
    if (blockIdx.x == gridDim.x - 1 && ntiles * MTILE < nvox) {  // the last partial tile
        const u64 base = ntiles * MTILE + (u64)threadIdx.x * VPT;
        unsigned marked = 0;
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const bool in = base + k < nvox;
            l[k] = in ? labels[base + k] : NO_VOXEL;
            marked |= ((in && mask[base + k] == value) ? 1u : 0u) << k;
        }
        marked_fold(l, marked, n, counts, nbg);
    }
    for (int o = 32; o > 0; o >>= 1) xor_add(nbg, o);
    if ((threadIdx.x & 63) == 0 && nbg) atomicAdd(counts, nbg);
}

}  // namespace

extern "C" {

int dlv_fill_holes_u8_dev(dlv_ctx* ctx, uint8_t* mask_dev, int Z, int Y, int X, uint8_t fill_value, uint64_t* voxels_filled,
                          uint64_t* holes) {
    if (!ctx || !mask_dev || !voxels_filled || !holes) return DLV_EINVAL;
    DLV_TRY(check_volume(ctx, "fill_holes", Z, Y, X));
    if (fill_value == 0) return dlv_fail(ctx, DLV_EINVAL, "fill_holes: fill_value 0 is the background");
    if (X > 65536) return dlv_fail(ctx, DLV_EUNSUP, "fill_holes: X = %d, x0 / x1 are uint16", X);
    const u64 nrows = (u64)Z * Y;
    if (nrows > (((u64)1 << 32) / (u64)X)) return dlv_fail(ctx, DLV_EUNSUP, "fill_holes: volumes above 2^32 voxels are not supported");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    // row table (slot WS_CCL; the labelling that follows takes the slot over): [row_start u32 nrows + 1 | extent u32 nrows |
    // group sums u32, one per scan group (<= 2^22: one workgroup per group in the scan) | bad flag u32, holes u32, voxels u64]
    WsCarve c;
    const size_t rows_off = c.take(((size_t)nrows + 1) * 4), ext_off = c.take((size_t)nrows * 4);
    const size_t gsum_off = c.take((size_t)scan_groups(nrows) * 4), out_off = c.take(16);
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_CCL, c.end, (void**)&ws));
    u32* row_start = (u32*)(ws + rows_off);
    u32* ext = (u32*)(ws + ext_off);
    u32* gsum = (u32*)(ws + gsum_off);
    u32* bad_flag = (u32*)(ws + out_off);
    u32* holes_dev = bad_flag + 1;
    u64* voxels_dev = (u64*)(ws + out_off + 8);
    DLV_HIP(ctx, hipMemsetAsync(ws + out_off, 0, 16, ctx->stream));
    const unsigned grows = (unsigned)std::min<u64>(nrows, FILL_MAX_WG);
    DlvProf pr(ctx, "fill_holes", 0.0, (double)nrows * X);
    hipLaunchKernelGGL(fill_count_kernel, dim3(grows), dim3(FT), 0, ctx->stream, mask_dev, nrows, X, (u32)fill_value, row_start, ext, bad_flag);
    DLV_LAUNCH_CHECK(ctx, "fill_count_kernel");
    // the counts become row_start in place, row_start[nrows] the number of gaps (<= 2^31)
    DLV_TRY(dev_excl_scan(ctx, row_start, nrows, row_start, gsum, row_start + nrows, "fill_scan_kernel"));
    u32 bad = 0, n_gaps = 0;
    DLV_HIP(ctx, hipMemcpyAsync(&bad, bad_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(&n_gaps, row_start + nrows, 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) return dlv_fail(ctx, DLV_EINVAL, "fill_holes: the mask already holds fill_value %d", (int)fill_value);
    *voxels_filled = 0;
    *holes = 0;
    if (n_gaps == 0) return DLV_OK;  // no row has background between foreground: no hole
    // gap table (slot WS_MISC): [parent u32 n_gaps + 1 | row u32 n_gaps | x0 u16 n_gaps | x1 u16 n_gaps]
    WsCarve g;
    const size_t parent_off = g.take(((size_t)n_gaps + 1) * 4), grow_off = g.take((size_t)n_gaps * 4);
    const size_t x0_off = g.take((size_t)n_gaps * 2), x1_off = g.take((size_t)n_gaps * 2);
    char* gs;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, g.end, (void**)&gs));
    u32* parent = (u32*)(gs + parent_off);
    u32* grow = (u32*)(gs + grow_off);
    unsigned short* x0 = (unsigned short*)(gs + x0_off);
    unsigned short* x1 = (unsigned short*)(gs + x1_off);
    const unsigned ggaps = (unsigned)std::min<u64>(((u64)n_gaps + 256) / 256, (u64)256 * 32);
    DLV_HIP(ctx, hipMemsetAsync(grow, 0xff, (size_t)n_gaps * 4, ctx->stream));  // (a row that is none, until the emit names it)
    hipLaunchKernelGGL(fill_iota_kernel, dim3(ggaps), dim3(256), 0, ctx->stream, parent, (u64)n_gaps + 1);
    hipLaunchKernelGGL(fill_emit_kernel, dim3(grows), dim3(FT), 0, ctx->stream, mask_dev, nrows, X, row_start, n_gaps, x0, x1, grow);
    DLV_LAUNCH_CHECK(ctx, "fill_emit_kernel");
    hipLaunchKernelGGL(fill_union_kernel, dim3(ggaps), dim3(256), 0, ctx->stream, Z, Y, row_start, ext, n_gaps, x0, x1, grow, parent);
    DLV_LAUNCH_CHECK(ctx, "fill_union_kernel");
    hipLaunchKernelGGL(fill_write_kernel, dim3(ggaps), dim3(256), 0, ctx->stream, mask_dev, nrows, X, n_gaps, x0, x1, grow, parent, fill_value,
                       voxels_dev, holes_dev);
    DLV_LAUNCH_CHECK(ctx, "fill_write_kernel");
    pr.end();
    u32 nh = 0;
    u64 nv = 0;
    DLV_HIP(ctx, hipMemcpyAsync(&nh, holes_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(&nv, voxels_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *voxels_filled = nv;
    *holes = nh;
    return DLV_OK;
}

int dlv_cc_count_marked_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint8_t* mask_dev, uint64_t nvox, uint64_t n, uint8_t value,
                            uint32_t* counts_dev) {
    if (!ctx || !labels_dev || !mask_dev || !counts_dev) return DLV_EINVAL;
    DLV_TRY(check_label_count(ctx, "cc_count_marked", n));
    if ((uintptr_t)labels_dev & 3) return dlv_fail(ctx, DLV_EINVAL, "labels must be 4-byte aligned");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    DLV_HIP(ctx, hipMemsetAsync(counts_dev, 0, ((size_t)n + 1) * 4, ctx->stream));
    if (nvox == 0) return DLV_OK;
    const int gs = (int)std::min<u64>(std::max<u64>(nvox / MTILE, 1), (u64)256 * 32);
    DlvProf pr(ctx, "cc_count_marked", 0.0, (double)nvox);
    if ((((uintptr_t)labels_dev & 15) | ((uintptr_t)mask_dev & 3)) == 0)
        hipLaunchKernelGGL(cc_count_marked_kernel<true>, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, mask_dev, (u64)nvox, (u32)n,
                           (u32)value, counts_dev);
    else
        hipLaunchKernelGGL(cc_count_marked_kernel<false>, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, mask_dev, (u64)nvox, (u32)n,
                           (u32)value, counts_dev);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_count_marked_kernel");
    return DLV_OK;
}

}  // extern "C"
