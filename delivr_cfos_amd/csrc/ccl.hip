// ccl.hip - 26-connected component labelling on the device, the seam merge of slabs labelled on several GPUs and the size
// filter.  (The per-label statistics of the labels: cc_stats.hip.)
//
// Replaces cc3d.connected_components(bin_img, return_N=True) (count_blobs.py:61; cc3d 3.12.3 is a
// third-party C++ two-pass union-find, not vendored).  Output contract: label(component) = 1 + rank of its
// minimum linear index z*Y*X + y*X + x among all components; 0 = background.
//
// Algorithm: union-find over the voxel index space with atomicMin links (the root of a tree is
// the minimum linear index of its component), 13 backward neighbours per foreground voxel, path
// compression, then a raster-order renumbering of the roots by a two-level prefix sum.  Integer
// work only: results are bit-exact and independent of scheduling.
#include "common.h"
#include "cc_check.h"
#include "dev_scan.h"
#include <cstdlib>

namespace {

__device__ __forceinline__ u32 uf_find(const u32* __restrict__ L, u32 i) {
    u32 p;
    while ((p = __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != i) i = p;
    return i;
}

__device__ __forceinline__ void uf_union(u32* L, u32 a, u32 b) {
    bool done = false;
    while (!done) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a < b) {
            const u32 old = atomicMin(L + b, a);
            done = (old == b);
            b = old;
        } else if (b < a) {
            const u32 old = atomicMin(L + a, b);
            done = (old == a);
            a = old;
        } else {
            done = true;
        }
    }
}

// foreground bits of the 16 voxels [i0, i0 + 16) of the mask (bit k = voxel i0 + k); one 16-byte load when the chunk is
// whole and the mask pointer is 16-byte aligned (i0 is a multiple of 16).  A sparse mask (cells: < 1 % foreground) is
// scanned at 16 voxels per load, and every kernel below returns early on a chunk without foreground.
__device__ __forceinline__ unsigned mask_bits16(const uint8_t* __restrict__ mask, u64 i0, u64 n, bool aligned) {
    unsigned bits = 0;
    if (aligned && i0 + 16 <= n) {
        const uint4 u = *reinterpret_cast<const uint4*>(mask + i0);
        if ((u.x | u.y | u.z | u.w) == 0u) return 0u;
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if ((w[q] >> (8 * b)) & 0xffu) bits |= 1u << (4 * q + b);
    } else {
        for (int k = 0; k < 16; ++k)
            if (i0 + k < n && mask[i0 + k]) bits |= 1u << k;
    }
    return bits;
}

// chunks per workgroup of ccl_init_kernel: whole iterations of its 256 threads.  The kernel and the launch record of
// dlv_ccl26_dev (dlv_diag_ccl_ran) ask the same function
__host__ __device__ __forceinline__ u64 ccl_init_per(u64 nch, u64 grid) { return ((nch + grid - 1) / grid + 255) / 256 * 256; }

// parents of the foreground voxels only (the background entries of L are never read: 17 GB of writes less on a
// 2^32-voxel volume)
// ... and the BIT MASK of the volume (one uint16 per 16 voxels): the only pass that reads the byte mask.  Every later
// kernel scans 1/8 byte per voxel instead of 1 (five scans: 6 -> 1.6 bytes per voxel on top of the 4 of the labels).
__global__ void __launch_bounds__(256) ccl_init_kernel(const uint8_t* __restrict__ mask, u32* __restrict__ L, u64 n,
                                                       bool aligned, unsigned short* __restrict__ bm, u32* __restrict__ list,
                                                       u32* __restrict__ list_n) {
    // A workgroup owns a contiguous range of chunks.  The chunks that hold foreground are collected in LDS and appended to
    // the global list with ONE atomic per flush (a per-wave atomic on the single counter serialised: 11 ms); the order of
    // the list is whatever the flushes give - the unions do not depend on it.  The union / compress / relabel kernels
    // then run over the list with every lane busy instead of a few per wave.
    constexpr int CAP = 2048;
    __shared__ u32 buf[CAP];
    __shared__ u32 fill, gbase;
    const u64 nch = (n + 15) / 16;
    const int lane = threadIdx.x & 63;
    const u64 per = ccl_init_per(nch, gridDim.x);
    const u64 cb = (u64)blockIdx.x * per, ce = min(cb + per, nch);
    if (threadIdx.x == 0) fill = 0;
    __syncthreads();
    auto flush = [&]() {  // (called by the whole workgroup)
        __syncthreads();
        const u32 cnt = fill;
        if (threadIdx.x == 0 && cnt) gbase = atomicAdd(list_n, cnt);
        __syncthreads();
        for (u32 i = threadIdx.x; i < cnt; i += 256) list[gbase + i] = buf[i];
        __syncthreads();
        if (threadIdx.x == 0) fill = 0;
        __syncthreads();
    };
    for (u64 c0 = cb; c0 < ce; c0 += 256) {  // (workgroup-uniform trip count)
        const u64 c = c0 + threadIdx.x;
        unsigned bits = c < ce ? mask_bits16(mask, c * 16, n, aligned) : 0u;
        if (c < ce) bm[c] = (unsigned short)bits;
        const unsigned long long hit = __ballot(bits != 0u);
        if (hit) {
            u32 base = 0;
            if (lane == 0) base = atomicAdd(&fill, (u32)__popcll(hit));
            base = __shfl(base, 0, 64);
            if (bits) buf[base + (u32)__popcll(hit & ((1ull << lane) - 1ull))] = (u32)c;
        }
        while (bits) {
            const int k = __ffs((int)bits) - 1;
            bits &= bits - 1;
            L[c * 16 + k] = (u32)(c * 16 + k);
        }
        __syncthreads();
        const u32 f = fill;  // every thread reads the value all adds of this iteration produced ...
        __syncthreads();     // ... and nobody adds for the next iteration before everybody has read it: the decision is uniform
        if (f > CAP - 256) flush();
    }
    flush();
}

// one thread per 16 consecutive voxels (linear index; a chunk may straddle rows): for every foreground voxel the
// 13 neighbours that precede it in raster order
__device__ __forceinline__ void ccl_merge_chunk(const unsigned short* __restrict__ bm, u32* __restrict__ L, int Y, int X, u64 c) {
    unsigned bits = bm[c];
    while (bits) {
        const int k = __ffs((int)bits) - 1;
        bits &= bits - 1;
        const u64 i = c * 16 + k;
        const int x = (int)(i % (u64)X);
        const u64 r = i / (u64)X;
        const int y = (int)(r % (u64)Y), z = (int)(r / (u64)Y);
        for (int dz = -1; dz <= 0; ++dz) {
            const int zz = z + dz;
            if (zz < 0) continue;
            const int dy_hi = dz < 0 ? 1 : 0;
            for (int dy = -1; dy <= dy_hi; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= Y) continue;
                const int dx_hi = (dz < 0 || dy < 0) ? 1 : -1;
                for (int dx = -1; dx <= dx_hi; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= X) continue;
                    const u64 j = ((u64)zz * Y + yy) * X + xx;
                    if ((bm[j >> 4] >> (j & 15)) & 1u) uf_union(L, (u32)i, (u32)j);
                }
            }
        }
    }
}

// The same unions for volumes whose rows are whole 16-voxel chunks (X % 16 == 0, aligned mask): the thread's chunk and the
// four neighbour rows that precede it in raster order - (z-1, y-1), (z-1, y), (z-1, y+1), (z, y-1) - are read as 16-byte
// chunks (+ the two voxels left and right of each) into 18-bit windows, and every foreground voxel is united with a
// REDUCED neighbour set: its left neighbour, and per neighbour row the voxel straight above (x) if that is foreground,
// else the diagonal ones (x-1, x+1) that are.  (x-1, x, x+1) of one row are chained by that row's own left-neighbour
// unions, so the centre stands for all three: the components are the same, with a third of the find/atomicMin traffic and
// no per-voxel byte loads.
__device__ __forceinline__ void ccl_merge_rows_chunk(const unsigned short* __restrict__ bm, u32* __restrict__ L, int Y, int X, u64 c,
                                                     unsigned bits) {
    const int cpr = X / 16;  // chunks per row
    const int x0 = (int)(c % (u64)cpr) * 16;
    const u64 row = c / (u64)cpr;
    const int y = (int)(row % (u64)Y), z = (int)(row / (u64)Y);
    // 18-bit window of a row around this chunk: bit k+1 <-> voxel x0 + k, bit 0 <-> x0 - 1, bit 17 <-> x0 + 16
    auto window = [&](u64 cch) -> unsigned {  // cch = chunk index of (row, x0): its 16 bits, the last of the chunk before, the first of the one after
        unsigned w = (unsigned)bm[cch] << 1;
        if (x0 > 0) w |= (unsigned)bm[cch - 1] >> 15;
        if (x0 + 16 < X) w |= ((unsigned)bm[cch + 1] & 1u) << 17;
        return w;
    };
    const u64 base = c * 16;
    const unsigned cur = (bits << 1) | (x0 > 0 ? (unsigned)bm[c - 1] >> 15 : 0u);
    u64 nbase[4];
    unsigned nwin[4];
    const int dzs[4] = {-1, -1, -1, 0}, dys[4] = {-1, 0, 1, -1};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int zz = z + dzs[r], yy = y + dys[r];
        nwin[r] = 0;
        nbase[r] = 0;
        if (zz >= 0 && yy >= 0 && yy < Y) {
            nbase[r] = ((u64)zz * Y + yy) * X + x0;
            nwin[r] = window(nbase[r] >> 4);
        }
    }
    while (bits) {
        const int k = __ffs((int)bits) - 1;
        bits &= bits - 1;
        const u32 i = (u32)(base + k);
        if ((cur >> k) & 1u) uf_union(L, i, i - 1);  // (x - 1) of this row
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned w3 = (nwin[r] >> k) & 7u;  // x-1, x, x+1 of the neighbour row
            if (!w3) continue;
            const u32 j = (u32)(nbase[r] + k);
            if (w3 & 2u) {
                uf_union(L, i, j);
            } else {
                if (w3 & 1u) uf_union(L, i, j - 1);
                if (w3 & 4u) uf_union(L, i, j + 1);
            }
        }
    }
}

// one thread per listed (= foreground) chunk; ROWS: the row-window form above (X % 16 == 0), else the per-voxel form
template <bool ROWS>
__global__ void __launch_bounds__(256) ccl_merge_list_kernel(const unsigned short* __restrict__ bm, u32* __restrict__ L, int Y, int X,
                                                             const u32* __restrict__ list, const u32* __restrict__ list_n) {
    const u32 cnt = *list_n;
    for (u32 t = blockIdx.x * blockDim.x + threadIdx.x; t < cnt; t += gridDim.x * blockDim.x) {
        const u64 c = list[t];
        if (ROWS) ccl_merge_rows_chunk(bm, L, Y, X, c, bm[c]);
        else ccl_merge_chunk(bm, L, Y, X, c);
    }
}

__global__ void __launch_bounds__(256) ccl_compress_kernel(const unsigned short* __restrict__ bm, u32* __restrict__ L,
                                                           const u32* __restrict__ list, const u32* __restrict__ list_n) {
    const u32 cnt = *list_n;
    for (u32 t = blockIdx.x * blockDim.x + threadIdx.x; t < cnt; t += gridDim.x * blockDim.x) {
        const u64 c = list[t];
        unsigned bits = bm[c];
        while (bits) {
            const int k = __ffs((int)bits) - 1;
            bits &= bits - 1;
            const u64 i = c * 16 + k;
            u32 r = (u32)i, p;
            while ((p = L[r]) != r) r = p;
            L[i] = r;  // racing writers store the same root; readers that see an older parent still reach it
        }
    }
}

constexpr int RPT = 16;                 // voxels per thread in the renumbering kernels
constexpr int RCHUNK = 256 * RPT;       // voxels per block

__global__ void __launch_bounds__(256) ccl_count_roots_kernel(const unsigned short* __restrict__ bm, const u32* __restrict__ L,
                                                              u64 n, u32* __restrict__ counts) {
    const u64 base = (u64)blockIdx.x * RCHUNK + (u64)threadIdx.x * RPT;
    int c = 0;
    unsigned bits = base < n ? (unsigned)bm[base >> 4] : 0u;
    while (bits) {
        const int k = __ffs((int)bits) - 1;
        bits &= bits - 1;
        if (L[base + k] == (u32)(base + k)) ++c;
    }
    int total;
    block_excl_scan(c, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = (u32)total;
}

// The union-find runs IN the label volume (round 6: L == labels; the separate parent array was 4 bytes per voxel of scratch -
// 17 GB for 2^32 voxels, 0.5 s of device allocation on a process's first labelling).  A root's entry becomes its label here; which
// entries are roots is recorded in a bit mask (one uint16 per 16 voxels, like bm) for the relabel pass: a non-root entry still
// holds its root's INDEX, and an index cannot be told from a label by its value.
__global__ void __launch_bounds__(256) ccl_assign_roots_kernel(const unsigned short* __restrict__ bm, const u32* __restrict__ L,
                                                               u64 n, const u32* __restrict__ offsets,
                                                               u32* __restrict__ labels, unsigned short* __restrict__ rb) {
    const u64 base = (u64)blockIdx.x * RCHUNK + (u64)threadIdx.x * RPT;
    int c = 0;
    unsigned roots = 0;
    unsigned bits = base < n ? (unsigned)bm[base >> 4] : 0u;
    while (bits) {
        const int k = __ffs((int)bits) - 1;
        bits &= bits - 1;
        if (L[base + k] == (u32)(base + k)) {
            ++c;
            roots |= 1u << k;
        }
    }
    if (base < n) rb[base >> 4] = (unsigned short)roots;  // (RPT == 16: a thread's voxels are one word of the bit masks)
    int total;
    u32 rank = offsets[blockIdx.x] + (u32)block_excl_scan(c, &total);
    while (roots) {
        const int k = __ffs((int)roots) - 1;
        roots &= roots - 1;
        labels[base + k] = ++rank;
    }
}

// every voxel of the label volume is written exactly once here (16 voxels = four 16-byte stores per thread): 0 for the
// background, the root's label for the rest (roots already hold theirs)
__global__ void __launch_bounds__(256) ccl_relabel_kernel(const unsigned short* __restrict__ bm, const unsigned short* __restrict__ rb,
                                                          u64 n, u32* labels, bool aligned) {
    const u64 nch = (n + 15) / 16;
    for (u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += (u64)gridDim.x * blockDim.x) {
        const u64 base = c * 16;
        const unsigned bits = bm[c], rbits = rb[c];
        u32 v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            v[k] = 0;
            if (bits & (1u << k)) {
                const u32 x = labels[base + k];             // a root: its label (ccl_assign_roots_kernel); else: its root's index
                v[k] = (rbits & (1u << k)) ? x : labels[x];  // (a root's entry never changes again: racing readers see its label)
            }
        }
        if (aligned && base + 16 <= n) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<uint4*>(labels + base + 4 * q) = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
            for (int k = 0; k < 16 && base + k < n; ++k) labels[base + k] = v[k];
        }
    }
}

// The label volume was zeroed (hipMemsetAsync: the fill runs at 6.9 TB/s); only the listed chunks are written
__global__ void __launch_bounds__(256) ccl_relabel_list_kernel(const unsigned short* __restrict__ bm, const unsigned short* __restrict__ rb, u64 n,
                                                               u32* labels, const u32* __restrict__ list,
                                                               const u32* __restrict__ list_n, bool aligned) {
    const u32 cnt = *list_n;
    for (u32 t = blockIdx.x * blockDim.x + threadIdx.x; t < cnt; t += gridDim.x * blockDim.x) {
        const u64 c = list[t], base = c * 16;
        const unsigned bits = bm[c], rbits = rb[c];
        u32 v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            v[k] = 0;
            if (bits & (1u << k)) {
                const u32 x = labels[base + k];             // a root: its label; else: its root's index (the volume is its own parent array)
                v[k] = (rbits & (1u << k)) ? x : labels[x];
            }
        }
        if (aligned && base + 16 <= n) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<uint4*>(labels + base + 4 * q) = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
            for (int k = 0; k < 16 && base + k < n; ++k) labels[base + k] = v[k];
        }
    }
}

// The same label volume with whole-line stores: a wave owns 1024 consecutive voxels and writes them with four store
// instructions of 64 x 16 contiguous bytes (the kernel above gives every lane 64 contiguous bytes, i.e. four instructions that
// each touch a quarter of 64 lines).  Needs the 16-byte alignment; the last partial block is written voxel by voxel.
__global__ void __launch_bounds__(256) ccl_relabel_lines_kernel(const unsigned short* __restrict__ bm, const unsigned short* __restrict__ rb, u64 n,
                                                                u32* labels) {
    const int lane = threadIdx.x & 63;
    const u64 nblk = n / 1024;
    const u64 wave0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 blk = wave0; blk < nblk; blk += nwaves) {
        const u64 base = blk * 1024;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u64 o = base + (u64)q * 256 + (u64)lane * 4;
            const unsigned m = ((unsigned)bm[o >> 4] >> (o & 15)) & 15u;  // this lane's four voxels (four lanes share a word)
            const unsigned rt = ((unsigned)rb[o >> 4] >> (o & 15)) & 15u;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (m) {  // (an entry is a root's label, or the index of its root - whose entry is its label and never changes again)
                const uint4 x = *reinterpret_cast<const uint4*>(labels + o);
                if (m & 1u) v.x = (rt & 1u) ? x.x : labels[x.x];
                if (m & 2u) v.y = (rt & 2u) ? x.y : labels[x.y];
                if (m & 4u) v.z = (rt & 4u) ? x.z : labels[x.z];
                if (m & 8u) v.w = (rt & 8u) ? x.w : labels[x.w];
            }
            *reinterpret_cast<uint4*>(labels + o) = v;
        }
    }
    if (wave0 == 0)
        for (u64 i = nblk * 1024 + lane; i < n; i += 64) {
            u32 v = 0u;
            if ((bm[i >> 4] >> (i & 15)) & 1u) {
                const u32 x = labels[i];
                v = ((rb[i >> 4] >> (i & 15)) & 1u) ? x : labels[x];
            }
            labels[i] = v;
        }
}

// The bit mask of a volume that is labelled already (bit k of word c: voxel 16 c + k holds a label): what ccl_init_kernel makes
// of the byte mask, for dlv_ccl_number_forest
__global__ void __launch_bounds__(256) ccl_bits_of_labels_kernel(const u32* __restrict__ fg, u64 n, unsigned short* __restrict__ bm) {
    const u64 nch = (n + 15) / 16;
    for (u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += (u64)gridDim.x * blockDim.x) {
        unsigned bits = 0;
        for (int k = 0; k < 16; ++k)
            if (c * 16 + k < n && fg[c * 16 + k] != 0u) bits |= 1u << k;
        bm[c] = (unsigned short)bits;
    }
}

// ---- multi-GPU seam merge: slabs are labelled independently; these kernels supply the pairs of
// labels that touch across a slab boundary and apply the global renumbering --------------------------------------
// a = labels of the last plane of the upper slab, b = labels of the first plane of the slab below it.  Every
// 26-adjacency across the seam is one of the 9 (dy,dx) neighbours in b of a voxel in a.  Emits (a,b) when the
// pair differs from the one the same voxel produced for the previous neighbour (cheap local dedupe; the host
// makes the list unique).  pairs == nullptr: count only.
__global__ void __launch_bounds__(256) seam_pairs_kernel(const u32* __restrict__ a, const u32* __restrict__ b, int Y, int X,
                                                         u32* __restrict__ pairs, u64 cap, u64* __restrict__ count) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (u64)Y * X) return;
    const u32 la = a[t];
    if (!la) return;
    const int x = (int)(t % X), y = (int)(t / X);
    u32 prev = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if ((unsigned)yy >= (unsigned)Y) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if ((unsigned)xx >= (unsigned)X) continue;
            const u32 lb = b[(u64)yy * X + xx];
            if (!lb || lb == prev) continue;
            prev = lb;
            const u64 slot = atomicAdd(count, 1ull);
            if (pairs && slot < cap) {
                pairs[2 * slot] = la;
                pairs[2 * slot + 1] = lb;
            }
        }
    }
}

__global__ void __launch_bounds__(256) relabel_lut_kernel(u32* __restrict__ labels, u64 n, const u32* __restrict__ lut, u32 head) {
    // 4 labels per thread (16-byte accesses); background (0) maps to lut[0] = 0 without a table read.  head (< 4): the labels in
    // front of the first 16-byte boundary of a volume that does not start on one - they and the tail go one by one
    if (blockIdx.x == 0 && threadIdx.x >= 4 && threadIdx.x - 4 < head) {
        const u32 l = labels[threadIdx.x - 4];
        if (l) labels[threadIdx.x - 4] = lut[l];
    }
    labels += head;
    n -= head;
    const u64 n4 = n / 4;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (u64)gridDim.x * blockDim.x) {
        uint4 v = reinterpret_cast<uint4*>(labels)[i];
        if (v.x | v.y | v.z | v.w) {
            v.x = v.x ? lut[v.x] : 0u;
            v.y = v.y ? lut[v.y] : 0u;
            v.z = v.z ? lut[v.z] : 0u;
            v.w = v.w ? lut[v.w] : 0u;
            reinterpret_cast<uint4*>(labels)[i] = v;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const u64 i = n4 * 4 + threadIdx.x;
        const u32 l = labels[i];
        if (l) labels[i] = lut[l];
    }
}

// ---- size filter (count_blobs' min_size / max_size; cc3d.dust): keep flags from the voxel count per label (dlv_cc_counts_dev,
// cc_stats.hip), order-preserving renumbering of the kept labels through a lookup table ---------------------------------------
// The lookup table of the size filter is made in three launches over the same n + 1 rows, in this order: size_keep_kernel writes
// the keep flags, the dev_scan_* kernels (dev_scan.h) turn them into their exclusive prefix sum (the number of kept labels below each label),
// size_lut_kernel turns that into the new label.  Both kernels ask size_keeps(), so that they cannot disagree about a label.
__device__ __forceinline__ bool size_keeps(const u32* __restrict__ counts, u64 l, u64 lo, u64 hi) {
    // label 1..n whose voxel count lies in [lo, hi]; label 0 is the background: never kept
    const u64 c = counts[l];
    return l > 0 && c >= lo && c <= hi;
}
__global__ void __launch_bounds__(256) size_keep_kernel(const u32* __restrict__ counts, u64 rows, u64 lo, u64 hi, u32* __restrict__ keep) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (u64)gridDim.x * blockDim.x)
        keep[i] = size_keeps(counts, i, lo, hi) ? 1u : 0u;
}
// lut[l] holds the exclusive scan of the flags: a kept label becomes that + 1, the others 0
__global__ void __launch_bounds__(256) size_lut_kernel(const u32* __restrict__ counts, u64 rows, u64 lo, u64 hi, u32* __restrict__ lut) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (u64)gridDim.x * blockDim.x)
        lut[i] = size_keeps(counts, i, lo, hi) ? lut[i] + 1u : 0u;
}

// The scratch of a labelling of n voxels (slot WS_CCL): root counts per renumbering block, their group sums, the two bit masks
// (foreground, roots), the chunk list - 0.5 B per voxel.  The union-find's parent array IS the label volume
// (ccl_assign_roots_kernel)
struct CclWs {
    u32 *counts, *gsum, *list_n, *list;
    unsigned short *bm, *rb;  // bit mask of the volume (ccl_init_kernel), root bits (written for every chunk by ccl_assign_roots_kernel)
    u64 nb, nch;
};
int ccl_ws_get(dlv_ctx* ctx, u64 n, CclWs& w) {
    w.nb = (n + RCHUNK - 1) / RCHUNK;
    w.nch = (n + 15) / 16;
    char* ws;
    WsCarve c;
    const size_t counts_off = c.take((size_t)(w.nb + 1) * 4), gsum_off = c.take((size_t)(scan_groups(w.nb) + 1) * 4);
    const size_t bm_off = c.take((size_t)(w.nch + 4) * 2), rb_off = c.take((size_t)(w.nch + 4) * 2);
    const size_t list_n_off = c.take(256), list_off = c.take((size_t)w.nch * 4 + 256);  // [list_n, pad, list[nch]]
    DLV_TRY(dlv_ws_get(ctx, WS_CCL, c.end, (void**)&ws));
    w.list_n = (u32*)(ws + list_n_off);
    w.list = (u32*)(ws + list_off);
    w.rb = (unsigned short*)(ws + rb_off);
    w.counts = (u32*)(ws + counts_off);
    w.gsum = (u32*)(ws + gsum_off);
    w.bm = (unsigned short*)(ws + bm_off);
    return DLV_OK;
}

// The roots of the forest in `labels` (an entry that holds its own index, among the voxels of w.bm) get the labels 1..N in raster
// order, w.rb records which entries they are, w.counts[w.nb] receives N: the renumbering of dlv_ccl26_dev, and of
// dlv_ccl_number_forest.  The other entries still hold their root's index when this returns.
int ccl_number_roots(dlv_ctx* ctx, const CclWs& w, u32* labels, u64 n) {
    hipLaunchKernelGGL(ccl_count_roots_kernel, dim3((unsigned)w.nb), dim3(256), 0, ctx->stream, w.bm, labels, n, w.counts);
    DLV_LAUNCH_CHECK(ctx, "ccl_count_roots_kernel");
    DLV_TRY(dev_excl_scan(ctx, w.counts, w.nb, w.counts, w.gsum, w.counts + w.nb, "ccl_scan_counts_kernel"));
    hipLaunchKernelGGL(ccl_assign_roots_kernel, dim3((unsigned)w.nb), dim3(256), 0, ctx->stream, w.bm, labels, n, w.counts, labels, w.rb);
    DLV_LAUNCH_CHECK(ctx, "ccl_assign_roots_kernel");
    return DLV_OK;
}

// every voxel of the volume is written: 0 for the background, the root's label for the rest.  ran (may be null): receives the
// kernel launched, in the numbering of dlv_ccl_ran.relabel
int ccl_relabel_whole(dlv_ctx* ctx, const CclWs& w, u32* labels, u64 n, bool aligned, int* ran = nullptr) {
    if (ran) *ran = aligned ? 1 : 2;  // (lines : chunks - the two launches below)
    if (aligned)
        hipLaunchKernelGGL(ccl_relabel_lines_kernel, dim3((unsigned)std::min<u64>((n / 1024 + 3) / 4 + 1, (u64)256 * 32)), dim3(256), 0,
                           ctx->stream, w.bm, w.rb, n, labels);
    else
        hipLaunchKernelGGL(ccl_relabel_kernel, dim3((unsigned)std::min<u64>((w.nch + 255) / 256, (u64)256 * 64)), dim3(256), 0, ctx->stream,
                           w.bm, w.rb, n, labels, aligned);
    DLV_LAUNCH_CHECK(ctx, "ccl_relabel_kernel");
    return DLV_OK;
}

}  // namespace

// common.h: the renumbering half of dlv_ccl26_dev for a forest that somebody else has built
int dlv_ccl_number_forest(dlv_ctx* ctx, const uint32_t* fg_dev, uint32_t* forest_dev, uint64_t n, uint64_t* n_out) {
    if (!ctx || !fg_dev || !forest_dev || !n_out || n == 0) return DLV_EINVAL;
    if (n > ((u64)1 << 32)) return dlv_fail(ctx, DLV_EUNSUP, "volumes above 2^32 voxels need 64-bit labels");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    CclWs w;
    DLV_TRY(ccl_ws_get(ctx, n, w));
    const int gs = (int)std::min<u64>((w.nch + 255) / 256, (u64)256 * 64);
    hipLaunchKernelGGL(ccl_bits_of_labels_kernel, dim3(gs), dim3(256), 0, ctx->stream, fg_dev, (u64)n, w.bm);
    DLV_LAUNCH_CHECK(ctx, "ccl_bits_of_labels_kernel");
    DLV_TRY(ccl_number_roots(ctx, w, forest_dev, n));
    DLV_TRY(ccl_relabel_whole(ctx, w, forest_dev, n, (reinterpret_cast<uintptr_t>(forest_dev) & 15) == 0));
    u32 total = 0;
    DLV_HIP(ctx, hipMemcpyAsync(&total, w.counts + w.nb, 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = total;
    return DLV_OK;
}

extern "C" {

int dlv_ccl26_dev(dlv_ctx* ctx, const uint8_t* mask_dev, int Z, int Y, int X, uint32_t* labels_dev, uint64_t* n_out) {
    if (!ctx || !mask_dev || !labels_dev || !n_out) return DLV_EINVAL;
    if (Z <= 0 || Y <= 0 || X <= 0) return dlv_fail(ctx, DLV_EINVAL, "empty volume");
    const u64 n = (u64)Z * Y * X;
    if (n > ((u64)1 << 32)) return dlv_fail(ctx, DLV_EUNSUP, "volumes above 2^32 voxels need 64-bit labels");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    CclWs w;
    DLV_TRY(ccl_ws_get(ctx, n, w));
    u32* L = labels_dev;
    int gs = (int)std::min<u64>((w.nch + 255) / 256, (u64)256 * 64);
    if (ctx->ccl_init_grid > 0) gs = std::min(gs, ctx->ccl_init_grid);  // (dlv_diag_set "ccl_init_grid": tests of the mid-loop flush)
    // 16-byte accesses need the mask 16-byte and the labels 16-byte aligned (hipMalloc / torch allocations are)
    const bool aligned = ((reinterpret_cast<uintptr_t>(mask_dev) | reinterpret_cast<uintptr_t>(labels_dev)) & 15) == 0;
    // bytes: the byte mask is read once (1 B), its bit mask written once and scanned by five kernels (6/8 B), the labels are
    // written once (4 B)
    DlvProf pr(ctx, "ccl26", 0.0, (double)n * (1 + 0.75 + 4));
    const bool simple = ctx->ccl_simple;  // A/B (dlv_diag_set): whole-volume relabel stores instead of memset + list
    DLV_HIP(ctx, hipMemsetAsync(w.list_n, 0, 4, ctx->stream));
    if (!simple) DLV_HIP(ctx, hipMemsetAsync(labels_dev, 0, (size_t)n * 4, ctx->stream));
    hipLaunchKernelGGL(ccl_init_kernel, dim3(gs), dim3(256), 0, ctx->stream, mask_dev, L, n, aligned, w.bm, w.list, w.list_n);
    DLV_LAUNCH_CHECK(ctx, "ccl_init_kernel");
    dlv_ccl_ran& ran = ctx->ccl_ran;  // what this call launches (dlv_diag_ccl_ran): written at the launch sites
    ran = dlv_ccl_ran();
    ran.aligned = aligned ? 1 : 0;
    ran.init_grid = gs;
    ran.init_per = ccl_init_per(w.nch, (u64)gs);
    ran.blocks = w.nb;
    ran.groups = scan_groups(w.nb);
    const int gl = 256 * 16;  // list kernels: grid-stride over the device-side count
    ran.merge_rows = (aligned && X % 16 == 0) ? 1 : 0;
    if (ran.merge_rows)
        hipLaunchKernelGGL(ccl_merge_list_kernel<true>, dim3(gl), dim3(256), 0, ctx->stream, w.bm, L, Y, X, w.list, w.list_n);
    else
        hipLaunchKernelGGL(ccl_merge_list_kernel<false>, dim3(gl), dim3(256), 0, ctx->stream, w.bm, L, Y, X, w.list, w.list_n);
    DLV_LAUNCH_CHECK(ctx, "ccl_merge_kernel");
    hipLaunchKernelGGL(ccl_compress_kernel, dim3(gl), dim3(256), 0, ctx->stream, w.bm, L, w.list, w.list_n);
    DLV_LAUNCH_CHECK(ctx, "ccl_compress_kernel");
    DLV_TRY(ccl_number_roots(ctx, w, labels_dev, n));
    if (!simple) {
        ran.relabel = 0;
        hipLaunchKernelGGL(ccl_relabel_list_kernel, dim3(gl), dim3(256), 0, ctx->stream, w.bm, w.rb, n, labels_dev, w.list, w.list_n, aligned);
    } else {
        DLV_TRY(ccl_relabel_whole(ctx, w, labels_dev, n, aligned, &ran.relabel));
    }
    DLV_LAUNCH_CHECK(ctx, "ccl_relabel_kernel");
    pr.end();
    u32 total = 0, listed = 0;
    DLV_HIP(ctx, hipMemcpyAsync(&total, w.counts + w.nb, 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(&listed, w.list_n, 4, hipMemcpyDeviceToHost, ctx->stream));  // (the launch record's list_n)
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ran.list_n = listed;
    *n_out = total;
    return DLV_OK;
}

int dlv_seam_pairs_dev(dlv_ctx* ctx, const uint32_t* plane_a_dev, const uint32_t* plane_b_dev, int Y, int X,
                       uint32_t* pairs_dev, uint64_t cap, uint64_t* count_out) {
    if (!ctx || !plane_a_dev || !plane_b_dev || !count_out) return DLV_EINVAL;
    if (Y <= 0 || X <= 0) return dlv_fail(ctx, DLV_EINVAL, "empty plane");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    u64* cnt;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, 8, (void**)&cnt));
    DLV_HIP(ctx, hipMemsetAsync(cnt, 0, 8, ctx->stream));
    const u64 n = (u64)Y * X;
    hipLaunchKernelGGL(seam_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, plane_a_dev,
                       plane_b_dev, Y, X, pairs_dev, pairs_dev ? cap : 0, cnt);
    DLV_LAUNCH_CHECK(ctx, "seam_pairs_kernel");
    DLV_HIP(ctx, hipMemcpyAsync(count_out, cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DLV_OK;
}

int dlv_relabel_u32_dev(dlv_ctx* ctx, uint32_t* labels_dev, uint64_t nvox, const uint32_t* lut_dev, uint64_t lut_len) {
    if (!ctx || !labels_dev || !lut_dev) return DLV_EINVAL;
    if (lut_len == 0) return dlv_fail(ctx, DLV_EINVAL, "empty lookup table");
    if (nvox == 0) return DLV_OK;
    if ((uintptr_t)labels_dev & 15) return dlv_fail(ctx, DLV_EINVAL, "labels must be 16-byte aligned");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const int gs = (int)std::min<u64>((nvox / 4 + 255) / 256 + 1, (u64)256 * 32);
    hipLaunchKernelGGL(relabel_lut_kernel, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, (u64)nvox, lut_dev, 0u);
    DLV_LAUNCH_CHECK(ctx, "relabel_lut_kernel");
    return DLV_OK;
}

int dlv_cc_size_filter_dev(dlv_ctx* ctx, uint32_t* labels_dev, uint64_t nvox, uint64_t n, const uint32_t* counts_dev,
                           int64_t min_size, int64_t max_size, uint64_t* n_kept_out) {
    if (!ctx || !labels_dev || !counts_dev || !n_kept_out) return DLV_EINVAL;
    if (min_size >= 0 && max_size >= 0 && min_size > max_size)
        return dlv_fail(ctx, DLV_EINVAL, "size filter: min_size %lld > max_size %lld", (long long)min_size, (long long)max_size);
    DLV_TRY(check_label_count(ctx, "size filter", n));
    if ((uintptr_t)labels_dev & 3) return dlv_fail(ctx, DLV_EINVAL, "labels must be 4-byte aligned");
    *n_kept_out = n;
    if (min_size < 0 && max_size < 0) return DLV_OK;  // no bound: nothing to do
    if (n == 0 || nvox == 0) return DLV_OK;           // no component: nothing to remove
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const u64 lo = min_size < 0 ? 0ull : (u64)min_size, hi = max_size < 0 ? ~0ull : (u64)max_size;
    const u64 rows = n + 1;
    // scratch: the lookup table (n + 1 labels), the sums of its 1024-label groups, the number of kept labels
    WsCarve c;
    const size_t lut_off = c.take((size_t)rows * 4), gsum_off = c.take((size_t)(scan_groups(rows) + 1) * 4), total_off = c.take(256);
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, c.end, (void**)&ws));
    u32* lut = (u32*)(ws + lut_off);
    u32* gsum = (u32*)(ws + gsum_off);
    u32* total = (u32*)(ws + total_off);
    // bytes: the volume is read and (where it holds foreground) written back; the table lookups stay in the caches
    DlvProf pr(ctx, "cc_size_filter", 0.0, (double)nvox * 8 + (double)rows * 20);
    const int gr = (int)std::min<u64>((rows + 255) / 256, (u64)256 * 32);
    hipLaunchKernelGGL(size_keep_kernel, dim3(gr), dim3(256), 0, ctx->stream, counts_dev, rows, lo, hi, lut);
    DLV_LAUNCH_CHECK(ctx, "size_keep_kernel");
    DLV_TRY(dev_excl_scan(ctx, lut, rows, lut, gsum, total, "ccl_scan_counts_kernel"));  // (in place, any number of labels)
    hipLaunchKernelGGL(size_lut_kernel, dim3(gr), dim3(256), 0, ctx->stream, counts_dev, rows, lo, hi, lut);
    DLV_LAUNCH_CHECK(ctx, "size_lut_kernel");
    const u32 head = (u32)std::min<u64>(((16 - ((uintptr_t)labels_dev & 15)) & 15) / 4, nvox);
    const int gs = (int)std::min<u64>((nvox / 4 + 255) / 256 + 1, (u64)256 * 32);
    hipLaunchKernelGGL(relabel_lut_kernel, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, (u64)nvox, lut, head);
    DLV_LAUNCH_CHECK(ctx, "relabel_lut_kernel");
    pr.end();
    u32 kept = 0;
    DLV_HIP(ctx, hipMemcpyAsync(&kept, total, 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_kept_out = kept;
    return DLV_OK;
}

}  // extern "C"
