// cc_stats.hip - per-label statistics of a label volume on the device: voxel count, coordinate sums and bounding box
// (dlv_cc_stats_dev, dlv_cc_stats_raw_dev), and the voxel count alone for the size filter (dlv_cc_counts_dev).
// Replaces cc3d.statistics(..., no_slice_conversion=True) (count_blobs.py:85) on the labels of dlv_ccl26_dev (ccl.hip).
// Integer work only: results are bit-exact and independent of scheduling.  Both kernels aggregate as cc_fold.h describes.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"

#include <algorithm>

namespace {

// ---- statistics: per label count, sum z/y/x (u64), bbox min/max (u32): ten atomics per (wave, label).  Background (label 0)
// is not accumulated here: its row is derived from the totals on the host, its bounding box by a per-wave reduction.
struct StatsAcc {
    u32 c;
    u64 vz, vy, vx;
    u32 z0, z1, y0, y1, x0, x1;
    static __device__ __forceinline__ StatsAcc none() { return {0u, 0ull, 0ull, 0ull, NO_VOXEL, 0u, NO_VOXEL, 0u, NO_VOXEL, 0u}; }
    __device__ __forceinline__ void combine(int o) {
        xor_add(c, o); xor_add(vz, o); xor_add(vy, o); xor_add(vx, o);
        xor_min(z0, o); xor_min(y0, o); xor_min(x0, o);
        xor_max(z1, o); xor_max(y1, o); xor_max(x1, o);
    }
};

__global__ void __launch_bounds__(256) cc_stats_kernel(const u32* __restrict__ labels, int Z, int Y, int X,
                                                       u32* __restrict__ counts, u64* __restrict__ sums,
                                                       u32* __restrict__ bbmin, u32* __restrict__ bbmax) {
    // a workgroup walks whole rows (z, y) in sweeps (cc_fold.h), with its own load scheme: 16-byte loads are decided once per
    // volume (X % 8 == 0 and an aligned volume: every row and every quad is whole), and elsewhere a thread takes 8 consecutive
    // voxels.  The trip counts are workgroup-uniform so that the shuffles below are convergent
    const int segs = (X + VPT - 1) / VPT;
    const int lane = threadIdx.x & 63;
    u32 bmin[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, bmax[3] = {0, 0, 0};
    bool any_bg = false;
    const bool vec = (X % VPT == 0) && ((reinterpret_cast<uintptr_t>(labels) & 15) == 0);
    const u64 nrows = (u64)Z * Y;
    const int sweeps = (segs + (int)blockDim.x - 1) / (int)blockDim.x;
    for (u64 row = blockIdx.x; row < nrows; row += gridDim.x)
    for (int sw = 0; sw < sweeps; ++sw) {
        const int sg = sw * (int)blockDim.x + (int)threadIdx.x;
        u32 l[VPT];
        const u32 z = (u32)(row / (u64)Y), y = (u32)(row % (u64)Y);
        // position of l[k]: x0 + k (+ gap for k >= 4).  Aligned rows: the two quads of the sweep layout; else gap = 0
        const u32 x0 = vec ? (u32)sw * blockDim.x * VPT + 4u * threadIdx.x : (u32)sg * VPT;
        const u32 gap = vec ? 4u * blockDim.x - 4u : 0u;
        if (vec) {
            const u64 base = row * (u64)X + x0;
            u32x4_t u0 = {NO_VOXEL, NO_VOXEL, NO_VOXEL, NO_VOXEL}, u1 = u0;
            if (x0 < (u32)X) u0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(labels + base));
            if (x0 + 4u + gap < (u32)X) u1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(labels + base + 4 + gap));
            l[0] = u0.x; l[1] = u0.y; l[2] = u0.z; l[3] = u0.w;
            l[4] = u1.x; l[5] = u1.y; l[6] = u1.z; l[7] = u1.w;
        } else if (sg < segs) {
            const u64 base = row * (u64)X + x0;
#pragma unroll
            for (int k = 0; k < VPT; ++k) l[k] = (x0 + k < (u32)X) ? labels[base + k] : NO_VOXEL;
        } else {
#pragma unroll
            for (int k = 0; k < VPT; ++k) l[k] = NO_VOXEL;
        }
        auto xpos = [&](int k) -> u32 { return x0 + (u32)k + (k >= 4 ? gap : 0u); };
        // background bookkeeping: the thread's zero voxels as a bit mask, first / last of them along x
        unsigned zm = 0, fgm = 0;
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            zm |= (l[k] == 0 ? 1u : 0u) << k;
            fgm |= ((l[k] != 0 && l[k] != NO_VOXEL) ? 1u : 0u) << k;
        }
        if (zm) {
            any_bg = true;
            bmin[0] = min(bmin[0], z); bmax[0] = max(bmax[0], z);
            bmin[1] = min(bmin[1], y); bmax[1] = max(bmax[1], y);
            bmin[2] = min(bmin[2], xpos(__ffs((int)zm) - 1)); bmax[2] = max(bmax[2], xpos(31 - __clz((int)zm)));
        }
        if (!__any(fgm != 0)) continue;  // (wave-uniform) nothing but background in this wave's 512 voxels
        // runs of equal foreground labels inside the thread's voxels, one run per pass of the loop below
        int k = 0;
        while (true) {
            // next run of this lane (if any)
            while (k < VPT && (l[k] == 0 || l[k] == NO_VOXEL)) ++k;
            const bool have = k < VPT;
            if (!__any(have)) break;
            u32 lab = 0, cnt = 0, sx = 0, mnx = NO_VOXEL, mxx = 0;
            if (have) {
                lab = l[k];
                while (k < VPT && l[k] == lab) {
                    ++cnt;
                    sx += xpos(k);
                    mnx = min(mnx, xpos(k));
                    mxx = max(mxx, xpos(k));
                    ++k;
                }
            }
            const StatsAcc own = {cnt, (u64)z * cnt, (u64)y * cnt, (u64)sx, z, z, y, y, mnx, mxx};  // (z and y are the row's)
            wave_fold_by_label<false>(lab, have, own, [&](u32 L, const StatsAcc& w) {
                atomicAdd(counts + L, w.c);
                atomicAdd(sums + 3 * (u64)L, w.vz);
                atomicAdd(sums + 3 * (u64)L + 1, w.vy);
                atomicAdd(sums + 3 * (u64)L + 2, w.vx);
                atomicMin(bbmin + 3 * (u64)L, w.z0); atomicMax(bbmax + 3 * (u64)L, w.z1);
                atomicMin(bbmin + 3 * (u64)L + 1, w.y0); atomicMax(bbmax + 3 * (u64)L + 1, w.y1);
                atomicMin(bbmin + 3 * (u64)L + 2, w.x0); atomicMax(bbmax + 3 * (u64)L + 2, w.x1);
            });
        }
    }
    if (__any(any_bg)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u32 lo = bmin[k], hi = bmax[k];
            for (int o = 32; o > 0; o >>= 1) xor_min(lo, o), xor_max(hi, o);
            if (lane == 0) {
                atomicMin(bbmin + k, lo);
                atomicMax(bbmax + k, hi);
            }
        }
    }
}

// ---- voxel counts (the size filter's input, ccl.hip) ----------------------------------------------------------------
// cc_stats_kernel's aggregation with ONE atomic per (wave, label) instead of ten.  The volume is walked as a flat array in
// tiles of 2048 voxels (a thread takes voxels [4t, 4t+4) and [1024 + 4t, 1024 + 4t + 4) of the tile: every 16-byte load
// instruction of a wave covers one contiguous KiB); the last partial tile, and every tile of a volume that does not start on a
// 16-byte boundary, is read label by label.  Labels above n are not counted (the table has n + 1 rows).
constexpr int CTILE = 256 * VPT;  // voxels per workgroup and sweep

struct CountAcc {
    u32 c;
    static __device__ __forceinline__ CountAcc none() { return {0u}; }
    __device__ __forceinline__ void combine(int o) { xor_add(c, o); }
};

__device__ __forceinline__ void cc_counts_fold(const u32 (&l)[VPT], u32 n, u32* __restrict__ counts, u32& nbg) {
    // bit k of chg: voxel k starts a run (differs from the voxel before it)
    unsigned chg = 1u | (1u << VPT);
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        nbg += l[k] == 0 ? 1u : 0u;
        if (k > 0) chg |= (l[k] != l[k - 1] ? 1u : 0u) << k;
    }
    unsigned starts = fg_mask(l, n) & chg;  // first voxels of this thread's foreground runs
    if (!__any(starts != 0)) return;        // (wave-uniform) nothing but background in this wave's 512 voxels
    while (true) {
        const bool have = starts != 0;
        if (!__any(have)) break;
        u32 lab = 0;
        CountAcc own = CountAcc::none();
        if (have) {
            const int k0 = __ffs((int)starts) - 1;
            lab = first_label(l, starts);
            starts &= starts - 1;
            own.c = (u32)(__ffs((int)(chg >> (k0 + 1))) - 1) + 1u;  // up to the next run's start (bit VPT ends the last one)
        }
        wave_fold_by_label<false>(lab, have, own, [&](u32 L, const CountAcc& w) { atomicAdd(counts + L, w.c); });
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) cc_counts_kernel(const u32* __restrict__ labels, u64 nvox, u32 n, u32* __restrict__ counts) {
    const u64 ntiles = nvox / CTILE;
    u32 nbg = 0;
    u32 l[VPT];
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (workgroup-uniform trip count: the shuffles are convergent)
        const u64 base = tile * CTILE + 4u * threadIdx.x;
        if (VEC) {
            const u32x4_t u0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(labels + base));
            const u32x4_t u1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(labels + base + CTILE / 2));
            l[0] = u0.x; l[1] = u0.y; l[2] = u0.z; l[3] = u0.w;
            l[4] = u1.x; l[5] = u1.y; l[6] = u1.z; l[7] = u1.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                l[k] = labels[base + k];
                l[4 + k] = labels[base + CTILE / 2 + k];
            }
        }
        cc_counts_fold(l, n, counts, nbg);
    }
    if (blockIdx.x == gridDim.x - 1 && ntiles * CTILE < nvox) {  // the last partial tile
        const u64 base = ntiles * CTILE + (u64)threadIdx.x * VPT;
#pragma unroll
        for (int k = 0; k < VPT; ++k) l[k] = base + k < nvox ? labels[base + k] : NO_VOXEL;
        cc_counts_fold(l, n, counts, nbg);
    }
    for (int o = 32; o > 0; o >>= 1) xor_add(nbg, o);
    if ((threadIdx.x & 63) == 0 && nbg) atomicAdd(counts, nbg);
}

// shared by dlv_cc_stats_dev / dlv_cc_stats_raw_dev: raw per-label accumulators copied to the host
struct StatsRaw {
    std::vector<char> host;
    size_t off_min, off_max, off_sum, rows;
    const u32* counts() const { return (const u32*)host.data(); }
    const u32* bbmin() const { return (const u32*)(host.data() + off_min); }
    const u32* bbmax() const { return (const u32*)(host.data() + off_max); }
    const u64* sums() const { return (const u64*)(host.data() + off_sum); }
};

int cc_stats_raw(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, StatsRaw& r) {
    if (Z <= 0 || Y <= 0 || X <= 0) return dlv_fail(ctx, DLV_EINVAL, "empty volume");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nvox = (u64)Z * Y * X;
    const size_t rows = (size_t)n + 1;
    // [counts u32 rows | bbmin u32 3*rows | bbmax u32 3*rows | pad | sums u64 3*rows]
    r.rows = rows;
    r.off_min = rows * 4;
    r.off_max = r.off_min + rows * 12;
    r.off_sum = (r.off_max + rows * 12 + 7) & ~(size_t)7;
    const size_t bytes = r.off_sum + rows * 24;
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, bytes, (void**)&ws));
    DLV_HIP(ctx, hipMemsetAsync(ws, 0, bytes, ctx->stream));
    DLV_HIP(ctx, hipMemsetAsync(ws + r.off_min, 0xff, rows * 12, ctx->stream));
    u32* counts = (u32*)ws;
    u32* bbmin = (u32*)(ws + r.off_min);
    u32* bbmax = (u32*)(ws + r.off_max);
    u64* sums = (u64*)(ws + r.off_sum);
    const u64 nitems = (u64)Z * Y * ((X + VPT - 1) / VPT);
    const int gs = (int)std::min<u64>((nitems + 255) / 256, (u64)256 * 32);
    DlvProf pr(ctx, "cc_stats", 0.0, (double)nvox * 4);
    hipLaunchKernelGGL(cc_stats_kernel, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, Z, Y, X, counts, sums, bbmin, bbmax);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_stats_kernel");
    r.host.resize(bytes);
    DLV_HIP(ctx, hipMemcpyAsync(r.host.data(), ws, bytes, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DLV_OK;
}

}  // namespace

extern "C" {

int dlv_cc_stats_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, uint32_t* voxel_counts,
                     uint16_t* bounding_boxes, double* centroids) {
    if (!ctx || !labels_dev || !voxel_counts || !bounding_boxes || !centroids) return DLV_EINVAL;
    if (Z > 65536 || Y > 65536 || X > 65536) return dlv_fail(ctx, DLV_EUNSUP, "bounding boxes are uint16");
    StatsRaw r;
    DLV_TRY(cc_stats_raw(ctx, labels_dev, Z, Y, X, n, r));
    const u64 nvox = (u64)Z * Y * X;
    const size_t rows = r.rows;
    const u32 *hc = r.counts(), *hmin = r.bbmin(), *hmax = r.bbmax();
    const u64* hs = r.sums();
    u64 fg = 0, fs[3] = {0, 0, 0};
    for (size_t l = 1; l < rows; ++l) {
        voxel_counts[l] = hc[l];
        fg += hc[l];
        for (int k = 0; k < 3; ++k) {
            fs[k] += hs[3 * l + k];
            bounding_boxes[6 * l + 2 * k] = (uint16_t)hmin[3 * l + k];
            bounding_boxes[6 * l + 2 * k + 1] = (uint16_t)hmax[3 * l + k];
            centroids[3 * l + k] = hc[l] ? (double)hs[3 * l + k] / (double)hc[l] : NAN;
        }
    }
    // background row: totals minus the foreground
    const u64 dims[3] = {(u64)Z, (u64)Y, (u64)X};
    const u64 bgc = nvox - fg;
    voxel_counts[0] = (uint32_t)bgc;
    for (int k = 0; k < 3; ++k) {
        const u64 all = (nvox / dims[k]) * (dims[k] * (dims[k] - 1) / 2);
        centroids[k] = bgc ? (double)(all - fs[k]) / (double)bgc : NAN;
        bounding_boxes[2 * k] = bgc ? (uint16_t)hmin[k] : 0;
        bounding_boxes[2 * k + 1] = bgc ? (uint16_t)hmax[k] : 0;
    }
    return DLV_OK;
}

int dlv_cc_stats_raw_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, uint32_t* counts,
                         uint32_t* bbmin, uint32_t* bbmax, uint64_t* sums) {
    if (!ctx || !labels_dev || !counts || !bbmin || !bbmax || !sums) return DLV_EINVAL;
    StatsRaw r;
    DLV_TRY(cc_stats_raw(ctx, labels_dev, Z, Y, X, n, r));
    memcpy(counts, r.counts(), r.rows * 4);
    memcpy(bbmin, r.bbmin(), r.rows * 12);
    memcpy(bbmax, r.bbmax(), r.rows * 12);
    memcpy(sums, r.sums(), r.rows * 24);
    return DLV_OK;
}

int dlv_cc_counts_dev(dlv_ctx* ctx, const uint32_t* labels_dev, uint64_t nvox, uint64_t n, uint32_t* counts_dev) {
    if (!ctx || !labels_dev || !counts_dev) return DLV_EINVAL;
    DLV_TRY(check_label_count(ctx, "cc_counts", n));
    if ((uintptr_t)labels_dev & 3) return dlv_fail(ctx, DLV_EINVAL, "labels must be 4-byte aligned");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    DLV_HIP(ctx, hipMemsetAsync(counts_dev, 0, ((size_t)n + 1) * 4, ctx->stream));
    if (nvox == 0) return DLV_OK;
    const int gs = (int)std::min<u64>(std::max<u64>(nvox / CTILE, 1), (u64)256 * 32);
    DlvProf pr(ctx, "cc_counts", 0.0, (double)nvox * 4);
    if (((uintptr_t)labels_dev & 15) == 0)
        hipLaunchKernelGGL(cc_counts_kernel<true>, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, (u64)nvox, (u32)n, counts_dev);
    else
        hipLaunchKernelGGL(cc_counts_kernel<false>, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, (u64)nvox, (u32)n, counts_dev);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_counts_kernel");
    return DLV_OK;
}

}  // extern "C"
