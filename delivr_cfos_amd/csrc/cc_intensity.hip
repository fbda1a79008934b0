// cc_intensity.hip - per-label statistics of the raw uint16 volume under a label volume (dlv_cc_intensity_dev): sum, sum of
// squares, minimum and maximum of the raw intensities of every component.  The reference has no counterpart (its users take
// them on the host from the label file and the raw file); the labels are in HBM at the end of count_blobs' labelling and the
// raw volume is the one run_inference uploaded, so this is one streaming pass over 4 + 2 bytes per voxel.
//
// Integer work only (u64 sums, u32 minima / maxima): results are exact and independent of scheduling.  No overflow: a
// component has at most 2^32 - 1 voxels and 65535^2 < 2^32, so the sum of squares stays below 2^64.
#include "common.h"

#include <algorithm>
#include <vector>

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int IPT = 8;  // voxels per thread and sweep: two quads of one row

__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
    const u32 lo = __shfl_xor((u32)v, o, 64), hi = __shfl_xor((u32)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}

// cc_stats_kernel's structure (ccl.hip): a workgroup walks whole rows (z, y) - no per-thread 64-bit division, and the two
// arrays, whose pitches differ (the raw file is padded to window multiples, the labels are not), are addressed from their own
// row starts.  Per sweep of T threads a thread takes voxels [4t, 4t+4) and [4(T+t), 4(T+t)+4) of the sweep's 8T voxels, so that
// each of its vector loads is part of one contiguous run per wave instruction (1 KiB of labels, 512 B of raw).  A row of labels
// that starts on a 16-byte boundary is read with 16-byte loads, a row of raw that starts on an 8-byte boundary with 8-byte
// loads - decided per row and per array: with an odd X or pitch the alignment changes from row to row.  The quad that crosses
// the end of the row, and every quad of a row that is not aligned, is read element by element.
// Contributions are aggregated before they reach memory: a thread folds the voxels of equal label among its 8 (its runs of
// equal labels, also across the gap between the quads), the lanes of a wave that hold the same label are combined with
// shuffles and ONE leader lane issues the four atomics (a brain-sized single component would otherwise serialise on one
// address).  A wave whose 512 voxels hold no label 1..n skips its raw loads and the fold.  Background (0) and labels above n
// are not accumulated; 0xffffffff stands for "no voxel".
__global__ void __launch_bounds__(256) cc_intensity_kernel(const u32* __restrict__ labels, const unsigned short* __restrict__ raw,
                                                           int Z, int Y, int X, long long pitch_y, long long pitch_z, u32 n,
                                                           u64* __restrict__ sum, u64* __restrict__ sumsq,
                                                           u32* __restrict__ vmin, u32* __restrict__ vmax) {
    typedef u32 u32x4_t __attribute__((ext_vector_type(4)));
    typedef u32 u32x2_t __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63;
    const u32 T = blockDim.x;
    const u64 nrows = (u64)Z * Y;
    const int sweeps = (X + (int)T * IPT - 1) / ((int)T * IPT);  // (workgroup-uniform trip counts: the shuffles below are convergent)
    for (u64 row = blockIdx.x; row < nrows; row += gridDim.x) {
        const u32 z = (u32)(row / (u64)Y), y = (u32)(row % (u64)Y);
        const u32* lrow = labels + row * (u64)X;
        const unsigned short* rrow = raw + (u64)z * (u64)pitch_z + (u64)y * (u64)pitch_y;
        const bool lvec = (reinterpret_cast<uintptr_t>(lrow) & 15) == 0;
        const bool rvec = (reinterpret_cast<uintptr_t>(rrow) & 7) == 0;
        for (int sw = 0; sw < sweeps; ++sw) {
            // quad q of this thread starts at xq[q]; voxel k = 4q + j sits at xq[q] + j
            const u32 xq[2] = {(u32)sw * T * IPT + 4u * threadIdx.x, (u32)sw * T * IPT + 4u * (T + threadIdx.x)};
            u32 l[IPT];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (lvec && xq[q] + 4u <= (u32)X) {
                    const u32x4_t u = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(lrow + xq[q]));
                    l[4 * q] = u.x; l[4 * q + 1] = u.y; l[4 * q + 2] = u.z; l[4 * q + 3] = u.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) l[4 * q + j] = (xq[q] + j < (u32)X) ? lrow[xq[q] + j] : 0xffffffffu;
                }
            }
            unsigned todo = 0;  // bit k: voxel k holds a label 1..n that is not folded yet
#pragma unroll
            for (int k = 0; k < IPT; ++k) todo |= ((l[k] != 0 && l[k] <= n) ? 1u : 0u) << k;
            if (!__any(todo != 0)) continue;  // (wave-uniform) nothing to measure in this wave's 512 voxels
            u32 r[IPT];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (rvec && xq[q] + 4u <= (u32)X) {
                    const u32x2_t u = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(rrow + xq[q]));
                    r[4 * q] = u.x & 0xffffu; r[4 * q + 1] = u.x >> 16; r[4 * q + 2] = u.y & 0xffffu; r[4 * q + 3] = u.y >> 16;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) r[4 * q + j] = (xq[q] + j < (u32)X) ? (u32)rrow[xq[q] + j] : 0u;
                }
            }
            // one pass per distinct label of the thread (one, as a rule)
            while (true) {
                const bool have = todo != 0;
                if (!__any(have)) break;
                const int k0 = __ffs((int)todo) - 1;
                u32 lab = 0;
#pragma unroll
                for (int k = 0; k < IPT; ++k) lab = (k == k0) ? l[k] : lab;  // (no dynamic index into the registers)
                u32 s = 0, mn = 0xffffffffu, mx = 0;
                u64 sq = 0;
#pragma unroll
                for (int k = 0; k < IPT; ++k) {
                    const bool in = ((todo >> k) & 1u) && l[k] == lab;
                    const u32 v = in ? r[k] : 0u;
                    s += v;               // (<= 8 * 65535)
                    sq += (u64)(v * v);   // (65535^2 < 2^32)
                    mn = min(mn, in ? r[k] : 0xffffffffu);
                    mx = max(mx, v);
                    todo &= ~((in ? 1u : 0u) << k);
                }
                // lanes holding the same label are combined; one leader per distinct label issues the atomics
                bool pending = have;
                while (true) {
                    const unsigned long long m = __ballot(pending);
                    if (!m) break;
                    const int leader = __ffsll((long long)m) - 1;
                    const u32 L = __shfl(lab, leader, 64);
                    const bool mine = pending && lab == L;
                    u32 ws = mine ? s : 0u;  // (<= 512 * 65535: fits 32 bits)
                    u64 wq = mine ? sq : 0ull;
                    u32 w0 = mine ? mn : 0xffffffffu, w1 = mine ? mx : 0u;
                    // (wave-uniform) a label that one lane alone holds - a cell's one run in this stretch of the row, the common
                    // case of a cell mask - needs no reduction: the leader's own values are the wave's
                    if (__popcll(__ballot(mine)) > 1)
                        for (int o = 32; o > 0; o >>= 1) {
                            ws += __shfl_xor(ws, o, 64);
                            wq += shfl_xor64(wq, o);
                            w0 = min(w0, __shfl_xor(w0, o, 64));
                            w1 = max(w1, __shfl_xor(w1, o, 64));
                        }
                    if (lane == leader) {
                        atomicAdd(sum + L, (u64)ws);
                        atomicAdd(sumsq + L, wq);
                        atomicMin(vmin + L, w0);
                        atomicMax(vmax + L, w1);
                    }
                    pending = pending && !mine;
                }
            }
        }
    }
}

}  // namespace

extern "C" int dlv_cc_intensity_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint16_t* raw_dev, int Z, int Y, int X,
                                    int64_t raw_pitch_y, int64_t raw_pitch_z, uint64_t n, uint64_t* sum, uint64_t* sumsq,
                                    uint16_t* vmin, uint16_t* vmax) {
    if (!ctx || !labels_dev || !raw_dev || !sum || !sumsq || !vmin || !vmax) return DLV_EINVAL;
    if (Z < 1 || Y < 1 || X < 1) return dlv_fail(ctx, DLV_EINVAL, "cc_intensity: empty volume");
    if (raw_pitch_y < X || raw_pitch_z / Y < raw_pitch_y)
        return dlv_fail(ctx, DLV_EINVAL, "cc_intensity: raw pitches (%lld, %lld) do not hold rows of %d and planes of %d rows",
                        (long long)raw_pitch_z, (long long)raw_pitch_y, X, Y);
    if (n >= 0xffffffffull) return dlv_fail(ctx, DLV_EINVAL, "cc_intensity: n = %llu does not fit the uint32 labels", (unsigned long long)n);
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)raw_dev & 1))
        return dlv_fail(ctx, DLV_EINVAL, "cc_intensity: labels must be 4-byte aligned, raw 2-byte aligned");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rows = (size_t)n + 1;
    // device accumulators: [sum u64 rows | sumsq u64 rows | min u32 rows | max u32 rows]; an absent label keeps 0, 0, ~0, 0
    const size_t off_sq = rows * 8, off_min = rows * 16, off_max = rows * 20, bytes = rows * 24;
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, bytes, (void**)&ws));
    DLV_HIP(ctx, hipMemsetAsync(ws, 0, bytes, ctx->stream));
    DLV_HIP(ctx, hipMemsetAsync(ws + off_min, 0xff, rows * 4, ctx->stream));
    const u64 nvox = (u64)Z * Y * X;
    const int gs = (int)std::min<u64>((u64)Z * Y, (u64)256 * 32);
    DlvProf pr(ctx, "cc_intensity", 0.0, (double)nvox * 6);
    hipLaunchKernelGGL(cc_intensity_kernel, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, raw_dev, Z, Y, X, (long long)raw_pitch_y,
                       (long long)raw_pitch_z, (u32)n, (u64*)ws, (u64*)(ws + off_sq), (u32*)(ws + off_min), (u32*)(ws + off_max));
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_intensity_kernel");
    std::vector<u32> host(rows * 2);
    DLV_HIP(ctx, hipMemcpyAsync(sum, ws, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(sumsq, ws + off_sq, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(host.data(), ws + off_min, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t l = 0; l < rows; ++l) {  // (0xffffffff -> 0xFFFF: the "absent" marker survives the narrowing)
        vmin[l] = (uint16_t)host[l];
        vmax[l] = (uint16_t)host[rows + l];
    }
    return DLV_OK;
}
