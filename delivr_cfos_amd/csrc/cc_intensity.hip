// cc_intensity.hip - per-label statistics of the raw uint16 volume under a label volume (dlv_cc_intensity_dev): sum, sum of
// squares, minimum and maximum of the raw intensities of every component.  The reference has no counterpart (its users take
// them on the host from the label file and the raw file); the labels are in HBM at the end of count_blobs' labelling and the
// raw volume is the one run_inference uploaded, so this is one streaming pass over 4 + 2 bytes per voxel.
//
// Integer work only (u64 sums, u32 minima / maxima): results are exact and independent of scheduling.  No overflow: a
// component has at most 2^32 - 1 voxels and 65535^2 < 2^32, so the sum of squares stays below 2^64.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"

#include <algorithm>
#include <vector>

namespace {

// a (thread's, then a wave's) raw values under one label
struct IntensityAcc {
    u32 s;   // (<= 512 * 65535 per wave: fits 32 bits)
    u64 sq;
    u32 mn, mx;
    static __device__ __forceinline__ IntensityAcc none() { return {0u, 0ull, NO_VOXEL, 0u}; }
    __device__ __forceinline__ void combine(int o) {
        xor_add(s, o); xor_add(sq, o);
        xor_min(mn, o); xor_max(mx, o);
    }
};

// The sweep layout and the aggregation of cc_fold.h over the rows of the labels and of the raw volume, whose pitches differ
// (the raw file is padded to window multiples, the labels are not): 16-byte loads of labels and 8-byte loads of raw, each
// decided per row and per array, both nontemporal (one streaming pass).  A wave whose 512 voxels hold no label 1..n skips its
// raw loads and the fold.  A thread folds the voxels of equal label among its 8 (its runs of equal labels, also across the gap
// between the quads); the leader lane of a (wave, label) issues four atomics.  Background (0) and labels above n are not
// accumulated.
__global__ void __launch_bounds__(256) cc_intensity_kernel(const u32* __restrict__ labels, const unsigned short* __restrict__ raw,
                                                           int Z, int Y, int X, long long pitch_y, long long pitch_z, u32 n,
                                                           u64* __restrict__ sum, u64* __restrict__ sumsq,
                                                           u32* __restrict__ vmin, u32* __restrict__ vmax) {
    const u64 nrows = (u64)Z * Y;
    const int sweeps = row_sweeps(X);
    for (u64 row = blockIdx.x; row < nrows; row += gridDim.x) {
        const u32 z = (u32)(row / (u64)Y), y = (u32)(row % (u64)Y);
        const u32* lrow = labels + row * (u64)X;
        const unsigned short* rrow = raw + (u64)z * (u64)pitch_z + (u64)y * (u64)pitch_y;
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2], l[VPT], r[VPT];
            quad_starts(sw, xq);
            load_quads<true>(lrow, true, xq, (u32)X, l);
            unsigned todo = fg_mask(l, n);    // the voxels that are not folded yet
            if (!__any(todo != 0)) continue;  // (wave-uniform) nothing to measure in this wave's 512 voxels
            load_raw_quads<true>(rrow, xq, (u32)X, r);
            // one pass per distinct label of the thread (one, as a rule)
            while (__any(todo != 0)) {
                const bool have = todo != 0;
                const u32 lab = first_label(l, todo);
                IntensityAcc own = IntensityAcc::none();
#pragma unroll
                for (int k = 0; k < VPT; ++k) {
                    const bool in = ((todo >> k) & 1u) && l[k] == lab;
                    const u32 v = in ? r[k] : 0u;
                    own.s += v;               // (<= 8 * 65535)
                    own.sq += (u64)(v * v);   // (65535^2 < 2^32)
                    own.mn = min(own.mn, in ? r[k] : NO_VOXEL);
                    own.mx = max(own.mx, v);
                    todo &= ~((in ? 1u : 0u) << k);
                }
                wave_fold_by_label<true>(lab, have, own, [&](u32 L, const IntensityAcc& w) {
                    atomicAdd(sum + L, (u64)w.s);
                    atomicAdd(sumsq + L, w.sq);
                    atomicMin(vmin + L, w.mn);
                    atomicMax(vmax + L, w.mx);
                });
            }
        }
    }
}

}  // namespace

extern "C" int dlv_cc_intensity_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint16_t* raw_dev, int Z, int Y, int X,
                                    int64_t raw_pitch_y, int64_t raw_pitch_z, uint64_t n, uint64_t* sum, uint64_t* sumsq,
                                    uint16_t* vmin, uint16_t* vmax) {
    if (!ctx || !labels_dev || !raw_dev || !sum || !sumsq || !vmin || !vmax) return DLV_EINVAL;
    DLV_TRY(check_volume(ctx, "cc_intensity", Z, Y, X));
    DLV_TRY(check_raw_pitches(ctx, "cc_intensity", Y, X, raw_pitch_y, raw_pitch_z));
    DLV_TRY(check_label_count(ctx, "cc_intensity", n));
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
