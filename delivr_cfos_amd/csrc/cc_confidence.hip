// cc_confidence.hip - per-label statistics of the network's probability volume under a label volume (dlv_cc_confidence_dev):
// sum, minimum and maximum of every component's probabilities and the position of its peak.  The reference has no counterpart
// (its users take them on the host from the label file and network_output.npy); the labels are in HBM at the end of
// count_blobs' labelling and the probabilities are one upload away, so this is one streaming pass over 4 + 4 bytes per voxel.
//
// Fixed point: a probability p becomes q(p) = rint(clamp(p, 0, 1) * 2^24), NaN counting as 0 - the product is exact in float32,
// rint rounds half to even, and above 0.5 (every voxel of a cell at the default threshold) q loses nothing.  Everything after
// that is integer work (u64 sums, u32 minima, u64 keyed maxima): results are exact and independent of scheduling.  No
// overflow: a component has at most 2^32 - 1 voxels and q <= 2^24, so its sum stays below 2^56.
// The peak - the voxel of largest q, the first in C-raster order on a tie - and the maximum are ONE u64 maximum of the key
// (q << 39) | (2^39 - 1 - index): the larger q wins, then the smaller index.  A volume of fewer than 2^39 voxels keeps the
// index inside its 39 bits and the key of every voxel above 0, the value of a label without a voxel.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int INDEX_BITS = 39;
constexpr u64 INDEX_MASK = (1ull << INDEX_BITS) - 1;

__device__ __forceinline__ u32 quantise(float p) {
    float c = p > 0.0f ? p : 0.0f;  // (NaN fails the comparison: 0)
    c = c < 1.0f ? c : 1.0f;
    return (u32)rintf(c * 16777216.0f);
}

// a (thread's, then a wave's) probabilities under one label
struct ConfidenceAcc {
    u64 s;   // (<= 512 * 2^24 per wave)
    u32 mn;
    u64 key;
    static __device__ __forceinline__ ConfidenceAcc none() { return {0ull, NO_VOXEL, 0ull}; }
    __device__ __forceinline__ void combine(int o) {
        xor_add(s, o);
        xor_min(mn, o);
        xor_max(key, o);
    }
};

// The sweep layout and the aggregation of cc_fold.h over the rows of the labels and of the probabilities, both unpadded: 16-byte
// nontemporal loads of each, decided per row.  A wave whose 512 voxels hold no label 1..n skips its probability loads and the
// fold.  A thread folds the voxels of equal label among its 8; the leader lane of a (wave, label) issues three atomics.
// Background (0) and labels above n are not accumulated.
__global__ void __launch_bounds__(256) cc_confidence_kernel(const u32* __restrict__ labels, const float* __restrict__ prob,
                                                            int Z, int Y, int X, u32 n, u64* __restrict__ sum,
                                                            u32* __restrict__ vmin, u64* __restrict__ peak) {
    const u64 nrows = (u64)Z * Y;
    const int sweeps = row_sweeps(X);
    for (u64 row = blockIdx.x; row < nrows; row += gridDim.x) {
        const u64 row0 = row * (u64)X;  // the linear index of the row's first voxel
        const u32* lrow = labels + row0;
        const float* prow = prob + row0;
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2], l[VPT];
            float p[VPT];
            quad_starts(sw, xq);
            load_quads<true>(lrow, true, xq, (u32)X, l);
            unsigned todo = fg_mask(l, n);    // the voxels that are not folded yet
            if (!__any(todo != 0)) continue;  // (wave-uniform) nothing to measure in this wave's 512 voxels
            load_float_quads<true>(prow, xq, (u32)X, p);
            // one pass per distinct label of the thread (one, as a rule)
            while (__any(todo != 0)) {
                const bool have = todo != 0;
                const u32 lab = first_label(l, todo);
                ConfidenceAcc own = ConfidenceAcc::none();
#pragma unroll
                for (int k = 0; k < VPT; ++k) {
                    const bool in = ((todo >> k) & 1u) && l[k] == lab;
                    const u32 q = quantise(p[k]);
                    const u64 key = ((u64)q << INDEX_BITS) | (INDEX_MASK - (row0 + voxel_x(xq, k)));
                    own.s += in ? q : 0u;
                    own.mn = min(own.mn, in ? q : NO_VOXEL);
                    own.key = max(own.key, in ? key : 0ull);
                    todo &= ~((in ? 1u : 0u) << k);
                }
                wave_fold_by_label<true>(lab, have, own, [&](u32 L, const ConfidenceAcc& w) {
                    atomicAdd(sum + L, w.s);
                    atomicMin(vmin + L, w.mn);
                    atomicMax(peak + L, w.key);
                });
            }
        }
    }
}

}  // namespace

extern "C" int dlv_cc_confidence_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const float* prob_dev, int Z, int Y, int X, uint64_t n,
                                     uint64_t* sum_q, uint32_t* min_q, uint32_t* max_q, uint64_t* peak_index) {
    if (!ctx || !labels_dev || !prob_dev || !sum_q || !min_q || !max_q || !peak_index) return DLV_EINVAL;
    DLV_TRY(check_volume(ctx, "cc_confidence", Z, Y, X));
    if ((u64)Z * Y > INDEX_MASK / (u64)X)  // (Z * Y fits 62 bits; the product of all three could wrap)
        return dlv_fail(ctx, DLV_EINVAL, "cc_confidence: a volume of %d x %d x %d voxels: the peak's index has %d bits", Z, Y, X, INDEX_BITS);
    const u64 nvox = (u64)Z * Y * X;
    DLV_TRY(check_label_count(ctx, "cc_confidence", n));
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)prob_dev & 3))
        return dlv_fail(ctx, DLV_EINVAL, "cc_confidence: labels and probabilities must be 4-byte aligned");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rows = (size_t)n + 1;
    // device accumulators: [sum u64 rows | key u64 rows | min u32 rows]; an absent label keeps 0, 0, ~0
    const size_t off_key = rows * 8, off_min = rows * 16, bytes = rows * 20;
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, bytes, (void**)&ws));
    DLV_HIP(ctx, hipMemsetAsync(ws, 0, bytes, ctx->stream));
    DLV_HIP(ctx, hipMemsetAsync(ws + off_min, 0xff, rows * 4, ctx->stream));
    const int gs = (int)std::min<u64>((u64)Z * Y, (u64)256 * 32);
    DlvProf pr(ctx, "cc_confidence", 0.0, (double)nvox * 8);
    hipLaunchKernelGGL(cc_confidence_kernel, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, prob_dev, Z, Y, X, (u32)n, (u64*)ws,
                       (u32*)(ws + off_min), (u64*)(ws + off_key));
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_confidence_kernel");
    std::vector<u64> keys(rows);
    DLV_HIP(ctx, hipMemcpyAsync(sum_q, ws, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(keys.data(), ws + off_key, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(min_q, ws + off_min, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t l = 0; l < rows; ++l) {  // (key 0: no voxel)
        max_q[l] = (uint32_t)(keys[l] >> INDEX_BITS);
        peak_index[l] = keys[l] ? INDEX_MASK - (keys[l] & INDEX_MASK) : ~0ull;
    }
    return DLV_OK;
}
