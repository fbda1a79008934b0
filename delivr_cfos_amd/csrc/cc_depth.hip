// cc_depth.hip - the exact label-wise squared Euclidean distance map of a label volume and its per-label summary
// (dlv_cc_depth_dev): for every voxel of a label 1..n the squared distance, in integer spacings (wz, wy, wx), to the nearest voxel
// of another label - the background, a touching cell, a label above n and every position outside the volume alike - and per
// label the largest value, the voxel that holds it and the sum.  sqrt of the largest value is the radius of the largest ball
// inscribed in the cell, and the voxel is a point that always lies inside it.  The reference has no counterpart (its users call
// scipy.ndimage.distance_transform_edt per cell on the host).  paint.hip's dlv_edt_u16_dev is fp64, treats the foreground as one
// object and is sized for the down-sampled depth map: here two touching cells must not see into each other.
//
// Three separable passes, x, y, z.  With G the result of the passes before it, a pass along an axis of spacing w gives
//   G'(v) = min over the positions u of v's line of (w |v - u|)^2 + (G(u) where L(u) == L(v), else 0),
// the outside of the volume counting as positions of another label: after the x pass the squared distance to the nearest other
// label inside the row, after the y pass inside the plane, after the z pass inside the volume (a voxel of another label on the line
// stands for its whole row / plane at distance 0; a voxel of the same label beyond it is farther away than it).
//  x: the run [x0, x1] of a voxel's label in its row gives (wx min(x - x0 + 1, x1 - x + 1))^2: two wave scans per row.
//  y, z: a thread per voxel walks outward in both directions, d = 1, 2, ..., while (w d)^2 is below its best value - neighbouring
//     lanes read neighbouring x, so every step is a coalesced row access - and stops at the first voxel of another label.  The walk
//     is as long as the cell is thick: short on a cell mask, quadratic in the thickness on one solid block, by design.
// Integer work only: exact and independent of scheduling.  No overflow: on entry w_a ceil((dim_a + 1) / 2) < 65536 on every
// axis, a walk or a run reaches the outside of the volume within ceil(dim_a / 2) steps, so every (w d)^2 and every value of the
// map is below 2^32; a candidate G(u) + (w d)^2 is compared as G(u) < best - (w d)^2 and only formed when it is below best.
// The peak - the voxel of largest value, the first in C-raster order on a tie - and the maximum are ONE u64 maximum of the key
// (D2 << 32) | (2^32 - 1 - index), as in cc_confidence.hip; a measured voxel has D2 >= 1, so key 0 is a label without a voxel.
//
// Measured once on an MI355X (profiles/README.md, "cc_depth"): the bench's 1024 x 2048 x 2048 cell mask, 10.7 + 8.1 + 8.3 ms for
// x, y, z beside a copy rate of 4.7 TB/s in the same process; one solid component of 256^3, 0.06 + 2.7 + 4.3 ms.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int ROW_WAVES = 4;  // the waves of a workgroup of the x pass: a row each

__device__ __forceinline__ bool quad_is_vector(const u32* row, u32 x, u32 X) {
    return (reinterpret_cast<uintptr_t>(row) & 15) == 0 && x + 4u <= X;
}
// the four values at [x, x + 4) of a row of the map: one 16-byte access where load_quads takes one, element by element elsewhere
__device__ __forceinline__ void store_quad(u32* row, u32 x, u32 X, const u32 (&v)[4]) {
    if (quad_is_vector(row, x, X)) {
        u32x4_t u = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<u32x4_t*>(row + x) = u;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < X) row[x + j] = v[j];
    }
}
__device__ __forceinline__ void load_quad(const u32* row, u32 x, u32 X, u32 (&v)[4]) {
    if (quad_is_vector(row, x, X)) {
        const u32x4_t u = *reinterpret_cast<const u32x4_t*>(row + x);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (x + j < X) ? row[x + j] : 0u;
    }
}

// inclusive maximum over the lanes up to this one / minimum over the lanes from this one on
__device__ __forceinline__ u32 wave_prefix_max(u32 v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const u32 u = __shfl_up(v, o, 64);
        v = lane >= o ? max(v, u) : v;
    }
    return v;
}
__device__ __forceinline__ u32 wave_suffix_min(u32 v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const u32 u = __shfl_down(v, o, 64);
        v = lane + o < 64 ? min(v, u) : v;
    }
    return v;
}

// The x pass.  A wave takes a row in sweeps of 512 voxels, a lane the quads [4 lane, 4 lane + 4) and 256 voxels further on (the
// quad loads of cc_fold.h).  Forward over the row: a voxel whose left neighbour holds another label (or is the row's start)
// starts a run; the start of every voxel's run is a prefix maximum of those positions, carried from quad to quad; x - x0 + 1 is
// written to the map.  Backward: the run ends likewise, as a suffix minimum; the lane reads back what it wrote itself (program
// order: no barrier) and writes (wx min(x - x0 + 1, x1 - x + 1))^2, or 0 for a voxel that is not measured.  Runs compare raw
// labels: a label above n bounds its neighbours and is not measured itself.  Trip counts are wave-uniform; no workgroup barrier.
__global__ void __launch_bounds__(64 * ROW_WAVES) cc_depth_x_kernel(const u32* __restrict__ labels, u32 X, u64 nrows, u32 wx, u32 n,
                                                                  u32* map) {
    const int lane = threadIdx.x & 63;
    const u32 sweeps = (X + 511u) / 512u;
    for (u64 r = (u64)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6); r < nrows; r += (u64)gridDim.x * ROW_WAVES) {
        const u32* lrow = labels + r * X;
        u32* mrow = map + r * X;
        u32 carry = 0, edge = NO_VOXEL;  // the start of the run that reaches the quad from the left, and the label before the quad
        for (u32 sw = 0; sw < sweeps; ++sw) {
            const u32 xq[2] = {sw * 512u + 4u * lane, sw * 512u + 4u * lane + 256u};
            u32 l[VPT];
            load_quads<false>(lrow, true, xq, X, l);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u32 up = __shfl_up(l[4 * q + 3], 1, 64);
                const u32 before = lane ? up : edge;
                u32 s[4], last = 0;  // the start of voxel j's run where it lies in this quad, else 0 (the identity of the maximum)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    last = l[4 * q + j] != (j ? l[4 * q + j - 1] : before) ? xq[q] + j : last;
                    s[j] = last;
                }
                const u32 incl = wave_prefix_max(last, lane);
                const u32 below = __shfl_up(incl, 1, 64);
                const u32 reach = lane ? max(below, carry) : carry;
                u32 v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = xq[q] + j - max(s[j], reach) + 1u;
                store_quad(mrow, xq[q], X, v);
                carry = max(carry, __shfl(incl, 63, 64));
                edge = __shfl(l[4 * q + 3], 63, 64);
            }
        }
        carry = X - 1u, edge = NO_VOXEL;  // the end of the run that reaches the quad from the right, and the label after the quad
        for (u32 sw = sweeps; sw-- > 0;) {
            const u32 xq[2] = {sw * 512u + 4u * lane, sw * 512u + 4u * lane + 256u};
            u32 l[VPT];
            load_quads<false>(lrow, true, xq, X, l);
#pragma unroll
            for (int q = 1; q >= 0; --q) {
                const u32 down = __shfl_down(l[4 * q], 1, 64);
                const u32 after = lane < 63 ? down : edge;
                u32 e[4], first = NO_VOXEL;  // the end of voxel j's run where it lies in this quad, else the identity of the minimum
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    first = l[4 * q + j] != (j < 3 ? l[4 * q + j + 1] : after) ? xq[q] + j : first;
                    e[j] = first;
                }
                const u32 incl = wave_suffix_min(first, lane);
                const u32 above = __shfl_down(incl, 1, 64);
                const u32 reach = lane < 63 ? min(above, carry) : carry;
                u32 v[4];
                load_quad(mrow, xq[q], X, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32 lab = l[4 * q + j];
                    const u32 m = min(v[j], min(e[j], reach) - (xq[q] + j) + 1u);  // (<= ceil(X / 2) inside the row)
                    v[j] = (lab != 0 && lab <= n) ? (wx * m) * (wx * m) : 0u;
                }
                store_quad(mrow, xq[q], X, v);
                carry = min(carry, __shfl(incl, 0, 64));
                edge = __shfl(l[4 * q], 0, 64);
            }
        }
    }
}

// a wave's voxels under one label: the key of the deepest one and the sum of their values
struct DepthAcc {
    u64 key;
    u64 s;  // (<= 64 * 2^32 per wave)
    static __device__ __forceinline__ DepthAcc none() { return {0ull, 0ull}; }
    __device__ __forceinline__ void combine(int o) {
        xor_max(key, o);
        xor_add(s, o);
    }
};

// The y pass (along_z false: `line` is X) and the z pass (along_z true: `line` is Y * X; FOLD).  A workgroup walks whole rows, a
// thread a voxel of the row: 256 consecutive x.  src -> dst, never in place: a walk reads values of its pass' input only.  Every
// voxel of dst is written, 0 where the label is not measured.  FOLD: the lanes of a wave are folded by label (cc_fold.h), and the
// leader lane of a (wave, label) issues the two atomics.  Trip counts over rows and x are workgroup-uniform.
template <bool FOLD>
__global__ void __launch_bounds__(256) cc_depth_walk_kernel(const u32* __restrict__ labels, const u32* __restrict__ src,
                                                            u32* __restrict__ dst, int Z, int Y, int X, bool along_z, u32 w, u32 n,
                                                            u64* __restrict__ peak, u64* __restrict__ sum) {
    const u64 nrows = (u64)Z * Y;
    const long long line = along_z ? (long long)Y * X : (long long)X;
    const u32 dim = along_z ? (u32)Z : (u32)Y;
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u32 pos = along_z ? (u32)(r / (u64)Y) : (u32)(r % (u64)Y);
        const u64 row0 = r * (u64)X;
        for (u32 x0 = 0; x0 < (u32)X; x0 += blockDim.x) {
            const u32 x = x0 + threadIdx.x;
            const bool in = x < (u32)X;
            const u64 idx = row0 + x;
            const u32 lab = in ? labels[idx] : 0u;
            const bool measured = lab != 0 && lab <= n;
            u32 best = 0;
            if (measured) {
                best = src[idx];
                const u32* lp = labels + idx;
                const u32* gp = src + idx;
                for (u32 d = 1;; ++d) {
                    const u32 wd2 = (w * d) * (w * d);  // (w d < 65536 up to the step that leaves the volume)
                    if (wd2 >= best) break;
                    bool other = d > pos || pos + d >= dim;  // a side that leaves the volume
                    if (d <= pos) {
                        if (lp[-(long long)d * line] != lab) other = true;
                        else {
                            const u32 g = gp[-(long long)d * line];
                            best = g < best - wd2 ? g + wd2 : best;
                        }
                    }
                    if (pos + d < dim) {
                        if (lp[(long long)d * line] != lab) other = true;
                        else {
                            const u32 g = gp[(long long)d * line];  // (>= 1 under the label: best stays above wd2)
                            best = g < best - wd2 ? g + wd2 : best;
                        }
                    }
                    if (other) {  // (every farther position costs more than this one)
                        best = wd2;
                        break;
                    }
                }
            }
            if (in) dst[idx] = best;
            if (FOLD && __any(measured)) {  // (wave-uniform)
                const DepthAcc own = {((u64)best << 32) | (0xffffffffull - idx), (u64)best};
                wave_fold_by_label<true>(lab, measured, own, [&](u32 L, const DepthAcc& a) {
                    atomicMax(peak + L, a.key);
                    atomicAdd(sum + L, a.s);
                });
            }
        }
    }
}

}  // namespace

// the three passes for checked arguments (common.h): D2 into work_a, the keys and sums into the scratch slot; no read-back
int dlv_cc_depth_passes(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                        uint32_t* work_a_dev, uint32_t* work_b_dev, size_t extra_bytes, DlvDepthTables* out) {
    const u64 nvox = (u64)Z * Y * X;
    const size_t rows = (size_t)n + 1;
    // device accumulators: [key u64 rows | sum u64 rows | the caller's bytes]; an absent label keeps zeros
    WsCarve carve;
    const size_t off_key = carve.take(rows * 8), off_sum = carve.take(rows * 8), off_extra = carve.take(extra_bytes);
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, carve.end, (void**)&ws));
    DLV_HIP(ctx, hipMemsetAsync(ws, 0, carve.end, ctx->stream));
    const u64 nrows = (u64)Z * Y;
    const int gx = (int)std::min<u64>((nrows + ROW_WAVES - 1) / ROW_WAVES, (u64)256 * 32);
    const int gw = (int)std::min<u64>(nrows, (u64)256 * 32);
    // x: labels -> work_a; y: work_a -> work_b; z: work_b -> work_a
    {
        DlvProf pr(ctx, "cc_depth_x", 0.0, (double)nvox * 12);
        hipLaunchKernelGGL(cc_depth_x_kernel, dim3(gx), dim3(64 * ROW_WAVES), 0, ctx->stream, labels_dev, (u32)X, nrows, (u32)wx, (u32)n,
                           work_a_dev);
        pr.end();
    }
    DLV_LAUNCH_CHECK(ctx, "cc_depth_x_kernel");
    {
        DlvProf pr(ctx, "cc_depth_y", 0.0, (double)nvox * 12);
        hipLaunchKernelGGL(cc_depth_walk_kernel<false>, dim3(gw), dim3(256), 0, ctx->stream, labels_dev, (const u32*)work_a_dev, work_b_dev,
                           Z, Y, X, false, (u32)wy, (u32)n, (u64*)nullptr, (u64*)nullptr);
        pr.end();
    }
    DLV_LAUNCH_CHECK(ctx, "cc_depth_walk_kernel (y)");
    {
        DlvProf pr(ctx, "cc_depth_z", 0.0, (double)nvox * 12);
        hipLaunchKernelGGL(cc_depth_walk_kernel<true>, dim3(gw), dim3(256), 0, ctx->stream, labels_dev, (const u32*)work_b_dev, work_a_dev,
                           Z, Y, X, true, (u32)wz, (u32)n, (u64*)(ws + off_key), (u64*)(ws + off_sum));
        pr.end();
    }
    DLV_LAUNCH_CHECK(ctx, "cc_depth_walk_kernel (z)");
    out->key = (uint64_t*)(ws + off_key);
    out->sum = (uint64_t*)(ws + off_sum);
    out->extra = ws + off_extra;
    return DLV_OK;
}

extern "C" int dlv_cc_depth_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                                uint32_t* work_a_dev, uint32_t* work_b_dev, uint32_t* max_d2, uint64_t* sum_d2, uint64_t* peak_index) {
    if (!ctx) return DLV_EINVAL;
    if (!labels_dev || !work_a_dev || !work_b_dev) return dlv_fail(ctx, DLV_EINVAL, "cc_depth: labels_dev, work_a_dev or work_b_dev is NULL");
    if (!max_d2 || !sum_d2 || !peak_index) return dlv_fail(ctx, DLV_EINVAL, "cc_depth: max_d2, sum_d2 or peak_index is NULL");
    DLV_TRY(check_volume(ctx, "cc_depth", Z, Y, X));
    DLV_TRY(check_spacing(ctx, "cc_depth", "z", wz));
    DLV_TRY(check_spacing(ctx, "cc_depth", "y", wy));
    DLV_TRY(check_spacing(ctx, "cc_depth", "x", wx));
    DLV_TRY(check_label_count(ctx, "cc_depth", n));
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)work_a_dev & 3) || ((uintptr_t)work_b_dev & 3))
        return dlv_fail(ctx, DLV_EINVAL, "cc_depth: labels, work_a and work_b must be 4-byte aligned");
    DLV_TRY(check_reach(ctx, "cc_depth", "z", wz, Z));
    DLV_TRY(check_reach(ctx, "cc_depth", "y", wy, Y));
    DLV_TRY(check_reach(ctx, "cc_depth", "x", wx, X));
    const u64 nvox = (u64)Z * Y * X;  // (each dimension is below 2^17 here: no wrap)
    if (nvox > ((u64)1 << 32)) return dlv_fail(ctx, DLV_EUNSUP, "cc_depth: volumes above 2^32 voxels: the peak's index has 32 bits");
    const size_t bytes = (size_t)nvox * 4;
    if (ranges_overlap(work_a_dev, labels_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "cc_depth: work_a_dev overlaps labels_dev");
    if (ranges_overlap(work_b_dev, labels_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "cc_depth: work_b_dev overlaps labels_dev");
    if (ranges_overlap(work_b_dev, work_a_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "cc_depth: work_b_dev overlaps work_a_dev");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rows = (size_t)n + 1;
    DlvDepthTables t;
    DLV_TRY(dlv_cc_depth_passes(ctx, labels_dev, Z, Y, X, n, wz, wy, wx, work_a_dev, work_b_dev, 0, &t));
    std::vector<u64> keys(rows);
    DLV_HIP(ctx, hipMemcpyAsync(keys.data(), t.key, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(sum_d2, t.sum, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t l = 0; l < rows; ++l) {  // (key 0: no voxel)
        max_d2[l] = (uint32_t)(keys[l] >> 32);
        peak_index[l] = keys[l] ? 0xffffffffull - (keys[l] & 0xffffffffull) : ~0ull;
    }
    return DLV_OK;
}
