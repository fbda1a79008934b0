// cc_fold.h - the device pieces the per-label statistics kernels share (cc_stats.hip, cc_intensity.hip, cc_shape.hip,
// cc_quantiles.hip): the sweep geometry of a row, its quad loads, and the aggregation of a wave's contributions by label - folded
// into one value per label (wave_fold_by_label) or ranked into places (wave_rank_by_label).  Header only, no state.
//
// Sweep layout.  A workgroup of T threads walks whole rows (z, y) of the label volume - no per-thread 64-bit division, and
// arrays of different pitches are addressed from their own row starts.  A row is cut into sweeps of 8 T voxels; in a sweep
// thread t takes the two quads [4t, 4t+4) and [4(T+t), 4(T+t)+4), so that each of its vector loads is part of one contiguous run
// per wave instruction (1 KiB of labels) - with 8 consecutive voxels per thread every instruction touched half of each line.
// Trip counts over rows and sweeps are workgroup-uniform, and 0xffffffff stands for "no voxel" (past the row's end).
// Aggregation.  Contributions are combined before they reach memory: a thread folds its voxels of equal label into one
// accumulator, the lanes of a wave that hold the same label are reduced with shuffles, and ONE leader lane per (wave, label)
// issues the atomics - a brain-sized single component would otherwise serialise hundreds of millions of atomics on one address.
#pragma once
#include <hip/hip_runtime.h>

#include "cc_types.h"

namespace {

constexpr int VPT = 8;                 // voxels per thread and sweep: two quads of one row
constexpr u32 NO_VOXEL = 0xffffffffu;  // differs from every label 0..n (n < 2^32 - 1)

__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
    const u32 lo = __shfl_xor((u32)v, o, 64), hi = __shfl_xor((u32)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}

// one butterfly step of a wave-wide sum / minimum / maximum (the identities: 0, NO_VOXEL, 0)
__device__ __forceinline__ void xor_add(u32& v, int o) { v += __shfl_xor(v, o, 64); }
__device__ __forceinline__ void xor_add(u64& v, int o) { v += shfl_xor64(v, o); }
__device__ __forceinline__ void xor_min(u32& v, int o) { v = min(v, __shfl_xor(v, o, 64)); }
__device__ __forceinline__ void xor_max(u32& v, int o) { v = max(v, __shfl_xor(v, o, 64)); }
__device__ __forceinline__ void xor_min(u64& v, int o) { v = min(v, shfl_xor64(v, o)); }
__device__ __forceinline__ void xor_max(u64& v, int o) { v = max(v, shfl_xor64(v, o)); }

__device__ __forceinline__ int row_sweeps(int X) { return (X + (int)blockDim.x * VPT - 1) / ((int)blockDim.x * VPT); }

// quad q of this thread starts at xq[q] in sweep sw; voxel k = 4q + j sits at xq[q] + j
__device__ __forceinline__ void quad_starts(int sw, u32 (&xq)[2]) {
    xq[0] = (u32)sw * blockDim.x * VPT + 4u * threadIdx.x;
    xq[1] = xq[0] + 4u * blockDim.x;
}
__device__ __forceinline__ u32 voxel_x(const u32 (&xq)[2], int k) { return xq[k >> 2] + (u32)(k & 3); }

// NT: a nontemporal vector load for a kernel that streams the array once; a plain one where rows are read again
template <bool NT, typename V>
__device__ __forceinline__ V load_vec(const V* p) { return NT ? __builtin_nontemporal_load(p) : *p; }

// the thread's two label quads of one row: 16-byte loads where the row starts on a 16-byte boundary and the quad lies inside
// it - decided per row: with an odd X the alignment changes from row to row -, element by element elsewhere; NO_VOXEL past the
// end of the row and for a row outside the buffer (exists == false: row is not read)
template <bool NT>
__device__ __forceinline__ void load_quads(const u32* __restrict__ row, bool exists, const u32 (&xq)[2], u32 X, u32 (&v)[VPT]) {
    const bool vec = exists && (reinterpret_cast<uintptr_t>(row) & 15) == 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (vec && xq[q] + 4u <= X) {
            const u32x4_t u = load_vec<NT>(reinterpret_cast<const u32x4_t*>(row + xq[q]));
            v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * q + j] = (exists && xq[q] + j < X) ? row[xq[q] + j] : NO_VOXEL;
        }
    }
}

// its twin for a row of the raw uint16 volume: 8-byte loads where the row starts on an 8-byte boundary, 0 past the end
template <bool NT>
__device__ __forceinline__ void load_raw_quads(const unsigned short* __restrict__ row, const u32 (&xq)[2], u32 X, u32 (&v)[VPT]) {
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 7) == 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (vec && xq[q] + 4u <= X) {
            const u32x2_t u = load_vec<NT>(reinterpret_cast<const u32x2_t*>(row + xq[q]));
            v[4 * q] = u.x & 0xffffu; v[4 * q + 1] = u.x >> 16; v[4 * q + 2] = u.y & 0xffffu; v[4 * q + 3] = u.y >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * q + j] = (xq[q] + j < X) ? (u32)row[xq[q] + j] : 0u;
        }
    }
}

// its twin for a row of a float volume: 16-byte loads where the row starts on a 16-byte boundary, 0.0f past the end
template <bool NT>
__device__ __forceinline__ void load_float_quads(const float* __restrict__ row, const u32 (&xq)[2], u32 X, float (&v)[VPT]) {
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (vec && xq[q] + 4u <= X) {
            const f32x4_t u = load_vec<NT>(reinterpret_cast<const f32x4_t*>(row + xq[q]));
            v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * q + j] = (xq[q] + j < X) ? row[xq[q] + j] : 0.0f;
        }
    }
}

// bit k: voxel k holds a label 1..n (background, labels above n and NO_VOXEL are not measured)
__device__ __forceinline__ unsigned fg_mask(const u32 (&l)[VPT], u32 n) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < VPT; ++k) m |= ((l[k] != 0 && l[k] <= n) ? 1u : 0u) << k;
    return m;
}

// the label at the lowest set bit of m (0 for an empty m), without a dynamic index into the registers
__device__ __forceinline__ u32 first_label(const u32 (&l)[VPT], unsigned m) {
    const int k0 = __ffs((int)m) - 1;
    u32 lab = 0;
#pragma unroll
    for (int k = 0; k < VPT; ++k) lab = (k == k0) ? l[k] : lab;
    return lab;
}

// THE LEADER LOOP.  The lanes of a wave that hold the same label are combined, and one leader lane per distinct label calls emit(L, w) with the
// wave's total w for the label L: that is where a kernel issues its atomics.  Acc is the kernel's accumulator: static none()
// gives the identity, combine(o) is one butterfly step on itself (xor_add / xor_min / xor_max of every field).
// CONVERGENCE: every lane of the wave must reach the call, under wave-uniform control flow (__any / __ballot or workgroup-
// uniform trip counts decide the branches and loops around it); `have` is false for a lane with nothing (lab, own: ignored).
// SKIP_SINGLE: a label that one lane alone holds - a cell's one run in this stretch of the row, the common case of a cell mask -
// is emitted without the reduction: the leader's own values are the wave's (a second ballot per label buys six shuffle rounds).
template <bool SKIP_SINGLE, typename Acc, typename Emit>
__device__ __forceinline__ void wave_fold_by_label(u32 lab, bool have, const Acc& own, Emit emit) {
    const int lane = threadIdx.x & 63;
    bool pending = have;
    while (true) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const u32 L = __shfl(lab, leader, 64);
        const bool mine = pending && lab == L;
        Acc w = mine ? own : Acc::none();
        if (!SKIP_SINGLE || __popcll(__ballot(mine)) > 1)  // (wave-uniform)
            for (int o = 32; o > 0; o >>= 1) w.combine(o);
        if (lane == leader) emit(L, w);
        pending = pending && !mine;
    }
}

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const u32 lo = __shfl((u32)v, src, 64), hi = __shfl((u32)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

// THE RANK LOOP, the leader loop's twin for a kernel that hands out places instead of folding values (cc_quantiles.hip): a
// lane that holds cnt items of the label lab learns where they go in the wave's contribution to that label.  leader: the first
// lane with the label - the one that reserves `total` places with ONE returning atomic; before: the items of the lanes below this
// one that hold the same label (its exclusive rank); total: the items of all of them.  A lane without `have` names itself as its
// leader, with total 0.  No atomic is issued in here, so the leaders of all labels of the wave can issue theirs in one instruction
// afterwards and every lane reads its base with one shuffle from its leader.
// CONVERGENCE: as for wave_fold_by_label.  A label that one lane alone holds skips the scan.
struct LabelRank {
    int leader;
    u32 before, total;
};
__device__ __forceinline__ LabelRank wave_rank_by_label(u32 lab, bool have, u32 cnt) {
    const int lane = threadIdx.x & 63;
    LabelRank r = {lane, 0u, 0u};
    bool pending = have;
    while (true) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const u32 L = __shfl(lab, leader, 64);
        const bool mine = pending && lab == L;
        const u32 own = mine ? cnt : 0u;
        u32 incl = own;
        const bool single = __popcll(__ballot(mine)) == 1;  // (wave-uniform)
        if (!single)
            for (int o = 1; o < 64; o <<= 1) {
                const u32 up = __shfl_up(incl, o, 64);
                incl += lane >= o ? up : 0u;
            }
        const u32 total = __shfl(incl, single ? leader : 63, 64);
        if (mine) r = {leader, incl - own, total};
        pending = pending && !mine;
    }
    return r;
}

}  // namespace
