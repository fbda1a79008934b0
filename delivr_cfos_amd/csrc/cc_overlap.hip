// cc_overlap.hip - the overlap table of two label volumes on the device (dlv_cc_overlap_count_dev, dlv_cc_overlap_dev): every pair
// of labels (a, b) that share voxels, with the number of voxels they share - what compare_cells.py turns into detection precision /
// recall, merges, splits and per-cell partners.  The reference has no counterpart.  A voxel takes part when 1 <= a <= n_a and
// 1 <= b <= n_b; its key is (a << 32) | b, never 0.  compare_cells.overlap_table_np is the numpy statement of the result.
//
// Count.  cc_fold.h's row sweep with workgroups of ONE wave, as cc_runs.hip: a wave walks whole rows in sweeps of 512 voxels and
// loads the quads of both volumes.  A pair segment is a maximal stretch of one key inside a row; a voxel starts one when its key
// differs from the key of the voxel before it (0 outside the row and for a voxel that takes no part), which a lane learns from the
// lane below it (lane 0: from memory).  The number of segments S bounds the number of distinct pairs P, and so does n_a * n_b: the
// caller sizes the table and the outputs from min(S, n_a * n_b).
// Insert.  An open-addressed table in HBM (cc_pair_table.h, shared with cc_neighbours.hip): cap slots (a power of two >= 2 * min(S, n_a * n_b)) of {uint64 key, uint64 voxels},
// zeroed first, key 0 = empty.  A key is hashed with the 64-bit finaliser of splitmix64 and probed linearly: a relaxed load of the
// slot's key, a 64-bit compare-and-swap where it reads empty, and a 64-bit atomic add on the voxels of the slot that holds the key.
// Contributions are combined before they reach memory, in three steps:
//   - a sweep whose voxels all hold ONE key (the inside of a large cell over a large cell, or the one small pair of a sparse mask)
//     is added to a carry the wave keeps in registers - every lane its own voxels, no shuffle -, and the carry is reduced and
//     inserted by one lane only when another key takes its place or the wave has walked its last row: a brain-sized component of A
//     over a brain-sized component of B costs one atomic per (wave, change of key), not one per voxel or per sweep;
//   - elsewhere a thread folds the stretches of equal key among its eight voxels into items (as cc_counts_fold does), and
//   - the lanes that hold the same key are reduced by a leader loop on the 64-bit key (wave_fold_by_key, the twin of cc_fold.h's
//     wave_fold_by_label; like wave_rank_by_label it issues no atomic itself), after which the leaders of ALL keys of the wave probe
//     side by side: the compare-and-swap returns a value, and a probe per pass of the leader loop would put those latencies in a row.
// Compact.  One pass over the slots writes the occupied ones to keys_out / voxels_out at a cursor advanced once per wave and 512
// slots (eight ballots + popcounts, one returning atomic: with one atomic per 64 slots the pass ran at the rate of that one word,
// 0.40 ms for 2 million slots).  The device order is unspecified; HipEngine.cc_overlap sorts by key on the host.
//
// Every loop is bounded: a probe visits at most cap slots, and a key that finds none - or an occupied slot beyond out_cap - sets an
// overflow word, which the host turns into an error that names the table.  With the S of the count on the same volumes neither can
// happen (P <= min(S, n_a * n_b) <= cap / 2).  No loop waits for another wave or spins on memory.  Integer work only, and the
// additions commute: the table is exact and independent of scheduling.  Deviation from the issue's sketch: the carry above.
//
// Measured once on an MI355X (profiles/README.md, "cc_overlap"; count / table / compact, and cc_stats_kernel on the labels of A):
// 512^3 labels of a 1 % cell mask against the same mask moved by one voxel (671 008 segments, 167 752 pairs, 2^21 slots = 32 MiB)
// 0.180 / 0.461 / 0.059 ms beside 3.36 ms; labels of a 50 % random mask against another's (25.2 million segments, 11 pairs - such a
// mask is one component and a few specks -, 256 slots; the largest pair holds 33.5 million voxels) 0.242 / 0.532 / 0.007 ms beside
// 48.5 ms: the carry keeps the one heavy slot out of the way.  1024 x 2048 x 2048, the bench's cell mask against itself moved by one
// voxel (2.88 million segments, 538 627 pairs, 2^23 slots = 128 MiB): 5.57 / 5.55 / 0.21 ms beside 5.01 ms - count and insert read
// their 8 bytes per voxel at 6.2 TB/s, 1.11 of a cc_stats pass each, against the bound of two.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"
#include "cc_pair_table.h"

#include <algorithm>

namespace {

constexpr int OT = 64;                    // threads per workgroup: one wave, one row at a time
constexpr u64 OVERLAP_MAX_WG = 256 * 32;  // workgroups per launch; rows beyond that are walked grid-stride
constexpr int MAX_X = 1 << 30;            // (the sweep arithmetic is 32-bit)

// The keys of this lane's two quads of sweep sw of row r (0: the voxel takes no part or lies past the row's end).  Returns false -
// for the whole wave - where the sweep holds no key.
__device__ __forceinline__ bool load_keys(const u32* __restrict__ row_a, const u32* __restrict__ row_b, u32 X, int sw, u32 n_a, u32 n_b,
                                          u32 (&xq)[2], u64 (&key)[VPT]) {
    u32 la[VPT], lb[VPT];
    quad_starts(sw, xq);
    load_quads<true>(row_a, true, xq, X, la);
    load_quads<true>(row_b, true, xq, X, lb);
    bool any = false;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        // (l - 1 < n: false for 0, for NO_VOXEL and for a label above n, n <= 2^32 - 2)
        const bool in = la[k] - 1u < n_a && lb[k] - 1u < n_b;
        key[k] = in ? ((u64)la[k] << 32) | lb[k] : 0ull;
        any |= in;
    }
    return __any(any);
}

__device__ __forceinline__ u64 key_at(const u32* __restrict__ row_a, const u32* __restrict__ row_b, u32 x, u32 n_a, u32 n_b) {
    const u32 a = row_a[x], b = row_b[x];
    return (a - 1u < n_a && b - 1u < n_b) ? ((u64)a << 32) | b : 0ull;
}

// ---- count: *total += the pair segments of the volume ------------------------------------------------------------------------
__global__ void __launch_bounds__(OT) cc_overlap_count_kernel(const u32* __restrict__ a, const u32* __restrict__ b, u64 nrows, int X, u32 n_a,
                                                              u32 n_b, u64* __restrict__ total) {
    const int lane = threadIdx.x & 63;
    const int sweeps = row_sweeps(X);
    u64 c = 0;  // this lane's segment starts
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u32 *row_a = a + r * (u64)X, *row_b = b + r * (u64)X;
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2];
            u64 key[VPT];
            if (!load_keys(row_a, row_b, (u32)X, sw, n_a, n_b, xq, key)) continue;  // (wave-uniform)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                u64 before = shfl64(key[4 * q + 3], (lane + 63) & 63);  // the lane below this one
                // (xq - 1 < X also keeps a quad past the row's end inside the row)
                if (lane == 0) before = (xq[q] > 0 && xq[q] - 1u < (u32)X) ? key_at(row_a, row_b, xq[q] - 1u, n_a, n_b) : 0ull;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u64 k = key[4 * q + j];
                    c += (k != 0 && k != before) ? 1u : 0u;
                    before = k;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) xor_add(c, o);
    if (lane == 0 && c) atomicAdd(total + W_COUNT, c);
}

// ---- insert ------------------------------------------------------------------------------------------------------------------
// voxels of `key` into its slot (cc_pair_table.h: at most cap probes, the overflow word where no slot is left)
__device__ __forceinline__ void table_add(u64* __restrict__ table, u64 cap, u64 key, u64 voxels, u64* __restrict__ words) {
    if (u64* at = pair_slot(table, cap, key, words)) atomicAdd(at, voxels);
}

// THE LEADER LOOP ON A 64-BIT KEY, the twin of cc_fold.h's wave_fold_by_label: the lanes of a wave that hold the same key are
// combined, and the first of them learns the wave's total for the key.  No atomic is issued in here (as in wave_rank_by_label), so
// the leaders of all keys act together afterwards.  CONVERGENCE: every lane of the wave must reach the call, under wave-uniform
// control flow; `have` is false for a lane with nothing (key, cnt: ignored).  A key that one lane alone holds skips the reduction.
struct KeyFold {
    bool leader;
    u32 total;
};
__device__ __forceinline__ KeyFold wave_fold_by_key(u64 key, bool have, u32 cnt) {
    const int lane = threadIdx.x & 63;
    KeyFold r = {false, 0u};
    bool pending = have;
    while (true) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const u64 K = shfl64(key, leader);
        const bool mine = pending && key == K;
        u32 w = mine ? cnt : 0u;
        if (__popcll(__ballot(mine)) > 1)  // (wave-uniform)
            for (int o = 32; o > 0; o >>= 1) xor_add(w, o);
        if (lane == leader) r = {true, w};
        pending = pending && !mine;
    }
    return r;
}

__global__ void __launch_bounds__(OT) cc_overlap_insert_kernel(const u32* __restrict__ a, const u32* __restrict__ b, u64 nrows, int X, u32 n_a,
                                                               u32 n_b, u64* __restrict__ table, u64 cap, u64* __restrict__ words) {
    const int lane = threadIdx.x & 63;
    const int sweeps = row_sweeps(X);
    u64 carry_key = 0;  // (wave-uniform) the key of the sweeps of one key seen last
    u64 carry = 0;      // this lane's voxels of it
    auto flush = [&]() {  // (called under wave-uniform control flow)
        if (carry_key == 0) return;
        for (int o = 32; o > 0; o >>= 1) xor_add(carry, o);
        if (lane == 0) table_add(table, cap, carry_key, carry, words);
        carry = 0;
    };
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u32 *row_a = a + r * (u64)X, *row_b = b + r * (u64)X;
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2];
            u64 key[VPT];
            if (!load_keys(row_a, row_b, (u32)X, sw, n_a, n_b, xq, key)) continue;  // (wave-uniform)
            // bit k of in: voxel k holds a key; bit k of chg: it starts a stretch (differs from the voxel before it in the registers:
            // the two quads are not neighbours in the row, which a sum does not mind)
            unsigned in = 0, chg = 1u | (1u << VPT);
            u64 mine = 0;  // a key of this lane (0: none)
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                in |= (key[k] != 0 ? 1u : 0u) << k;
                if (k > 0) chg |= (key[k] != key[k - 1] ? 1u : 0u) << k;
                mine = key[k] != 0 ? key[k] : mine;
            }
            // one key in the whole sweep: into the carry
            const unsigned long long holders = __ballot(in != 0);
            const u64 K = shfl64(mine, __ffsll((long long)holders) - 1);
            bool other = false;
#pragma unroll
            for (int k = 0; k < VPT; ++k) other |= key[k] != 0 && key[k] != K;
            if (!__any(other)) {  // (wave-uniform)
                if (K != carry_key) {
                    flush();
                    carry_key = K;
                }
                carry += (u64)__popc(in);
                continue;
            }
            // several keys: items per thread, the leader loop per round of items, the leaders' probes side by side
            unsigned starts = in & chg;
            while (__any(starts != 0)) {  // (wave-uniform; at most VPT rounds)
                const bool have = starts != 0;
                u64 item = 0;
                u32 cnt = 0;
                if (have) {
                    const int k0 = __ffs((int)starts) - 1;
#pragma unroll
                    for (int k = 0; k < VPT; ++k) item = (k == k0) ? key[k] : item;
                    starts &= starts - 1;
                    cnt = (u32)(__ffs((int)(chg >> (k0 + 1))) - 1) + 1u;  // up to the next stretch's start (bit VPT ends the last one)
                }
                const KeyFold f = wave_fold_by_key(item, have, cnt);
                if (f.leader) table_add(table, cap, item, (u64)f.total, words);
            }
        }
    }
    flush();
}

// what both entries check of the volumes, before anything is launched
int overlap_args(dlv_ctx* ctx, const char* what, const void* a_dev, const void* b_dev, int Z, int Y, int X, uint64_t n_a, uint64_t n_b) {
    DLV_TRY(check_volume(ctx, what, Z, Y, X));
    if (X > MAX_X) return dlv_fail(ctx, DLV_EUNSUP, "%s: X = %d exceeds %d", what, X, MAX_X);
    if (n_a > 0xfffffffeull || n_b > 0xfffffffeull)
        return dlv_fail(ctx, DLV_EINVAL, "%s: n_a = %llu, n_b = %llu do not fit the uint32 labels", what, (unsigned long long)n_a,
                        (unsigned long long)n_b);
    if (((uintptr_t)a_dev & 3) || ((uintptr_t)b_dev & 3)) return dlv_fail(ctx, DLV_EINVAL, "%s: the label volumes must be 4-byte aligned", what);
    return DLV_OK;
}

unsigned overlap_grid(u64 nrows) { return (unsigned)std::min<u64>(nrows, OVERLAP_MAX_WG); }

}  // namespace

extern "C" {

int dlv_cc_overlap_count_dev(dlv_ctx* ctx, const uint32_t* a_dev, const uint32_t* b_dev, int Z, int Y, int X, uint64_t n_a, uint64_t n_b,
                             uint64_t* n_segments) {
    if (!ctx || !a_dev || !b_dev || !n_segments) return DLV_EINVAL;
    DLV_TRY(overlap_args(ctx, "cc_overlap_count", a_dev, b_dev, Z, Y, X, n_a, n_b));
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nrows = (u64)Z * Y;
    u64* words;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, W_WORDS * 8, (void**)&words));
    DLV_HIP(ctx, hipMemsetAsync(words, 0, W_WORDS * 8, ctx->stream));
    DlvProf pr(ctx, "cc_overlap_count", 0.0, (double)nrows * X * 8);
    hipLaunchKernelGGL(cc_overlap_count_kernel, dim3(overlap_grid(nrows)), dim3(OT), 0, ctx->stream, a_dev, b_dev, nrows, X, (u32)n_a, (u32)n_b,
                       words);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_overlap_count_kernel");
    u64 s = 0;
    DLV_HIP(ctx, hipMemcpyAsync(&s, words + W_COUNT, 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_segments = s;
    return DLV_OK;
}

int dlv_cc_overlap_dev(dlv_ctx* ctx, const uint32_t* a_dev, const uint32_t* b_dev, int Z, int Y, int X, uint64_t n_a, uint64_t n_b,
                       uint64_t n_segments, uint64_t* table_dev, uint64_t cap, uint64_t* keys_out_dev, uint64_t* voxels_out_dev,
                       uint64_t out_cap, uint64_t* n_pairs) {
    if (!ctx || !a_dev || !b_dev || !table_dev || !keys_out_dev || !voxels_out_dev || !n_pairs) return DLV_EINVAL;
    DLV_TRY(overlap_args(ctx, "cc_overlap", a_dev, b_dev, Z, Y, X, n_a, n_b));
    if (((uintptr_t)table_dev & 15) || ((uintptr_t)keys_out_dev & 7) || ((uintptr_t)voxels_out_dev & 7))
        return dlv_fail(ctx, DLV_EINVAL, "cc_overlap: the table must be 16-byte, the outputs 8-byte aligned");
    // P <= min(S, n_a * n_b)
    const u64 bound = std::min<u64>(n_segments, (u64)n_a * (u64)n_b);  // (n < 2^32: the product fits)
    if (bound > (1ull << 62)) return dlv_fail(ctx, DLV_EINVAL, "cc_overlap: %llu segments are beyond any table", (unsigned long long)n_segments);
    if (cap == 0 || (cap & (cap - 1)) || cap < 2 * bound)
        return dlv_fail(ctx, DLV_EINVAL, "cc_overlap: a table of %llu slots; expected a power of two >= 2 * min(segments, n_a * n_b) = %llu",
                        (unsigned long long)cap, (unsigned long long)(2 * bound));
    if (out_cap < bound)
        return dlv_fail(ctx, DLV_EINVAL, "cc_overlap: outputs of %llu entries; min(segments, n_a * n_b) = %llu", (unsigned long long)out_cap,
                        (unsigned long long)bound);
    if (bound == 0) {  // no voxel takes part: nothing to launch
        *n_pairs = 0;
        return DLV_OK;
    }
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nrows = (u64)Z * Y;
    u64* words;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, W_WORDS * 8, (void**)&words));
    DLV_HIP(ctx, hipMemsetAsync(words, 0, W_WORDS * 8, ctx->stream));
    {
        DlvProf pr(ctx, "cc_overlap_table", 0.0, (double)nrows * X * 8 + (double)cap * 16);
        DLV_HIP(ctx, hipMemsetAsync(table_dev, 0, (size_t)cap * 16, ctx->stream));
        hipLaunchKernelGGL(cc_overlap_insert_kernel, dim3(overlap_grid(nrows)), dim3(OT), 0, ctx->stream, a_dev, b_dev, nrows, X, (u32)n_a,
                           (u32)n_b, (u64*)table_dev, (u64)cap, words);
        pr.end();
    }
    DLV_LAUNCH_CHECK(ctx, "cc_overlap_insert_kernel");
    {
        DlvProf pr(ctx, "cc_overlap_compact", 0.0, (double)cap * 16);
        hipLaunchKernelGGL(pair_table_compact_kernel<u64>, dim3(pair_table_compact_grid(cap)), dim3(PT_CT), 0, ctx->stream, (const u64*)table_dev,
                           (u64)cap, (u64*)keys_out_dev, (u64*)voxels_out_dev, (u64)out_cap, words);
        pr.end();
    }
    DLV_LAUNCH_CHECK(ctx, "pair_table_compact_kernel");
    u64 host[W_WORDS] = {0, 0};
    DLV_HIP(ctx, hipMemcpyAsync(host, words, W_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (host[W_OVERFLOW])
        return dlv_fail(ctx, DLV_ESTATE, "cc_overlap: the pair table of %llu slots (outputs of %llu entries) overflowed: %llu segments is not the "
                        "count of these volumes", (unsigned long long)cap, (unsigned long long)out_cap, (unsigned long long)n_segments);
    *n_pairs = host[W_COUNT];
    return DLV_OK;
}

}  // extern "C"
