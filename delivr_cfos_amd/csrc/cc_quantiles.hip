// cc_quantiles.hip - per-label order statistics of the raw uint16 volume under a label volume (dlv_cc_quantiles_dev): for a
// label with m voxels whose raw values sorted ascending are v[0..m), the level p (per cent) reads v[(p (m - 1)) / 100] - the
// "lower" quantile, a value the label holds.  The moment statistics of cc_intensity.hip fold additively per wave; order
// statistics do not, so this is a kernel pair of its own: GATHER every label's values into its segment of one value buffer, then
// SELECT the ranks in every segment.
//
//   1. counts and offsets: the counting kernel of cc_stats.hip (dlv_cc_counts_dev), the exclusive prefix sum of the n + 1 counts
//      on the host into 64-bit offsets (the foreground of a brain-sized mask can exceed 2^32 voxels).
//   2. gather: one streaming pass over labels and raw in the sweep layout of cc_fold.h.  Places are handed out per (wave, label):
//      the lanes that hold a label rank themselves (wave_rank_by_label), the first of them reserves the wave's places with ONE
//      returning atomic on the label's cursor - the leaders of all labels of a wave in the same instruction -, and every lane
//      stores its values behind the base it reads from its leader.  The order inside a segment depends on scheduling; the
//      selection does not depend on the order.
//   3. select: for every level the largest t with #{v < t} <= rank is v[rank]; t is built bit by bit from the top, 16 rounds, all
//      levels counted in the same pass.
//      Segments of up to SMALL_MAX = 512 values: one wave per label, the segment loaded once into 8 registers per lane; a count is
//      a compare and the population count of its lane mask, so the 16 rounds run on wave-uniform scalars without a shuffle.
//      Longer segments (THE CHOICE the interface leaves open): one workgroup per label and a two-pass byte histogram in LDS
//      instead of 16 passes of one wave over memory - pass 1 counts the high bytes and finds, per level, the high byte that holds
//      the rank and the rank inside it; pass 2 counts the low bytes of the values with that high byte.  The segment is read
//      twice, with 16-byte loads; the bins are 32-bit, enough for any m < 2^32.  The host lists these labels from the counts.
//
// Integer work only: the result is exact and independent of scheduling.  After the gather a label's cursor is its segment's
// end, which is the start of the next label's segment: the selection needs no second table.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"

#include <algorithm>
#include <vector>

extern "C" int dlv_cc_counts_dev(dlv_ctx* ctx, const uint32_t* labels_dev, uint64_t nvox, uint64_t n, uint32_t* counts_dev);

namespace {

constexpr int MAX_LEVELS = 8;
constexpr int SMALL_REGS = 8;                  // values per lane of the one-wave selection
constexpr u32 SMALL_MAX = 64 * SMALL_REGS;     // the longest segment it takes
constexpr u32 NO_VALUE = 0xffffffffu;          // below no candidate: an empty place of the registers

struct Levels {
    int n;
    int p[MAX_LEVELS];
};

// ---- gather -----------------------------------------------------------------------------------------------------------
// cc_intensity_kernel's walk (labels by their own rows, raw by its pitches, both nontemporal, a wave without a label 1..n skips
// its raw loads).  A thread takes the voxels of equal label among its 8 in one pass, as there; cursor[l] starts as the offset of
// l's segment and ends as its end.  cap = the places of the buffer: a store is checked against it (labels that changed between
// the counting and this pass must not write past the buffer).
__global__ void __launch_bounds__(256) cc_gather_kernel(const u32* __restrict__ labels, const unsigned short* __restrict__ raw,
                                                        int Z, int Y, int X, long long pitch_y, long long pitch_z, u32 n,
                                                        u64* __restrict__ cursor, unsigned short* __restrict__ vals, u64 cap) {
    const u64 nrows = (u64)Z * Y;
    const int sweeps = row_sweeps(X);
    const int lane = threadIdx.x & 63;
    for (u64 row = blockIdx.x; row < nrows; row += gridDim.x) {
        const u32 z = (u32)(row / (u64)Y), y = (u32)(row % (u64)Y);
        const u32* lrow = labels + row * (u64)X;
        const unsigned short* rrow = raw + (u64)z * (u64)pitch_z + (u64)y * (u64)pitch_y;
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2], l[VPT], r[VPT];
            quad_starts(sw, xq);
            load_quads<true>(lrow, true, xq, (u32)X, l);
            unsigned todo = fg_mask(l, n);    // the voxels that have no place yet
            if (!__any(todo != 0)) continue;  // (wave-uniform) nothing to gather in this wave's 512 voxels
            load_raw_quads<true>(rrow, xq, (u32)X, r);
            // one pass per distinct label of the thread (one, as a rule)
            while (__any(todo != 0)) {
                const bool have = todo != 0;
                const u32 lab = first_label(l, todo);
                unsigned in = 0;  // the thread's voxels of this label
#pragma unroll
                for (int k = 0; k < VPT; ++k) in |= ((((todo >> k) & 1u) && l[k] == lab) ? 1u : 0u) << k;
                todo &= ~in;
                const LabelRank rk = wave_rank_by_label(lab, have, (u32)__popc(in));
                u64 base = 0;
                if (have && lane == rk.leader) base = atomicAdd(cursor + lab, (u64)rk.total);
                u64 slot = shfl64(base, rk.leader) + rk.before;
#pragma unroll
                for (int k = 0; k < VPT; ++k)
                    if ((in >> k) & 1u) {
                        if (slot < cap) vals[slot] = (unsigned short)r[k];
                        ++slot;
                    }
            }
        }
    }
}

// ---- select: segments of up to SMALL_MAX values, one wave per label ---------------------------------------------------------
__global__ void __launch_bounds__(256) cc_select_small_kernel(const unsigned short* __restrict__ vals, const u64* __restrict__ cursor,
                                                              u32 n, Levels lv, u64 cap, unsigned short* __restrict__ out) {
    const u64 label = (u64)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64 + 1;
    if (label > n) return;  // (wave-uniform: the whole wave leaves)
    const int lane = threadIdx.x & 63;
    const u64 start = cursor[label - 1], end = cursor[label];
    if (end <= start || end - start > SMALL_MAX || end > cap) return;  // absent (its row stays 0), or the workgroup kernel's; (cap: as in the gather)
    const u32 m = (u32)(end - start);
    const int nreg = (int)((m + 63) / 64);
    u32 v[SMALL_REGS];
#pragma unroll
    for (int j = 0; j < SMALL_REGS; ++j) {
        const u32 i = (u32)j * 64 + (u32)lane;
        v[j] = (j < nreg && i < m) ? (u32)vals[start + i] : NO_VALUE;
    }
    u32 rank[MAX_LEVELS], ans[MAX_LEVELS];
#pragma unroll
    for (int i = 0; i < MAX_LEVELS; ++i) {
        rank[i] = i < lv.n ? ((u32)lv.p[i] * (m - 1)) / 100u : 0u;  // (100 * 511 fits)
        ans[i] = 0;
    }
    for (int bit = 15; bit >= 0; --bit) {
#pragma unroll
        for (int i = 0; i < MAX_LEVELS; ++i) {
            if (i >= lv.n) break;  // (uniform)
            const u32 cand = ans[i] | (1u << bit);
            u32 below = 0;  // #{v < cand}, wave-uniform
#pragma unroll
            for (int j = 0; j < SMALL_REGS; ++j)
                if (j < nreg) below += (u32)__popcll(__ballot(v[j] < cand));
            if (below <= rank[i]) ans[i] = cand;
        }
    }
#pragma unroll
    for (int i = 0; i < MAX_LEVELS; ++i)
        if (i < lv.n && lane == i) out[label * (u64)lv.n + i] = (unsigned short)ans[i];
}

// ---- select: longer segments, one workgroup per label, two passes of byte histograms ---------------------------------------
// one more value of bin `bin` in a histogram in LDS, called by any set of lanes: where all of them hit the same bin (a constant
// region of the raw volume: every lane would queue on one LDS word), the first adds for all
__device__ __forceinline__ void hist_add(u32* hist, u32 bin) {
    const unsigned long long active = __ballot(true);
    const u32 first = (u32)__builtin_amdgcn_readfirstlane((int)bin);
    if (__ballot(bin == first) == active) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)active) - 1) atomicAdd(hist + first, (u32)__popcll(active));
    } else {
        atomicAdd(hist + bin, 1u);
    }
}

// PASS 0: hist[0] counts the high bytes.  PASS 1: hist[i] counts the low bytes of the values whose high byte is level i's
__device__ __forceinline__ void hist_value(u32 (*hist)[256], int pass, const u32* hi_bin, int nl, u32 v) {
    if (pass == 0) {
        hist_add(hist[0], v >> 8);
    } else {
        for (int i = 0; i < nl; ++i)
            if ((v >> 8) == hi_bin[i]) hist_add(hist[i], v & 255u);
    }
}

__global__ void __launch_bounds__(256) cc_select_large_kernel(const unsigned short* __restrict__ vals, const u64* __restrict__ cursor,
                                                              const u32* __restrict__ large, Levels lv, u64 cap,
                                                              unsigned short* __restrict__ out) {
    __shared__ u32 hist[MAX_LEVELS][256];
    __shared__ u32 hi_bin[MAX_LEVELS];
    __shared__ u64 sub_rank[MAX_LEVELS];  // the rank among the values of the level's high byte
    const u32 label = large[blockIdx.x];
    const u64 start = cursor[label - 1], end = cursor[label], m = end - start;
    if (end <= start || end > cap) return;  // (workgroup-uniform; cap: as in the gather)
    // [start, head) and [tail, end) value by value, [head, tail) in 16-byte loads of 8 values (vals is 16-byte aligned)
    const u64 head = std::min<u64>(end, (start + 7) & ~(u64)7), tail = std::max<u64>(head, end & ~(u64)7);
    const int t = threadIdx.x;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = t; i < MAX_LEVELS * 256; i += 256) (&hist[0][0])[i] = 0;
        __syncthreads();
        if (start + t < head) hist_value(hist, pass, hi_bin, lv.n, vals[start + t]);
        if (tail + t < end) hist_value(hist, pass, hi_bin, lv.n, vals[tail + t]);
        for (u64 i = head + (u64)t * 8; i < tail; i += 256 * 8) {
            const u32x4_t u = *reinterpret_cast<const u32x4_t*>(vals + i);
            const u32 w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hist_value(hist, pass, hi_bin, lv.n, w[k] & 0xffffu);
                hist_value(hist, pass, hi_bin, lv.n, w[k] >> 16);
            }
        }
        __syncthreads();
        if (t < lv.n) {  // the bin that holds the rank: 256 steps of one thread per level
            const u64 rank = pass == 0 ? ((u64)lv.p[t] * (m - 1)) / 100u : sub_rank[t];
            const u32* h = hist[pass == 0 ? 0 : t];
            u64 below = 0;
            u32 bin = 0;
            while (bin < 255 && rank >= below + h[bin]) below += h[bin++];
            if (pass == 0) {
                hi_bin[t] = bin;
                sub_rank[t] = rank - below;
            } else {
                out[(u64)label * lv.n + t] = (unsigned short)((hi_bin[t] << 8) | bin);
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int dlv_cc_quantiles_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint16_t* raw_dev, int Z, int Y, int X,
                                    int64_t raw_pitch_y, int64_t raw_pitch_z, uint64_t n, int n_levels, const int* levels,
                                    uint16_t* out, uint32_t* counts) {
    if (!ctx || !labels_dev || !raw_dev || !levels || !out || !counts) return DLV_EINVAL;
    DLV_TRY(check_volume(ctx, "cc_quantiles", Z, Y, X));
    DLV_TRY(check_raw_pitches(ctx, "cc_quantiles", Y, X, raw_pitch_y, raw_pitch_z));
    DLV_TRY(check_label_count(ctx, "cc_quantiles", n));
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)raw_dev & 1))
        return dlv_fail(ctx, DLV_EINVAL, "cc_quantiles: labels must be 4-byte aligned, raw 2-byte aligned");
    if (n_levels < 1 || n_levels > MAX_LEVELS) return dlv_fail(ctx, DLV_EINVAL, "cc_quantiles: %d levels, expected 1..%d", n_levels, MAX_LEVELS);
    Levels lv = {n_levels, {0}};
    for (int i = 0; i < n_levels; ++i) {
        if (levels[i] < 0 || levels[i] > 100 || (i > 0 && levels[i] <= levels[i - 1]))
            return dlv_fail(ctx, DLV_EINVAL, "cc_quantiles: level %d = %d: expected per cent 0..100, strictly increasing", i, levels[i]);
        lv.p[i] = levels[i];
    }
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rows = (size_t)n + 1;
    const u64 nvox = (u64)Z * Y * X;
    // 1. the counts (4 bytes per label), then their exclusive prefix sum: start[l] = the voxels of the labels 1..l-1
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, rows * 4, (void**)&ws));
    DLV_TRY(dlv_cc_counts_dev(ctx, labels_dev, nvox, n, (u32*)ws));
    std::vector<u32> host_counts(rows);
    DLV_HIP(ctx, hipMemcpyAsync(host_counts.data(), ws, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    host_counts[0] = 0;  // (the background is not measured)
    std::vector<u64> start(rows);
    std::vector<u32> large;
    u64 fg = 0;
    for (size_t l = 0; l < rows; ++l) {
        start[l] = fg;
        fg += host_counts[l];
        if (host_counts[l] > SMALL_MAX) large.push_back((u32)l);
    }
    std::vector<uint16_t> host_out(rows * (size_t)n_levels, 0);
    if (fg > 0) {
        // [cursors u64 rows | labels of the long segments u32 | result u16 rows x levels | values u16 fg], each part on a 16-byte boundary
        const auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        const size_t off_large = up16(rows * 8), off_out = off_large + up16(large.size() * 4);
        const size_t off_vals = off_out + up16(host_out.size() * 2), bytes = off_vals + (size_t)fg * 2;
        const int rc = dlv_ws_get(ctx, WS_MISC, bytes, (void**)&ws);
        if (rc != DLV_OK && rc != DLV_ENOMEM) return rc;
        if (rc == DLV_ENOMEM)
            return dlv_fail(ctx, DLV_ENOMEM, "cc_quantiles: %llu foreground voxels of %zu labels need %zu bytes of scratch (2 per voxel, %zu for the "
                            "labels): not available", (unsigned long long)fg, rows - 1, bytes, off_vals);
        u64* cursor = (u64*)ws;
        unsigned short* out_dev = (unsigned short*)(ws + off_out);
        unsigned short* vals = (unsigned short*)(ws + off_vals);
        DLV_HIP(ctx, hipMemcpyAsync(cursor, start.data(), rows * 8, hipMemcpyHostToDevice, ctx->stream));
        if (!large.empty())
            DLV_HIP(ctx, hipMemcpyAsync(ws + off_large, large.data(), large.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        DLV_HIP(ctx, hipMemsetAsync(out_dev, 0, host_out.size() * 2, ctx->stream));
        // 2. gather
        const int gs = (int)std::min<u64>((u64)Z * Y, (u64)256 * 32);
        DlvProf pg(ctx, "cc_quantiles_gather", 0.0, (double)nvox * 6 + (double)fg * 2);
        hipLaunchKernelGGL(cc_gather_kernel, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, raw_dev, Z, Y, X, (long long)raw_pitch_y,
                           (long long)raw_pitch_z, (u32)n, cursor, vals, fg);
        pg.end();
        DLV_LAUNCH_CHECK(ctx, "cc_gather_kernel");
        // 3. select
        DlvProf ps(ctx, "cc_quantiles_select", 0.0, (double)fg * 2 + (double)rows * 8);
        hipLaunchKernelGGL(cc_select_small_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, vals, cursor, (u32)n, lv, fg, out_dev);
        if (!large.empty())
            hipLaunchKernelGGL(cc_select_large_kernel, dim3((unsigned)large.size()), dim3(256), 0, ctx->stream, vals, cursor,
                               (const u32*)(ws + off_large), lv, fg, out_dev);
        ps.end();
        DLV_LAUNCH_CHECK(ctx, "cc_select kernels");
        DLV_HIP(ctx, hipMemcpyAsync(host_out.data(), out_dev, host_out.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
        DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    memcpy(out, host_out.data(), host_out.size() * 2);
    memcpy(counts, host_counts.data(), rows * 4);
    return DLV_OK;
}
