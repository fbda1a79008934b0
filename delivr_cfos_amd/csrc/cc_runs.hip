// cc_runs.hip - the run-length coding of a label volume on the device (dlv_cc_runs_count_dev, dlv_cc_runs_emit_dev) and its
// decoder (dlv_cc_runs_decode_dev): the payload of count_blobs' <brain>-<N>-cc3d.runs file (label_runs.py holds the format and
// the numpy reference).  A run is a maximal stretch of one non-zero label inside a row (z, y); per row the runs are counted, the
// counts are scanned into row_start, and every run's first x, last x and label are written at row_start[row] + its rank in the row.
// The reference has no counterpart: it writes the dense volume.  The labels are in HBM at the end of count_blobs' labelling, so the
// coder reads them twice (count, emit: 8 bytes per voxel) and writes 8 bytes per run; the decoder reads the runs of a row where the
// row has any and writes every voxel of the volume once, zeros included (4 bytes per voxel).
//
// Layout: cc_fold.h's row sweep with workgroups of ONE wave - a wave walks whole rows in sweeps of 512 voxels, so that the number of
// runs before a voxel is a wave scan plus a count carried from sweep to sweep in a register: no LDS, no barrier, no atomic.  The
// k-th start and the k-th end of a row belong to the same run, so a run's end finds its place from the starts alone: it is the
// (starts up to and including its voxel) - 1.
//
// Integer work only, every output element has one writer: results are exact and independent of scheduling.  No overflow: a row has
// at most X <= 65536 runs (checked on entry), so a row's count and its ranks fit 32 bits with room, a scan group of 1024 rows
// holds at most 2^26 runs, and everything above a group - the group sums, row_start and the total - is 64 bits; x0 and x1 are at
// most 65535.  The emitter and the decoder check every run index against n_runs, and the decoder writes inside the row only,
// whatever the run arrays hold.
//
// Measured once on an MI355X (profiles/README.md, "cc_runs"): 512^3 labels, count + scan + emit 0.226 ms on a 1 % mask of small
// cells (671 008 runs; 0.069 of cc_stats_kernel on the same labels, against the bound of 2) and 0.355 ms on a 50 % random mask
// (33.6 million runs); the decode 0.313 and 0.603 ms.  1024 x 2048 x 2048, the bench's cell mask: 7 ms with the download of the runs.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"
#include "dev_scan.h"

#include <algorithm>

namespace {

constexpr int RT = 64;                 // threads per workgroup: one wave, one row at a time
constexpr u64 RUNS_MAX_WG = 256 * 32;  // workgroups per launch; rows beyond that are walked grid-stride

// The labels of this lane's two quads of sweep sw and the voxel before / after each quad (NO_VOXEL outside the row: it differs
// from every label, so a row's first voxel starts a run and its last one ends one).  The neighbours come from the lanes next to
// this one; lane 0 / lane 63 read theirs from memory.  Returns false - for the whole wave - where the sweep holds no label.
template <bool NT>
__device__ __forceinline__ bool load_sweep(const u32* __restrict__ row, u32 X, int sw, u32 (&xq)[2], u32 (&l)[VPT], u32 (&left)[2],
                                           u32 (&right)[2]) {
    const int lane = threadIdx.x & 63;
    quad_starts(sw, xq);
    load_quads<NT>(row, true, xq, X, l);
    bool fg = false;
#pragma unroll
    for (int k = 0; k < VPT; ++k) fg |= l[k] != 0 && l[k] != NO_VOXEL;
    if (!__any(fg)) return false;  // (wave-uniform)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const u32 up = __shfl_up(l[4 * q + 3], 1, 64), down = __shfl_down(l[4 * q], 1, 64);
        left[q] = up;
        right[q] = down;
        // (xq - 1 < X also keeps a quad past the row's end inside the row)
        if (lane == 0) left[q] = (xq[q] > 0 && xq[q] - 1u < X) ? row[xq[q] - 1u] : NO_VOXEL;
        if (lane == 63) right[q] = (xq[q] + 4u < X) ? row[xq[q] + 4u] : NO_VOXEL;
    }
    return true;
}

// bit k: voxel k starts a run / ends a run
__device__ __forceinline__ void run_flags(const u32 (&xq)[2], u32 X, const u32 (&l)[VPT], const u32 (&left)[2], const u32 (&right)[2],
                                          unsigned& starts, unsigned& ends) {
    starts = ends = 0;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int q = k >> 2, j = k & 3;
        const bool in = voxel_x(xq, k) < X && l[k] != 0;
        const u32 before = j == 0 ? left[q] : l[k - 1], after = j == 3 ? right[q] : l[k + 1];
        starts |= ((in && l[k] != before) ? 1u : 0u) << k;
        ends |= ((in && l[k] != after) ? 1u : 0u) << k;
    }
}

// ---- count: counts[row] = the runs of the row --------------------------------------------------------------------------------
__global__ void __launch_bounds__(RT) cc_runs_count_kernel(const u32* __restrict__ labels, u64 nrows, int X, u32* __restrict__ counts) {
    const int sweeps = row_sweeps(X);
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u32* row = labels + r * (u64)X;
        u32 c = 0;  // (<= 8 per sweep and lane)
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2], l[VPT], left[2], right[2];
            if (!load_sweep<true>(row, (u32)X, sw, xq, l, left, right)) continue;
            unsigned starts, ends;
            run_flags(xq, (u32)X, l, left, right, starts, ends);
            c += (u32)__popc(starts);
        }
        for (int o = 32; o > 0; o >>= 1) xor_add(c, o);
        if ((threadIdx.x & 63) == 0) counts[r] = c;
    }
}

// ---- emit: x0 / label at every start, x1 at every end, at row_start[row] + the run's rank in the row --------------------------
// A sweep lays the lanes' first quads before their second quads along x, so the starts before a voxel are: those of the sweeps
// before (carry), those of the quads before its quad (one wave scan of both quads' counts, 16 bits each: <= 256 per sweep) and
// those before it in its quad.
__global__ void __launch_bounds__(RT) cc_runs_emit_kernel(const u32* __restrict__ labels, u64 nrows, int X,
                                                          const u64* __restrict__ row_start, u64 n_runs, unsigned short* __restrict__ x0,
                                                          unsigned short* __restrict__ x1, u32* __restrict__ label) {
    const int lane = threadIdx.x & 63;
    const int sweeps = row_sweeps(X);
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u64 first = row_start[r];
        if (row_start[r + 1] == first) continue;  // (wave-uniform) a row without a run
        const u32* row = labels + r * (u64)X;
        u32 carry = 0;  // the starts of the sweeps before this one (<= X)
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2], l[VPT], left[2], right[2];
            if (!load_sweep<true>(row, (u32)X, sw, xq, l, left, right)) continue;
            unsigned starts, ends;
            run_flags(xq, (u32)X, l, left, right, starts, ends);
            const u32 own = (u32)__popc(starts & 0xfu) | ((u32)__popc(starts >> 4) << 16);
            u32 incl = own;
            for (int o = 1; o < 64; o <<= 1) {
                const u32 t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            const u32 total = __shfl(incl, 63, 64), excl = incl - own;
            u32 rank[2] = {carry + (excl & 0xffffu), carry + (total & 0xffffu) + (excl >> 16)};
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                const int q = k >> 2;
                if ((starts >> k) & 1u) {
                    const u64 at = first + rank[q];
                    if (at < n_runs) {
                        x0[at] = (unsigned short)voxel_x(xq, k);
                        label[at] = l[k];
                    }
                    ++rank[q];
                }
                if ((ends >> k) & 1u) {  // (its run's start is counted by now: rank >= 1)
                    const u64 at = first + rank[q] - 1u;
                    if (rank[q] > 0 && at < n_runs) x1[at] = (unsigned short)voxel_x(xq, k);
                }
            }
            carry += (total & 0xffffu) + (total >> 16);
        }
    }
}

// ---- decode: every voxel of rows [0, n_rows) written once ------------------------------------------------------------------------
// The runs of row r are [row_start[r] - row_start[0], row_start[r + 1] - row_start[0]) of the arrays, clamped to n_runs.  A lane
// finds the last run that starts at or before its quad's first voxel by bisection over the row's x0 and steps on from there: a
// voxel holds that run's label up to its x1 and 0 elsewhere.  Only voxels x < X are looked at, so a run is clamped to the row.
__global__ void __launch_bounds__(RT) cc_runs_decode_kernel(const u64* __restrict__ row_start, u64 n_rows, int X,
                                                            const unsigned short* __restrict__ x0, const unsigned short* __restrict__ x1,
                                                            const u32* __restrict__ label, u64 n_runs, u32* __restrict__ out) {
    const int sweeps = row_sweeps(X);
    const u64 origin = row_start[0];
    for (u64 r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const u64 b = min(row_start[r] - origin, n_runs), e = min(max(row_start[r + 1] - origin, b), n_runs);
        u32* orow = out + r * (u64)X;
        const bool vec = (reinterpret_cast<uintptr_t>(orow) & 15) == 0;
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2];
            quad_starts(sw, xq);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (xq[q] >= (u32)X) continue;
                u32 v[4] = {0u, 0u, 0u, 0u};
                if (e > b) {
                    u64 lo = b, hi = e;  // the runs [b, lo) start at or before xq, the runs [hi, e) after it
                    while (lo < hi) {
                        const u64 mid = lo + ((hi - lo) >> 1);
                        if ((u32)x0[mid] <= xq[q]) lo = mid + 1;
                        else hi = mid;
                    }
                    u64 cur = lo;  // the run of the voxel is cur - 1 (none yet: cur == b)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const u32 x = xq[q] + (u32)j;
                        if (cur < e && (u32)x0[cur] <= x) ++cur;
                        if (cur > b && x <= (u32)x1[cur - 1]) v[j] = label[cur - 1];
                    }
                }
                if (vec && xq[q] + 4u <= (u32)X) {
                    const u32x4_t u = {v[0], v[1], v[2], v[3]};
                    __builtin_nontemporal_store(u, reinterpret_cast<u32x4_t*>(orow + xq[q]));
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (xq[q] + (u32)j < (u32)X) orow[xq[q] + j] = v[j];
                }
            }
        }
    }
}

int runs_geometry(dlv_ctx* ctx, const char* what, int Z, int Y, int X) {
    DLV_TRY(check_volume(ctx, what, Z, Y, X));
    if (X > 65536) return dlv_fail(ctx, DLV_EUNSUP, "%s: X = %d, x0 / x1 are uint16", what, X);
    return DLV_OK;
}

unsigned runs_grid(u64 nrows) { return (unsigned)std::min<u64>(nrows, RUNS_MAX_WG); }

}  // namespace

extern "C" {

int dlv_cc_runs_count_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t* row_start_dev, uint64_t* n_runs) {
    if (!ctx || !labels_dev || !row_start_dev || !n_runs) return DLV_EINVAL;
    DLV_TRY(runs_geometry(ctx, "cc_runs_count", Z, Y, X));
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)row_start_dev & 7))
        return dlv_fail(ctx, DLV_EINVAL, "cc_runs_count: labels must be 4-byte, row_start 8-byte aligned");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nrows = (u64)Z * Y;
    const u64 ng = scan_groups(nrows);  // (one workgroup per group in the scan)
    if (ng > 0x7fffffffull) return dlv_fail(ctx, DLV_EUNSUP, "cc_runs_count: %llu rows exceed the launch grid", (unsigned long long)nrows);
    // [counts u32 nrows | pad | group sums u64 ng]
    const size_t off_gsum = ((size_t)nrows * 4 + 7) & ~(size_t)7;
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, off_gsum + (size_t)ng * 8, (void**)&ws));
    u32* counts = (u32*)ws;
    u64* gsum = (u64*)(ws + off_gsum);
    DlvProf pr(ctx, "cc_runs_count", 0.0, (double)nrows * X * 4);
    hipLaunchKernelGGL(cc_runs_count_kernel, dim3(runs_grid(nrows)), dim3(RT), 0, ctx->stream, labels_dev, nrows, X, counts);
    // the counts into the 64-bit row_start: 32-bit sums inside a scan group of 1024 rows (<= 2^26 runs), nothing above a group in
    // 32 bits; row_start[nrows] = R (<= the voxels of the volume)
    DLV_TRY(dev_excl_scan(ctx, counts, nrows, (u64*)row_start_dev, gsum, (u64*)row_start_dev + nrows, "cc_runs_count_kernel"));
    pr.end();
    DLV_HIP(ctx, hipMemcpyAsync(n_runs, row_start_dev + nrows, 8, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DLV_OK;
}

int dlv_cc_runs_emit_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, const uint64_t* row_start_dev, uint64_t n_runs,
                         uint16_t* x0_dev, uint16_t* x1_dev, uint32_t* label_dev) {
    if (!ctx || !labels_dev || !row_start_dev) return DLV_EINVAL;
    if (n_runs && (!x0_dev || !x1_dev || !label_dev)) return DLV_EINVAL;
    DLV_TRY(runs_geometry(ctx, "cc_runs_emit", Z, Y, X));
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)row_start_dev & 7) || ((uintptr_t)x0_dev & 1) || ((uintptr_t)x1_dev & 1) ||
        ((uintptr_t)label_dev & 3))
        return dlv_fail(ctx, DLV_EINVAL, "cc_runs_emit: a pointer is not aligned to its element");
    if (n_runs == 0) return DLV_OK;  // (nothing to write)
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nrows = (u64)Z * Y;
    DlvProf pr(ctx, "cc_runs_emit", 0.0, (double)nrows * X * 4 + (double)n_runs * 8);
    hipLaunchKernelGGL(cc_runs_emit_kernel, dim3(runs_grid(nrows)), dim3(RT), 0, ctx->stream, labels_dev, nrows, X, (const u64*)row_start_dev,
                       (u64)n_runs, x0_dev, x1_dev, label_dev);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_runs_emit_kernel");
    return DLV_OK;
}

int dlv_cc_runs_decode_dev(dlv_ctx* ctx, const uint64_t* row_start_dev, uint64_t n_rows, int X, const uint16_t* x0_dev,
                           const uint16_t* x1_dev, const uint32_t* label_dev, uint64_t n_runs, uint32_t* labels_out_dev) {
    if (!ctx || !row_start_dev || !labels_out_dev) return DLV_EINVAL;
    if (n_runs && (!x0_dev || !x1_dev || !label_dev)) return DLV_EINVAL;
    if (n_rows < 1 || X < 1) return dlv_fail(ctx, DLV_EINVAL, "cc_runs_decode: empty volume");
    if (X > 65536) return dlv_fail(ctx, DLV_EUNSUP, "cc_runs_decode: X = %d, x0 / x1 are uint16", X);
    if (((uintptr_t)labels_out_dev & 3) || ((uintptr_t)row_start_dev & 7) || ((uintptr_t)x0_dev & 1) || ((uintptr_t)x1_dev & 1) ||
        ((uintptr_t)label_dev & 3))
        return dlv_fail(ctx, DLV_EINVAL, "cc_runs_decode: a pointer is not aligned to its element");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    DlvProf pr(ctx, "cc_runs_decode", 0.0, (double)n_rows * X * 4 + (double)n_runs * 8);
    hipLaunchKernelGGL(cc_runs_decode_kernel, dim3(runs_grid(n_rows)), dim3(RT), 0, ctx->stream, (const u64*)row_start_dev, (u64)n_rows, X,
                       x0_dev, x1_dev, label_dev, (u64)n_runs, labels_out_dev);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_runs_decode_kernel");
    return DLV_OK;
}

}  // extern "C"
