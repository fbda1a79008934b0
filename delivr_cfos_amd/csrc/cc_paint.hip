// cc_paint.hip - blob painting from the labels (dlv_paint_labels_dev, dlv_paint_runs_dev): blob_highlighter with
// settings["mi355x"]["paint_from"] = "labels".  Replaces the loops of blob_highlighter.py:108-125 / :150-158 by what they are meant
// to draw: every voxel gets the value of the cell whose label it carries, out[v] = lut[label[v]], and 0 elsewhere - where paint.hip
// restates the loops as they are written (owner[v] = max{i+1 : box_i contains v}, times bin_img).  The labels are the dense uint32
// volume, or the run-length coding of cc_runs.hip: then the colour planes are written straight from the runs and the label volume
// is never built in HBM.  Two look-up tables indexed by label, either or both: uint32 r | g << 8 | b << 16 -> three uint8 planes,
// uint16 -> one uint16 plane; ONE pass over the labels or the runs writes every plane asked for (a template per combination).
// A label of 0 and a label >= n_lut write 0: the kernels clamp, they do not judge.
//
// Layout: cc_fold.h's row sweep with workgroups of ONE wave, as cc_runs.hip - a wave walks whole rows in sweeps of 512 voxels, a
// lane takes the quads [4l, 4l + 4) and [4(64 + l), 4(64 + l) + 4).  A lane's quad of one plane is ONE store: 32 bits of a byte
// plane, 64 bits of the uint16 plane (256 / 512 contiguous bytes per wave instruction), where the plane's row starts on that
// boundary and the quad lies inside the row - decided per row and per plane, since an odd X moves every row's alignment -, element
// by element elsewhere.  Every element of every output row has exactly one writer and is written once, zeros included: no atomics,
// no LDS, the planes need not be cleared, and the result is exact and independent of scheduling.  Integer work only.
// Run painter: a wave takes 64 consecutive rows at a time and reads their bounds in row_start with one load; every stretch of rows
// without a run - back to back in each plane - is filled with zeros by 16-byte stores in one go, without looking at the run
// arrays: on a cell mask that is most of the volume, and the case that decides the time.  In a row with runs a lane finds the last
// run that starts at or before its quad by bisection over the row's x0, as the decoder does; a quad wholly before the row's first
// run or after its last one skips the bisection.  Run indices are clamped to n_runs and only voxels x < X are written, whatever
// the arrays hold.
//
// Measured once on an MI355X (profiles/README.md, "cc_paint"): 512^3, RGB + uint16 planes, 1 % mask of small cells / 50 % random
// mask: from the runs 0.277 / 1.075 ms, from the labels 0.245 / 0.270 ms, the box path (paint.hip: owner + four applies) 1.130 /
// 1.659 ms.
#include "common.h"
#include "cc_fold.h"

#include <algorithm>

namespace {

constexpr int PT = 64;                  // threads per workgroup: one wave, one row at a time
constexpr u64 PAINT_MAX_WG = 256 * 32;  // workgroups per launch; rows beyond that are walked grid-stride

struct PaintArgs {
    u32 n_lut;  // (<= 0xffffffff: NO_VOXEL is never a valid index)
    const u32* __restrict__ lut_rgb;
    const unsigned short* __restrict__ lut_u16;
    uint8_t* __restrict__ r;
    uint8_t* __restrict__ g;
    uint8_t* __restrict__ b;
    unsigned short* __restrict__ u16;
};

// the output rows of one row of the volume and whether each starts on the boundary of its quad store
template <bool RGB, bool U16>
struct PaintRow {
    uint8_t *r, *g, *b;
    unsigned short* u16;
    bool vr, vg, vb, vu;
    __device__ __forceinline__ PaintRow(const PaintArgs& a, u64 off) {
        r = RGB ? a.r + off : nullptr;
        g = RGB ? a.g + off : nullptr;
        b = RGB ? a.b + off : nullptr;
        u16 = U16 ? a.u16 + off : nullptr;
        vr = (reinterpret_cast<uintptr_t>(r) & 3) == 0;
        vg = (reinterpret_cast<uintptr_t>(g) & 3) == 0;
        vb = (reinterpret_cast<uintptr_t>(b) & 3) == 0;
        vu = (reinterpret_cast<uintptr_t>(u16) & 7) == 0;
    }
};

// four bytes (packed, voxel j in bits 8j..) at x .. x + 3 of a byte row
__device__ __forceinline__ void store_quad_u8(uint8_t* __restrict__ row, bool vec, u32 x, u32 X, u32 packed) {
    if (vec && x + 4u <= X) {
        __builtin_nontemporal_store(packed, reinterpret_cast<u32*>(row + x));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + (u32)j < X) row[x + j] = (uint8_t)(packed >> (8 * j));
    }
}

// four uint16 (voxels 0, 1 in lo, 2, 3 in hi) at x .. x + 3 of a uint16 row
__device__ __forceinline__ void store_quad_u16(unsigned short* __restrict__ row, bool vec, u32 x, u32 X, u32 lo, u32 hi) {
    if (vec && x + 4u <= X) {
        const u32x2_t u = {lo, hi};
        __builtin_nontemporal_store(u, reinterpret_cast<u32x2_t*>(row + x));
    } else {
        if (x < X) row[x] = (unsigned short)lo;
        if (x + 1u < X) row[x + 1] = (unsigned short)(lo >> 16);
        if (x + 2u < X) row[x + 2] = (unsigned short)hi;
        if (x + 3u < X) row[x + 3] = (unsigned short)(hi >> 16);
    }
}

// the quad at x of every plane from its four labels (NO_VOXEL past the row's end: looked up as 0, not stored)
template <bool RGB, bool U16>
__device__ __forceinline__ void paint_quad(const PaintArgs& a, const PaintRow<RGB, U16>& o, u32 x, u32 X, const u32 (&lab)[4]) {
    u32 pr = 0, pg = 0, pb = 0, lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = lab[j] != 0 && lab[j] < a.n_lut;
        if (RGB) {
            const u32 c = ok ? a.lut_rgb[lab[j]] : 0u;
            pr |= (c & 0xffu) << (8 * j);
            pg |= ((c >> 8) & 0xffu) << (8 * j);
            pb |= ((c >> 16) & 0xffu) << (8 * j);
        }
        if (U16) {
            const u32 w = ok ? (u32)a.lut_u16[lab[j]] : 0u;
            if (j < 2) lo |= w << (16 * j);
            else hi |= w << (16 * (j - 2));
        }
    }
    if (RGB) {
        store_quad_u8(o.r, o.vr, x, X, pr);
        store_quad_u8(o.g, o.vg, x, X, pg);
        store_quad_u8(o.b, o.vb, x, X, pb);
    }
    if (U16) store_quad_u16(o.u16, o.vu, x, X, lo, hi);
}

// n bytes of zeros at p by one wave: bytes up to the first 16-byte boundary, 16-byte stores, bytes after the last boundary
__device__ __forceinline__ void zero_bytes(uint8_t* __restrict__ p, u64 n) {
    const u32 lane = threadIdx.x & 63;
    const u64 head = min(n, (u64)((16u - (u32)(reinterpret_cast<uintptr_t>(p) & 15)) & 15u));
    if (lane < head) p[lane] = 0;
    p += head;
    n -= head;
    const u64 nvec = n >> 4;
    const u32x4_t z = {0u, 0u, 0u, 0u};
    for (u64 i = lane; i < nvec; i += 64) __builtin_nontemporal_store(z, reinterpret_cast<u32x4_t*>(p) + i);
    if (lane < (n & 15)) p[(nvec << 4) + lane] = 0;
}

// ---- dense: out[v] = lut[labels[v]] ------------------------------------------------------------------------------------------------
template <bool RGB, bool U16>
__global__ void __launch_bounds__(PT) paint_labels_kernel(const u32* __restrict__ labels, u64 nrows, int X, PaintArgs a) {
    const int sweeps = row_sweeps(X);
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u32* row = labels + r * (u64)X;
        const PaintRow<RGB, U16> o(a, r * (u64)X);
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2], l[VPT];
            quad_starts(sw, xq);
            load_quads<true>(row, true, xq, (u32)X, l);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (xq[q] >= (u32)X) continue;
                const u32 lab[4] = {l[4 * q], l[4 * q + 1], l[4 * q + 2], l[4 * q + 3]};
                paint_quad<RGB, U16>(a, o, xq[q], (u32)X, lab);
            }
        }
    }
}

// ---- from the runs: rows [0, n_rows), every element written once -------------------------------------------------------------------
// The runs of row r are [row_start[r] - row_start[0], row_start[r + 1] - row_start[0]) of the arrays, clamped to n_runs (the
// decoder's addressing, cc_runs.hip).

// one row with the runs [b, e) (b < e)
template <bool RGB, bool U16>
__device__ __forceinline__ void paint_run_row(const PaintArgs& a, u64 r, int X, const unsigned short* __restrict__ x0,
                                              const unsigned short* __restrict__ x1, const u32* __restrict__ label, u64 b, u64 e) {
    const int sweeps = row_sweeps(X);
    const PaintRow<RGB, U16> o(a, r * (u64)X);
    const u32 first_x = x0[b], last_x = x1[e - 1];  // (the runs of a row are ordered: nothing before, nothing after)
    for (int sw = 0; sw < sweeps; ++sw) {
        u32 xq[2];
        quad_starts(sw, xq);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (xq[q] >= (u32)X) continue;
            u32 v[4] = {0u, 0u, 0u, 0u};
            if (xq[q] + 3u >= first_x && xq[q] <= last_x) {
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
            paint_quad<RGB, U16>(a, o, xq[q], (u32)X, v);
        }
    }
}

// A wave takes RB = 64 consecutive rows at a time: lane i reads the bounds of row i (one coalesced load for the wave, none per
// row), a ballot tells the rows that hold runs, and every stretch of rows without one - they lie back to back in each plane - is
// filled with zeros in one go, without looking at the run arrays: on a cell mask that is most of the volume.
constexpr int RB = 64;
template <bool RGB, bool U16>
__global__ void __launch_bounds__(PT) paint_runs_kernel(const u64* __restrict__ row_start, u64 n_rows, int X,
                                                        const unsigned short* __restrict__ x0, const unsigned short* __restrict__ x1,
                                                        const u32* __restrict__ label, u64 n_runs, PaintArgs a) {
    const u32 lane = threadIdx.x & 63;
    const u64 origin = row_start[0];
    for (u64 base = (u64)blockIdx.x * RB; base < n_rows; base += (u64)gridDim.x * RB) {
        const u64 mine = min(base + lane, n_rows - 1);  // (row_start holds n_rows + 1 entries)
        const u64 b = min(row_start[mine] - origin, n_runs), e = min(max(row_start[mine + 1] - origin, b), n_runs);
        const int cnt = (int)min((u64)RB, n_rows - base);
        const u64 with_runs = __ballot((int)lane < cnt && e > b);  // bit i: row base + i holds a run
        int i = 0;
        while (i < cnt) {  // (wave-uniform throughout)
            const u64 rest = with_runs >> i;
            const int j = rest ? i + __ffsll((long long)rest) - 1 : cnt;  // the rows [i, j) hold no run, row j < cnt does
            if (j > i) {
                const u64 off = (base + (u64)i) * (u64)X, n = (u64)(j - i) * (u64)X;
                if (RGB) {
                    zero_bytes(a.r + off, n);
                    zero_bytes(a.g + off, n);
                    zero_bytes(a.b + off, n);
                }
                if (U16) zero_bytes(reinterpret_cast<uint8_t*>(a.u16 + off), 2ull * n);
            }
            if (j < cnt) paint_run_row<RGB, U16>(a, base + (u64)j, X, x0, x1, label, shfl64(b, j), shfl64(e, j));
            i = j + 1;
        }
    }
}

unsigned paint_grid(u64 nrows) { return (unsigned)std::min<u64>(nrows, PAINT_MAX_WG); }
unsigned paint_runs_grid(u64 nrows) { return (unsigned)std::min<u64>((nrows + RB - 1) / RB, PAINT_MAX_WG); }

// the look-up description both entry points share -> a (wanted planes: 1 RGB, 2 uint16) or DLV_EINVAL
int paint_args(dlv_ctx* ctx, const char* what, uint64_t n_lut, const uint32_t* lut_rgb, const uint16_t* lut_u16, uint8_t* out_r,
               uint8_t* out_g, uint8_t* out_b, uint16_t* out_u16, PaintArgs* a, int* planes) {
    const int n_rgb_out = (out_r ? 1 : 0) + (out_g ? 1 : 0) + (out_b ? 1 : 0);
    if (n_lut < 1) return dlv_fail(ctx, DLV_EINVAL, "%s: an empty look-up table (entry 0 is the background)", what);
    if (!lut_rgb && !lut_u16) return dlv_fail(ctx, DLV_EINVAL, "%s: neither the RGB nor the uint16 look-up table is given", what);
    if (n_rgb_out != (lut_rgb ? 3 : 0))
        return dlv_fail(ctx, DLV_EINVAL, "%s: the RGB table goes with all three byte planes and they with it (%d given)", what, n_rgb_out);
    if ((lut_u16 != nullptr) != (out_u16 != nullptr))
        return dlv_fail(ctx, DLV_EINVAL, "%s: the uint16 table goes with the uint16 plane and it with the table", what);
    if (((uintptr_t)lut_rgb & 3) || ((uintptr_t)lut_u16 & 1) || ((uintptr_t)out_u16 & 1))
        return dlv_fail(ctx, DLV_EINVAL, "%s: a pointer is not aligned to its element", what);
    a->n_lut = (u32)std::min<uint64_t>(n_lut, 0xffffffffull);
    a->lut_rgb = lut_rgb;
    a->lut_u16 = lut_u16;
    a->r = out_r;
    a->g = out_g;
    a->b = out_b;
    a->u16 = out_u16;
    *planes = (lut_rgb ? 1 : 0) | (lut_u16 ? 2 : 0);
    return DLV_OK;
}

double paint_out_bytes(int planes) { return ((planes & 1) ? 3.0 : 0.0) + ((planes & 2) ? 2.0 : 0.0); }

}  // namespace

extern "C" {

int dlv_paint_labels_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n_lut, const uint32_t* lut_rgb_dev,
                         const uint16_t* lut_u16_dev, uint8_t* out_r, uint8_t* out_g, uint8_t* out_b, uint16_t* out_u16) {
    if (!ctx || !labels_dev) return DLV_EINVAL;
    if (Z < 1 || Y < 1 || X < 1) return dlv_fail(ctx, DLV_EINVAL, "paint_labels: empty volume");
    if ((uintptr_t)labels_dev & 3) return dlv_fail(ctx, DLV_EINVAL, "paint_labels: a pointer is not aligned to its element");
    PaintArgs a;
    int planes;
    DLV_TRY(paint_args(ctx, "paint_labels", n_lut, lut_rgb_dev, lut_u16_dev, out_r, out_g, out_b, out_u16, &a, &planes));
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nrows = (u64)Z * Y;
    const dim3 grid(paint_grid(nrows)), block(PT);
    DlvProf pr(ctx, "paint_labels", 0.0, (double)nrows * X * (4.0 + paint_out_bytes(planes)));
    if (planes == 3) hipLaunchKernelGGL((paint_labels_kernel<true, true>), grid, block, 0, ctx->stream, labels_dev, nrows, X, a);
    else if (planes == 1) hipLaunchKernelGGL((paint_labels_kernel<true, false>), grid, block, 0, ctx->stream, labels_dev, nrows, X, a);
    else hipLaunchKernelGGL((paint_labels_kernel<false, true>), grid, block, 0, ctx->stream, labels_dev, nrows, X, a);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "paint_labels_kernel");
    return DLV_OK;
}

int dlv_paint_runs_dev(dlv_ctx* ctx, const uint64_t* row_start_dev, uint64_t n_rows, int X, const uint16_t* x0_dev,
                       const uint16_t* x1_dev, const uint32_t* label_dev, uint64_t n_runs, uint64_t n_lut, const uint32_t* lut_rgb_dev,
                       const uint16_t* lut_u16_dev, uint8_t* out_r, uint8_t* out_g, uint8_t* out_b, uint16_t* out_u16) {
    if (!ctx || !row_start_dev) return DLV_EINVAL;
    if (n_runs && (!x0_dev || !x1_dev || !label_dev)) return DLV_EINVAL;
    if (n_rows < 1 || X < 1) return dlv_fail(ctx, DLV_EINVAL, "paint_runs: empty volume");
    if (X > 65536) return dlv_fail(ctx, DLV_EUNSUP, "paint_runs: X = %d, x0 / x1 are uint16", X);
    if (((uintptr_t)row_start_dev & 7) || ((uintptr_t)x0_dev & 1) || ((uintptr_t)x1_dev & 1) || ((uintptr_t)label_dev & 3))
        return dlv_fail(ctx, DLV_EINVAL, "paint_runs: a pointer is not aligned to its element");
    PaintArgs a;
    int planes;
    DLV_TRY(paint_args(ctx, "paint_runs", n_lut, lut_rgb_dev, lut_u16_dev, out_r, out_g, out_b, out_u16, &a, &planes));
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid(paint_runs_grid(n_rows)), block(PT);
    DlvProf pr(ctx, "paint_runs", 0.0, (double)n_rows * (8.0 + X * paint_out_bytes(planes)) + (double)n_runs * 8);
    if (planes == 3)
        hipLaunchKernelGGL((paint_runs_kernel<true, true>), grid, block, 0, ctx->stream, (const u64*)row_start_dev, (u64)n_rows, X, x0_dev,
                           x1_dev, label_dev, (u64)n_runs, a);
    else if (planes == 1)
        hipLaunchKernelGGL((paint_runs_kernel<true, false>), grid, block, 0, ctx->stream, (const u64*)row_start_dev, (u64)n_rows, X, x0_dev,
                           x1_dev, label_dev, (u64)n_runs, a);
    else
        hipLaunchKernelGGL((paint_runs_kernel<false, true>), grid, block, 0, ctx->stream, (const u64*)row_start_dev, (u64)n_rows, X, x0_dev,
                           x1_dev, label_dev, (u64)n_runs, a);
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "paint_runs_kernel");
    return DLV_OK;
}

}  // extern "C"
