// cc_shape.hip - per-label shape accumulators of a label volume (dlv_cc_shape_dev): voxel count, first and second moments of
// the coordinates and the exposed faces per axis, from which hostlogic.finish_shape derives the principal-axis variances,
// elongation and sphericity of every cell.  The reference has no counterpart (its users take them on the host from the label
// file); the labels are in HBM at the end of count_blobs' labelling, so this is one pass over 4 bytes per voxel that reads the
// four neighbour rows only where a wave holds a cell.
//
// Integer work only (u32 counts, u64 sums): results are exact and independent of scheduling.  No overflow: a coordinate is at
// most 65535 (checked on entry), so a product of two is below 2^32, and a component has fewer than 2^32 voxels - every sum of
// coordinates or products stays below 2^64, and so does a face count (at most 2 per voxel and axis).
//
// Measured once on an MI355X (profiles/README.md, "cc_shape"): 512^3 labels, 1.48 ms on a 1 % mask of small cells and 37.8 ms on a
// 50 % random mask (one giant component: bound by the atomics on its row), 0.46 and 0.78 of cc_stats_kernel on the same labels.
#include "common.h"
#include "cc_check.h"
#include "cc_fold.h"

#include <algorithm>

namespace {

// a (thread's, then a wave's) voxels under one label: z and y are the row's, so only x is summed here
struct ShapeAcc {
    u32 c_sv;   // count | surface voxels << 16  (<= 512 per wave: 16 bits each)
    u32 fz_fy;  // exposed faces along z | along y << 16  (<= 1024 per wave and axis)
    u32 fx;
    u32 sx;     // (<= 512 * 65535 per wave: fits 32 bits)
    u64 sxx;
    static __device__ __forceinline__ ShapeAcc none() { return {0u, 0u, 0u, 0u, 0ull}; }
    __device__ __forceinline__ void combine(int o) {
        xor_add(c_sv, o); xor_add(fz_fy, o); xor_add(fx, o);
        xor_add(sx, o); xor_add(sxx, o);
    }
};

// The sweep layout and the aggregation of cc_fold.h over the rows (z, y) of the measured planes [z_first, z_first + nz) of the
// buffer.  A wave whose 512 voxels hold no label 1..n stops there.  One that holds a label reads the rows (z-1, y), (z+1, y),
// (z, y-1) and (z, y+1) at the same x - a row outside the buffer reads as NO_VOXEL, which differs from every label - and the
// two voxels next to each quad along x (the row is in the cache by then: plain loads, not nontemporal ones).  Per voxel: 2 bits
// of exposed faces per axis.  A thread folds count, sum x, sum x^2, the three face counts and the surface voxels over its voxels
// of equal label (its runs, also across the gap between the quads); the leader lane of a (wave, label) turns the seven values
// into the 14 sums and issues the atomics.  There is no workgroup barrier.
__global__ void __launch_bounds__(256) cc_shape_kernel(const u32* __restrict__ labels, int Zb, int Y, int X, int z_first, int nz,
                                                       u32 z_abs0, u32 n, u32* __restrict__ counts, u64* __restrict__ sums,
                                                       u64* __restrict__ moments, u64* __restrict__ faces,
                                                       u32* __restrict__ surface) {
    const u64 nrows = (u64)nz * Y;
    const u64 plane = (u64)Y * X;
    const int sweeps = row_sweeps(X);
    for (u64 r = blockIdx.x; r < nrows; r += gridDim.x) {
        const u32 z = (u32)z_first + (u32)(r / (u64)Y), y = (u32)(r % (u64)Y);  // (the buffer's own)
        const u32* lrow = labels + (u64)z * plane + (u64)y * X;
        const bool has_zm = z > 0, has_zp = z + 1 < (u32)Zb, has_ym = y > 0, has_yp = y + 1 < (u32)Y;
        const u64 za = (u64)z_abs0 + z, ya = y;  // (absolute coordinates, <= 65535)
        for (int sw = 0; sw < sweeps; ++sw) {
            u32 xq[2], l[VPT];
            quad_starts(sw, xq);
            load_quads<false>(lrow, true, xq, (u32)X, l);
            unsigned todo = fg_mask(l, n);    // the voxels that are not folded yet
            if (!__any(todo != 0)) continue;  // (wave-uniform) nothing to measure in this wave's 512 voxels
            u32 e[VPT];  // exposed faces of voxel k: z in bits 0-1, y in bits 2-3, x in bits 4-5
            {
                u32 a[VPT], b[VPT];
                load_quads<false>(has_zm ? lrow - plane : lrow, has_zm, xq, (u32)X, a);
                load_quads<false>(has_zp ? lrow + plane : lrow, has_zp, xq, (u32)X, b);
#pragma unroll
                for (int k = 0; k < VPT; ++k) e[k] = (a[k] != l[k] ? 1u : 0u) + (b[k] != l[k] ? 1u : 0u);
                load_quads<false>(has_ym ? lrow - X : lrow, has_ym, xq, (u32)X, a);
                load_quads<false>(has_yp ? lrow + X : lrow, has_yp, xq, (u32)X, b);
#pragma unroll
                for (int k = 0; k < VPT; ++k) e[k] |= ((a[k] != l[k] ? 1u : 0u) + (b[k] != l[k] ? 1u : 0u)) << 2;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    // the voxels before and after the quad (xq - 1 < X also keeps a quad past the row's end inside the row)
                    const u32 left = (xq[q] > 0 && xq[q] - 1u < (u32)X) ? lrow[xq[q] - 1u] : NO_VOXEL;
                    const u32 right = (xq[q] + 4u < (u32)X) ? lrow[xq[q] + 4u] : NO_VOXEL;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const u32 lo = j == 0 ? left : l[4 * q + j - 1], hi = j == 3 ? right : l[4 * q + j + 1];
                        e[4 * q + j] |= ((lo != l[4 * q + j] ? 1u : 0u) + (hi != l[4 * q + j] ? 1u : 0u)) << 4;
                    }
                }
            }
            // one pass per distinct label of the thread (one, as a rule)
            while (__any(todo != 0)) {
                const bool have = todo != 0;
                const u32 lab = first_label(l, todo);
                u32 c = 0, sx = 0, fz = 0, fy = 0, fx = 0, sv = 0;  // (<= 8, 8 * 65535, 16, 16, 16, 8)
                u64 sxx = 0;
#pragma unroll
                for (int k = 0; k < VPT; ++k) {
                    const bool in = ((todo >> k) & 1u) && l[k] == lab;
                    const u32 x = voxel_x(xq, k);  // (< X <= 65536 where `in`)
                    c += in ? 1u : 0u;
                    sx += in ? x : 0u;
                    sxx += in ? (u64)(x * x) : 0ull;  // (65535^2 < 2^32)
                    fz += in ? (e[k] & 3u) : 0u;
                    fy += in ? ((e[k] >> 2) & 3u) : 0u;
                    fx += in ? ((e[k] >> 4) & 3u) : 0u;
                    sv += (in && e[k] != 0) ? 1u : 0u;
                    todo &= ~((in ? 1u : 0u) << k);
                }
                const ShapeAcc own = {c | (sv << 16), fz | (fy << 16), fx, sx, sxx};
                wave_fold_by_label<true>(lab, have, own, [&](u32 L, const ShapeAcc& w) {
                    const u64 cnt = w.c_sv & 0xffffu, s = w.sx;
                    atomicAdd(counts + L, (u32)cnt);
                    u64* S = sums + 3ull * L;
                    atomicAdd(S + 0, cnt * za);
                    atomicAdd(S + 1, cnt * ya);
                    atomicAdd(S + 2, s);
                    u64* M = moments + 6ull * L;  // zz, yy, xx, zy, zx, yx
                    atomicAdd(M + 0, cnt * (za * za));
                    atomicAdd(M + 1, cnt * (ya * ya));
                    atomicAdd(M + 2, w.sxx);
                    atomicAdd(M + 3, cnt * (za * ya));
                    atomicAdd(M + 4, za * s);
                    atomicAdd(M + 5, ya * s);
                    // (the inside of a large component exposes nothing)
                    u64* F = faces + 3ull * L;
                    if (w.fz_fy & 0xffffu) atomicAdd(F + 0, (u64)(w.fz_fy & 0xffffu));
                    if (w.fz_fy >> 16) atomicAdd(F + 1, (u64)(w.fz_fy >> 16));
                    if (w.fx) atomicAdd(F + 2, (u64)w.fx);
                    if (w.c_sv >> 16) atomicAdd(surface + L, w.c_sv >> 16);
                });
            }
        }
    }
}

}  // namespace

extern "C" int dlv_cc_shape_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Zb, int Y, int X, int z_first, int nz, int z_abs0,
                                uint64_t n, uint32_t* counts, uint64_t* sums, uint64_t* moments, uint64_t* faces,
                                uint32_t* surface_voxels) {
    if (!ctx || !labels_dev || !counts || !sums || !moments || !faces || !surface_voxels) return DLV_EINVAL;
    DLV_TRY(check_volume(ctx, "cc_shape", Zb, Y, X));
    if (nz < 1 || z_first < 0 || (long long)z_first + nz > Zb || z_abs0 < 0)
        return dlv_fail(ctx, DLV_EINVAL, "cc_shape: planes [%d, %d + %d) at absolute z %d do not lie in a buffer of %d planes", z_first,
                        z_first, nz, z_abs0, Zb);
    DLV_TRY(check_label_count(ctx, "cc_shape", n));
    if ((uintptr_t)labels_dev & 3) return dlv_fail(ctx, DLV_EINVAL, "cc_shape: labels must be 4-byte aligned");
    if ((long long)z_abs0 + Zb > 65536 || Y > 65536 || X > 65536) return dlv_fail(ctx, DLV_EUNSUP, "bounding boxes are uint16");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rows = (size_t)n + 1;
    // device accumulators, each in its host layout: [sums u64 3*rows | moments u64 6*rows | faces u64 3*rows | counts u32 rows |
    // surface u32 rows]; an absent label keeps zeros
    const size_t off_mom = rows * 24, off_faces = rows * 72, off_counts = rows * 96, off_surf = rows * 100, bytes = rows * 104;
    char* ws;
    DLV_TRY(dlv_ws_get(ctx, WS_MISC, bytes, (void**)&ws));
    DLV_HIP(ctx, hipMemsetAsync(ws, 0, bytes, ctx->stream));
    const u64 nvox = (u64)nz * Y * X;
    const int gs = (int)std::min<u64>((u64)nz * Y, (u64)256 * 32);
    DlvProf pr(ctx, "cc_shape", 0.0, (double)nvox * 4);
    hipLaunchKernelGGL(cc_shape_kernel, dim3(gs), dim3(256), 0, ctx->stream, labels_dev, Zb, Y, X, z_first, nz, (u32)z_abs0, (u32)n,
                       (u32*)(ws + off_counts), (u64*)ws, (u64*)(ws + off_mom), (u64*)(ws + off_faces), (u32*)(ws + off_surf));
    pr.end();
    DLV_LAUNCH_CHECK(ctx, "cc_shape_kernel");
    DLV_HIP(ctx, hipMemcpyAsync(sums, ws, rows * 24, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(moments, ws + off_mom, rows * 48, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(faces, ws + off_faces, rows * 24, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(counts, ws + off_counts, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipMemcpyAsync(surface_voxels, ws + off_surf, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DLV_OK;
}
