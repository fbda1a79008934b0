// cc_shell.hip - the background shell of every component of a label volume (dlv_cc_shell_dev): the labels are expanded into the
// background by `radius` synchronous steps of a 26-neighbourhood minimum, and the expanded voxels that were background - and
// that lie inside the tissue (raw != 0) - are the shell S.  dlv_cc_intensity_dev / dlv_cc_counts_dev on S then measure the
// tissue directly around every cell: the local background its own intensity is compared with.  The reference has no
// counterpart; its users dilate the cells on the host from the label file.
//
//   E_0 = L;  E_{k+1}(v) = E_k(v) where E_k(v) != 0, else the smallest non-zero E_k(u) over the 26 neighbours u of v inside the
//   volume (0 without one);  S(v) = E_r(v) where L(v) == 0 and raw(v) != 0, else 0.
//
// E_r(v) is the smallest label among the cells at the minimal Chebyshev distance from v (when that is <= r): it depends on the
// labels within distance r of v only, which is what lets a slab with r more planes on either side give the slab's exact S.
// Integer work only, one writer per output voxel, no atomics: the result is exact and independent of scheduling.
#include "common.h"
#include "cc_check.h"
#include "cc_tile.h"

#include <algorithm>

namespace {

constexpr u32 NONE = 0xffffffffu;  // background while the minimum is taken

__device__ __forceinline__ u32 min3(u32 a, u32 b, u32 c) { return min(a, min(b, c)); }

// One expansion step: dst = E_{k+1} of src = E_k, or with FINAL the shell S of the last step.  A workgroup of 256 threads owns
// the TZ x TY x TX voxels at (blockIdx.z, .y, .x).  It stages them with their halo in LDS (cc_tile.h), 0 as NONE, voxels outside
// the volume as NONE.  A tile whose input is all background, halo included, writes nothing: its output is zero in dst already
// (the launcher's note).  Otherwise every thread takes quads of
// four voxels along x: for a quad that holds a background voxel it reads the 9 rows around it (6 values each: one 16-byte
// read and the two neighbours) and folds the 3 x 3 x 3 minima.  FINAL: only voxels that are background in `labels` (src itself
// when radius is 1) are kept, and only where raw is not 0; raw (NULL: no such condition) is read just for the quads that
// reached a label.
template <bool FINAL>
__global__ void __launch_bounds__(256) cc_shell_sweep_kernel(const u32* __restrict__ src, const u32* __restrict__ labels,
                                                             const unsigned short* __restrict__ raw, int Z, int Y, int X,
                                                             long long pitch_y, long long pitch_z, u32* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) u32 tile[ROWS * PITCH];
    const TileAt t(Z, Y, X);
    u32 seen = 0;
    for (int i = threadIdx.x; i < ROWS * QX; i += 256) {
        const int row = i / QX, q = i % QX;
        u32x4_t v = tile_quad_of(src, t, row, q);
        seen |= v.x | v.y | v.z | v.w;
        v.x = v.x ? v.x : NONE; v.y = v.y ? v.y : NONE; v.z = v.z ? v.z : NONE; v.w = v.w ? v.w : NONE;
        *reinterpret_cast<u32x4_t*>(tile + tile_word(row, q)) = v;
    }
    for (int i = threadIdx.x; i < ROWS * 2; i += 256) {
        const int row = i >> 1, right = i & 1;
        const int z = t.z0 - 1 + row / (TY + 2), y = t.y0 - 1 + row % (TY + 2), x = right ? t.x0 + TX : t.x0 - 1;
        u32 v = 0;
        if (z >= 0 && z < Z && y >= 0 && y < Y && x >= 0 && x < X) v = src[((u64)z * Y + y) * (u64)X + x];
        seen |= v;
        tile[row * PITCH + (right ? 4 + TX : 3)] = v ? v : NONE;
    }
    if (!__syncthreads_or(seen != 0)) return;  // (workgroup-uniform) nothing to expand into this tile

    for (int i = threadIdx.x; i < TZ * TY * QX; i += 256) {
        const int q = i % QX, oy = (i / QX) % TY, oz = i / (QX * TY);
        const int z = t.z0 + oz, y = t.y0 + oy, x = t.x0 + 4 * q;
        if (z >= Z || y >= Y || x >= X) continue;
        const u32x4_t cen = *reinterpret_cast<const u32x4_t*>(tile + tile_word(tile_row(oz, oy), q));
        u32 e[4] = {cen.x, cen.y, cen.z, cen.w};  // E_{k+1}, NONE for 0
        if (e[0] == NONE || e[1] == NONE || e[2] == NONE || e[3] == NONE) {
            u32 m[4] = {NONE, NONE, NONE, NONE};
#pragma unroll
            for (int dz = 0; dz < 3; ++dz)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const u32* r = tile + ((oz + dz) * (TY + 2) + oy + dy) * PITCH + 3 + 4 * q;
                    const u32 a = r[0], f = r[5];
                    const u32x4_t b = *reinterpret_cast<const u32x4_t*>(r + 1);
                    m[0] = min(m[0], min3(a, b.x, b.y));
                    m[1] = min(m[1], min3(b.x, b.y, b.z));
                    m[2] = min(m[2], min3(b.y, b.z, b.w));
                    m[3] = min(m[3], min3(b.z, b.w, f));
                }
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = e[j] == NONE ? m[j] : e[j];
        }
        u32 out[4];
        if (!FINAL) {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = e[j] == NONE ? 0u : e[j];
        } else {
            bool bg[4] = {cen.x == NONE, cen.y == NONE, cen.z == NONE, cen.w == NONE};  // background in L
            if (labels != src) {  // (uniform) radius > 1: src is E_{r-1}, the cells are in `labels`
                const u32x4_t l = tile_quad_of(labels, t, tile_row(oz, oy), q);  // (0 beyond the end of the row: not kept below)
                bg[0] = l.x == 0; bg[1] = l.y == 0; bg[2] = l.z == 0; bg[3] = l.w == 0;
            }
            bool keep[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) keep[j] = bg[j] && e[j] != NONE && x + j < X;
            if (raw && (keep[0] || keep[1] || keep[2] || keep[3])) {
                const unsigned short* p = raw + (u64)z * (u64)pitch_z + (u64)y * (u64)pitch_y + x;
                if (x + 4 <= X && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
                    const u32x2_t u = *reinterpret_cast<const u32x2_t*>(p);
                    keep[0] = keep[0] && (u.x & 0xffffu) != 0; keep[1] = keep[1] && (u.x >> 16) != 0;
                    keep[2] = keep[2] && (u.y & 0xffffu) != 0; keep[3] = keep[3] && (u.y >> 16) != 0;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) keep[j] = keep[j] && p[j] != 0;  // (keep[j] implies x + j < X: not read otherwise)
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = keep[j] ? e[j] : 0u;
        }
        tile_store_quad(dst + ((u64)z * Y + y) * (u64)X + x, x, X, u32x4_t{out[0], out[1], out[2], out[3]});
    }
}

}  // namespace

extern "C" int dlv_cc_shell_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint16_t* raw_dev, int Z, int Y, int X,
                                int64_t raw_pitch_y, int64_t raw_pitch_z, int radius, uint32_t* shell_dev, uint32_t* scratch_dev) {
    if (!ctx) return DLV_EINVAL;
    if (!labels_dev) return dlv_fail(ctx, DLV_EINVAL, "cc_shell: labels_dev is NULL");
    if (!shell_dev) return dlv_fail(ctx, DLV_EINVAL, "cc_shell: shell_dev is NULL");
    DLV_TRY(check_volume(ctx, "cc_shell", Z, Y, X));
    if (radius < 1 || radius > 16) return dlv_fail(ctx, DLV_EINVAL, "cc_shell: radius %d is outside 1..16", radius);
    if (radius > 1 && !scratch_dev) return dlv_fail(ctx, DLV_EINVAL, "cc_shell: scratch_dev is NULL with radius %d (needed above 1)", radius);
    if (raw_dev) DLV_TRY(check_raw_pitches(ctx, "cc_shell", Y, X, raw_pitch_y, raw_pitch_z));
    if (((uintptr_t)labels_dev & 3) || ((uintptr_t)shell_dev & 3) || ((uintptr_t)scratch_dev & 3) || ((uintptr_t)raw_dev & 1))
        return dlv_fail(ctx, DLV_EINVAL, "cc_shell: labels, shell and scratch must be 4-byte aligned, raw 2-byte aligned");
    const dim3 grid = tile_grid(Z, Y, X);
    DLV_TRY(check_tile_grid(ctx, "cc_shell", grid, Z, Y, X));
    const u64 nvox = (u64)Z * Y * X;
    const size_t bytes = (size_t)nvox * 4;
    if (ranges_overlap(shell_dev, labels_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "cc_shell: shell_dev overlaps labels_dev");
    if (scratch_dev && ranges_overlap(scratch_dev, labels_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "cc_shell: scratch_dev overlaps labels_dev");
    if (scratch_dev && ranges_overlap(scratch_dev, shell_dev, bytes)) return dlv_fail(ctx, DLV_EINVAL, "cc_shell: scratch_dev overlaps shell_dev");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    // Step i = 1..radius writes shell_dev when radius - i is even, scratch_dev otherwise, and reads what step i - 1 wrote
    // (step 1: the labels).  Both buffers start as zeros and a tile without input writes nothing: the support of E_k only
    // grows, so what such a tile would overwrite - zeros, or the E_{k-1} of two steps ago - is zero on it already.
    DlvProf pr(ctx, "cc_shell", 0.0, (double)nvox * (4.0 * (radius > 1 ? 2 : 1) + 8.0 * radius));
    hipError_t cleared = hipMemsetAsync(shell_dev, 0, bytes, ctx->stream);  // (inside the timed bracket: part of the price)
    if (cleared == hipSuccess && radius > 1) cleared = hipMemsetAsync(scratch_dev, 0, bytes, ctx->stream);
    const u32* src = labels_dev;
    for (int i = 1; i <= radius && cleared == hipSuccess; ++i) {
        u32* dst = ((radius - i) & 1) ? scratch_dev : shell_dev;
        if (i < radius)
            hipLaunchKernelGGL(cc_shell_sweep_kernel<false>, grid, dim3(256), 0, ctx->stream, src, labels_dev, (const unsigned short*)nullptr,
                               Z, Y, X, 0ll, 0ll, dst);
        else
            hipLaunchKernelGGL(cc_shell_sweep_kernel<true>, grid, dim3(256), 0, ctx->stream, src, labels_dev, raw_dev, Z, Y, X,
                               (long long)raw_pitch_y, (long long)raw_pitch_z, dst);
        src = dst;
    }
    pr.end();
    DLV_HIP(ctx, cleared);
    DLV_LAUNCH_CHECK(ctx, "cc_shell_sweep_kernel");
    return DLV_OK;
}
