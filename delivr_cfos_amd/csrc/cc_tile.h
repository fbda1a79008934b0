// cc_tile.h - the LDS tile of the kernels that look at the 26 neighbours of every voxel of a uint32 volume (cc_shell.hip,
// cc_split.hip): a workgroup of 256 threads owns TZ x TY x TX voxels and stages them with a one-voxel halo, (TZ + 2) x (TY + 2)
// LDS rows of PITCH words.  Rows that start on a 16-byte boundary are moved with 16-byte accesses, the others (with an odd X the
// alignment changes from row to row) and the quad across the end of a row element by element.  Header only, no state; what is
// staged, in which order and with which barriers is the kernel's own business.
#pragma once
#include <hip/hip_runtime.h>

#include "cc_types.h"

namespace {

constexpr int TX = 64, TY = 8, TZ = 8;     // the voxels a workgroup writes: whole 256-byte runs in x
constexpr int QX = TX / 4;                 // quads per row
constexpr int PITCH = TX + 8;              // LDS row: interior at [4, 4 + TX) (16-byte aligned), the halo voxels at 3 and 4 + TX
constexpr int ROWS = (TZ + 2) * (TY + 2);  // the tile and its one-voxel halo

// the extents of the volume and the first voxel of the workgroup's tile
struct TileAt {
    int Z, Y, X, z0, y0, x0;
    __device__ __forceinline__ TileAt(int Z_, int Y_, int X_) : Z(Z_), Y(Y_), X(X_), z0(blockIdx.z * TZ), y0(blockIdx.y * TY), x0(blockIdx.x * TX) {}
};

__host__ __forceinline__ dim3 tile_grid(int Z, int Y, int X) { return dim3((X + TX - 1) / TX, (Y + TY - 1) / TY, (Z + TZ - 1) / TZ); }

// LDS row `row` (0 .. ROWS - 1) holds the row (z0 - 1 + row / (TY + 2), y0 - 1 + row % (TY + 2)) of the volume; the tile's own row
// (oz, oy) is LDS row tile_row(oz, oy), and quad q of a row (the voxels x0 + 4q .. + 3) starts at word tile_word(row, q)
__device__ __forceinline__ int tile_row(int oz, int oy) { return (oz + 1) * (TY + 2) + oy + 1; }
__device__ __forceinline__ int tile_word(int row, int q) { return row * PITCH + 4 + 4 * q; }

// quad q of LDS row `row` from a volume, 0 outside it
__device__ __forceinline__ u32x4_t tile_quad_of(const u32* __restrict__ vol, const TileAt& t, int row, int q) {
    const int Z = t.Z, Y = t.Y, X = t.X;
    const int z = t.z0 - 1 + row / (TY + 2), y = t.y0 - 1 + row % (TY + 2), x = t.x0 + 4 * q;
    u32x4_t v = {0, 0, 0, 0};
    if (z >= 0 && z < Z && y >= 0 && y < Y && x < X) {
        const u32* p = vol + ((u64)z * Y + y) * (u64)X + x;
        if (x + 4 <= X && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            v = *reinterpret_cast<const u32x4_t*>(p);
        } else {
            v.x = p[0];
            if (x + 1 < X) v.y = p[1];
            if (x + 2 < X) v.z = p[2];
            if (x + 3 < X) v.w = p[3];
        }
    }
    return v;
}

// the voxels of a quad at p = the voxel (z, y, x) that lie inside the row of X voxels
__device__ __forceinline__ void tile_store_quad(u32* p, int x, int X, u32x4_t v) {
    if (x + 4 <= X && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<u32x4_t*>(p) = v;
    } else {
        p[0] = v.x;
        if (x + 1 < X) p[1] = v.y;
        if (x + 2 < X) p[2] = v.z;
        if (x + 3 < X) p[3] = v.w;
    }
}

}  // namespace
