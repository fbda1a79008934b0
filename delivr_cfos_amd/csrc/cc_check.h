// cc_check.h - what the entry points of the label files check of their arguments before anything is launched, and the carver of
// their scratch slots.  Host only.  A check returns DLV_OK or fails through dlv_fail with a message that starts with `what`, the
// entry's name: DLV_TRY(check_volume(ctx, "cc_shell", Z, Y, X)).
#pragma once
#include "common.h"

namespace {

inline int check_volume(dlv_ctx* ctx, const char* what, int Z, int Y, int X) {
    if (Z < 1 || Y < 1 || X < 1) return dlv_fail(ctx, DLV_EINVAL, "%s: empty volume", what);
    return DLV_OK;
}

// the labels 0..n of a uint32 volume leave 0xffffffff free ("no voxel", cc_fold.h)
inline int check_label_count(dlv_ctx* ctx, const char* what, uint64_t n) {
    if (n >= 0xffffffffull) return dlv_fail(ctx, DLV_EINVAL, "%s: n = %llu does not fit the uint32 labels", what, (unsigned long long)n);
    return DLV_OK;
}

// the pitches (in elements) of the raw volume beside a label volume of rows of X voxels and planes of Y rows
inline int check_raw_pitches(dlv_ctx* ctx, const char* what, int Y, int X, int64_t pitch_y, int64_t pitch_z) {
    if (pitch_y < X || pitch_z / Y < pitch_y)
        return dlv_fail(ctx, DLV_EINVAL, "%s: raw pitches (%lld, %lld) do not hold rows of %d and planes of %d rows", what, (long long)pitch_z,
                        (long long)pitch_y, X, Y);
    return DLV_OK;
}

// the grid of a kernel that takes one workgroup per tile of the volume (cc_tile.h)
inline int check_tile_grid(dlv_ctx* ctx, const char* what, const dim3& grid, int Z, int Y, int X) {
    if (grid.y > 65535u || grid.z > 65535u) return dlv_fail(ctx, DLV_EINVAL, "%s: a volume of %d x %d x %d exceeds the launch grid", what, Z, Y, X);
    return DLV_OK;
}

// a voxel spacing of the distance map (cc_depth.hip)
inline int check_spacing(dlv_ctx* ctx, const char* what, const char* axis, int w) {
    if (w < 1 || w > 64) return dlv_fail(ctx, DLV_EINVAL, "%s: spacing w%s = %d is outside 1..64", what, axis, w);
    return DLV_OK;
}
// every (w d)^2 of a walk of the distance map, and so every value of the map, stays below 2^32
inline int check_reach(dlv_ctx* ctx, const char* what, const char* axis, int w, int dim) {
    if ((long long)w * (((long long)dim + 2) / 2) >= 65536)
        return dlv_fail(ctx, DLV_EUNSUP, "%s: axis %s: spacing %d over %d voxels: %d * ceil((%d + 1) / 2) does not stay below 65536, "
                        "the squared distances are uint32", what, axis, w, dim, w, dim);
    return DLV_OK;
}

// [a, a + bytes) and [b, b + bytes) share a byte
inline bool ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bytes && pb < pa + bytes;
}

// The parts of a scratch slot, one after the other, each on a 256-byte boundary: take(bytes) gives the offset of the next part,
// end is the size of the slot that holds the parts taken so far.
struct WsCarve {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = (end + 255) & ~(size_t)255;
        end = at + bytes;
        return at;
    }
};

}  // namespace
