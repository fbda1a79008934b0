// cc_pair_table.h - the open-addressed table of label pairs that cc_overlap.hip and cc_neighbours.hip fill, and its compaction.
// cap slots (a power of two) of {uint64 key, uint64 value} in HBM, zeroed by the caller, key 0 = empty.  A key is hashed with the
// 64-bit finaliser of splitmix64 and probed linearly: a relaxed load of the slot's key and a 64-bit compare-and-swap where it reads
// empty; what is done to the value of the slot that holds the key (an atomic add of voxels, an atomic maximum of a complemented
// distance) is the caller's business.  Every loop is bounded: a probe visits at most cap slots, and a key that finds none - or, in
// the compaction, an occupied slot beyond out_cap - sets the overflow word of the call's device words, which the host turns into an
// error that names the table.  No loop waits for another wave or spins on memory.  Header only, no state.
#pragma once
#include "cc_fold.h"

#include <type_traits>

namespace {

constexpr int PT_CT = 256;                   // threads per workgroup of the compaction
constexpr int PT_CPL = 8;                    // slots per lane and trip of the compaction
constexpr int PT_CSLOTS = 64 * PT_CPL;       // ... and per wave: one cursor atomic per 512 slots
constexpr u64 PT_COMPACT_MAX_WG = 256 * 8;

typedef u64 u64x2_t __attribute__((ext_vector_type(2)));

// device words of one call: [0] the segments of a count / the compaction's cursor, [1] the overflow word
enum { W_COUNT = 0, W_OVERFLOW = 1, W_WORDS = 2 };
constexpr u64 OVERFLOW_TABLE = 1, OVERFLOW_OUT = 2;

__device__ __forceinline__ u64 mix64(u64 x) {  // splitmix64's finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// the value word of the slot of `key`, claimed where the key is new: at most cap probes; nullptr, and the overflow word set, where
// no slot is left
__device__ __forceinline__ u64* pair_slot(u64* __restrict__ table, u64 cap, u64 key, u64* __restrict__ words) {
    const u64 mask = cap - 1;
    u64 slot = mix64(key) & mask;
    for (u64 i = 0; i < cap; ++i, slot = (slot + 1) & mask) {
        u64* at = table + 2 * slot;
        u64 held = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (a key, once set, never changes)
        if (held == 0) held = atomicCAS(at, 0ull, key);                                // (returns what was there: 0 = the slot is ours now)
        if (held == 0 || held == key) return at + 1;
    }
    atomicOr(words + W_OVERFLOW, OVERFLOW_TABLE);
    return nullptr;
}

// ---- compact: the occupied slots, in no particular order ---------------------------------------------------------------------
// One pass over the slots writes the occupied ones to keys_out / values_out at a cursor advanced once per wave and 512 slots (eight
// ballots + popcounts, one returning atomic: with one atomic per 64 slots the pass ran at the rate of that one word, 0.40 ms for
// 2 million slots).  V = u64: the value as it stands; V = u32: 2^32 - 1 - its low word (the complement cc_neighbours.hip stores).
template <typename V>
__global__ void __launch_bounds__(PT_CT) pair_table_compact_kernel(const u64* __restrict__ table, u64 cap, u64* __restrict__ keys_out,
                                                                   V* __restrict__ values_out, u64 out_cap, u64* __restrict__ words) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const u64 stride = (u64)gridDim.x * (PT_CT / 64) * PT_CSLOTS;
    // a wave takes PT_CSLOTS slots per trip, PT_CPL rounds of 64 neighbours (wave-uniform trip count)
    for (u64 first = ((u64)blockIdx.x * (PT_CT / 64) + (threadIdx.x >> 6)) * PT_CSLOTS; first < cap; first += stride) {
        u64x2_t s[PT_CPL];
        unsigned long long m[PT_CPL];
        u32 total = 0;
#pragma unroll
        for (int j = 0; j < PT_CPL; ++j) {
            const u64 slot = first + (u64)j * 64 + lane;
            s[j] = u64x2_t{0ull, 0ull};
            if (slot < cap) s[j] = *reinterpret_cast<const u64x2_t*>(table + 2 * slot);
            m[j] = __ballot(s[j].x != 0);
            total += (u32)__popcll(m[j]);
        }
        if (!total) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(words + W_COUNT, (u64)total);
        base = shfl64(base, 0);
#pragma unroll
        for (int j = 0; j < PT_CPL; ++j) {
            if (s[j].x != 0) {
                const u64 at = base + (u64)__popcll(m[j] & below);
                if (at < out_cap) {
                    keys_out[at] = s[j].x;
                    if constexpr (std::is_same<V, u64>::value) values_out[at] = s[j].y;
                    else values_out[at] = 0xffffffffu - (u32)s[j].y;
                } else {
                    atomicOr(words + W_OVERFLOW, OVERFLOW_OUT);
                }
            }
            base += (u64)__popcll(m[j]);
        }
    }
}

__host__ __forceinline__ unsigned pair_table_compact_grid(u64 cap) {
    const u64 per_wg = (u64)(PT_CT / 64) * PT_CSLOTS;
    return (unsigned)((cap + per_wg - 1) / per_wg < PT_COMPACT_MAX_WG ? (cap + per_wg - 1) / per_wg : PT_COMPACT_MAX_WG);
}

}  // namespace
