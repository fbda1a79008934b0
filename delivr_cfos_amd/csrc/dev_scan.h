// dev_scan.h - the device-wide exclusive scan of a table of u32 counts (ccl.hip: the roots per renumbering block and the size
// filter's keep flags; fill_holes.hip: the gaps per row; cc_runs.hip: the runs per row) and the 256-thread block scan under it.
// Header only, no state.
//
// Three coalesced steps (a single block walking 500 k counts with one strided stream per thread took 0.9 ms of a 9 ms labelling):
// the sums of SCAN_GROUP-count groups, a one-block scan of the group sums, then every group scans its own counts.  Inside a group
// the arithmetic is 32 bits; the group sums, the output and the total are Out: u32 (the output may be the input), or u64 for a
// total that does not fit 32 bits.  Unsigned integer work only: the result is exact.
#pragma once
#include "common.h"
#include "cc_types.h"

namespace {

constexpr int SCAN_GROUP = 1024;  // counts per group: four per thread of dev_scan_apply_kernel
__host__ __device__ __forceinline__ u64 scan_groups(u64 rows) { return (rows + SCAN_GROUP - 1) / SCAN_GROUP; }

// exclusive scan of v over the 256 threads of the workgroup; *total = the sum of all of them.  Every thread must call it.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* total) {
    __shared__ T wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T base = 0;
    for (int k = 0; k < wave; ++k) base += wsum[k];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return base + incl - v;
}

template <typename Out>
__global__ void __launch_bounds__(256) dev_scan_sums_kernel(const u32* __restrict__ in, u64 rows, Out* __restrict__ gsum) {
    const u64 g0 = (u64)blockIdx.x * SCAN_GROUP;
    u32 s = 0;
    for (int i = threadIdx.x; i < SCAN_GROUP; i += 256)
        if (g0 + i < rows) s += in[g0 + i];
    u32 total;
    block_excl_scan(s, &total);
    if (threadIdx.x == 0) gsum[blockIdx.x] = total;
}

// one workgroup: thread t owns `per` consecutive groups (more than one above 1024 groups)
template <typename Out>
__global__ void __launch_bounds__(1024) dev_scan_groups_kernel(Out* __restrict__ gsum, u64 ng, Out* __restrict__ total_out) {
    __shared__ Out part[1024];
    const u64 per = (ng + 1023) / 1024;
    const u64 b0 = min((u64)threadIdx.x * per, ng), b1 = min(b0 + per, ng);
    Out s = 0;
    for (u64 i = b0; i < b1; ++i) s += gsum[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        Out run = 0;
        for (int k = 0; k < 1024; ++k) {
            const Out v = part[k];
            part[k] = run;
            run += v;
        }
        *total_out = run;
    }
    __syncthreads();
    Out run = part[threadIdx.x];
    for (u64 i = b0; i < b1; ++i) {
        const Out v = gsum[i];
        gsum[i] = run;
        run += v;
    }
}

// (in and out are not __restrict__: out may be in - a thread reads its four counts before the block scan's barriers and writes
// them after)
template <typename Out>
__global__ void __launch_bounds__(256) dev_scan_apply_kernel(const u32* in, u64 rows, const Out* __restrict__ gsum, Out* out) {
    const u64 g0 = (u64)blockIdx.x * SCAN_GROUP;
    u32 v[SCAN_GROUP / 256];
    u32 mine = 0;
#pragma unroll
    for (int k = 0; k < SCAN_GROUP / 256; ++k) {  // thread t owns the 4 consecutive counts 4t .. 4t+3 of the group
        const u64 i = g0 + (u64)threadIdx.x * (SCAN_GROUP / 256) + k;
        v[k] = i < rows ? in[i] : 0u;
        mine += v[k];
    }
    u32 total;
    Out run = gsum[blockIdx.x] + block_excl_scan(mine, &total);
#pragma unroll
    for (int k = 0; k < SCAN_GROUP / 256; ++k) {
        const u64 i = g0 + (u64)threadIdx.x * (SCAN_GROUP / 256) + k;
        if (i < rows) out[i] = run;
        run += v[k];
    }
}

// out[i] = in[0] + .. + in[i - 1] for i < rows (>= 1; at most 2^31 - 1 groups: one workgroup per group), *total = the sum of all
// rows.  out may be in where Out is u32; gsum: scratch of scan_groups(rows) Outs; all on the device.  what: the name in the
// message of a failed launch.
template <typename Out>
int dev_excl_scan(dlv_ctx* ctx, const u32* in, u64 rows, Out* out, Out* gsum, Out* total, const char* what) {
    const u64 ng = scan_groups(rows);
    hipLaunchKernelGGL(dev_scan_sums_kernel<Out>, dim3((unsigned)ng), dim3(256), 0, ctx->stream, in, rows, gsum);
    hipLaunchKernelGGL(dev_scan_groups_kernel<Out>, dim3(1), dim3(1024), 0, ctx->stream, gsum, ng, total);
    hipLaunchKernelGGL(dev_scan_apply_kernel<Out>, dim3((unsigned)ng), dim3(256), 0, ctx->stream, in, rows, (const Out*)gsum, out);
    DLV_LAUNCH_CHECK(ctx, what);
    return DLV_OK;
}

}  // namespace
