// unet16_norm.h - InstanceNorm statistics (stats_finalize) and the InstanceNorm + Mish (+ MaxPool) passes.
// A fragment of unet_bf16.hip, which alone includes it (after common.h, prec16.h and its Mish helpers): one translation unit,
// one object, the flags of that file.
#pragma once
namespace {

// ---------------------------------------------------------------------------------------------------
// InstanceNorm statistics: partial sums -> per (n,c) scale/shift   y = x*scale + shift
// one wave per (n,c); fixed summation order (bitwise reproducible)
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) stats_finalize_kernel(const float* __restrict__ partials, int nparts, int C,
                                                            double inv_count, float eps, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float2* __restrict__ ss,
                                                            int* __restrict__ range_flag, int layer) {
    const int c = blockIdx.x % C, n = blockIdx.x / C;
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) {
        const float2 v = *reinterpret_cast<const float2*>(partials + (((long long)n * nparts + i) * C + c) * 2);
        s += v.x;
        q += v.y;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o, 64);
        q += __shfl_down(q, o, 64);
    }
    if (threadIdx.x == 0) {
        // Range guard: a raw value beyond the 16-bit format's range is stored as Inf, the next normalisation pass turns it into
        // Inf or NaN, and the next convolution's sums - these - stop being finite.  Detected here for free; without it the mask
        // silently becomes zeros (NaN >= 0 is false).  The first such layer wins (atomicMax of 100 - layer).
        if (!(fabs(s) <= 1.0e300 && fabs(q) <= 1.0e300)) atomicMax(range_flag, 100 - layer);
        const double mean = s * inv_count;
        double var = q * inv_count - mean * mean;
        if (var < 0.0) var = 0.0;
        // ... and which layer is the large one: the sums are those of the fp32 accumulators, so they stay finite when the STORED
        // 16-bit value overflows.  The largest |mean| + 8 sigma of every block is recorded (one atomic per (window, channel) of a
        // 64-thread workgroup); after a DLV_ERANGE the host reads it as the hint for dlv_unet_set_conv_shift: how far to move a
        // block that reported > 4096, and which blocks are too SMALL to be moved at all (positive floats order like their bit patterns)
        // (a plain read first: one atomic per (window, channel) on ONE address cost 40-160 us per launch - 16 k workgroups of a
        // 64-window batch queue up on it, +24 % on a pass of 64 x 64 x 32 windows, measured; after the first few workgroups the
        // word already holds a larger value and the others only read it.  A stale read is harmless: atomicMax decides.)
        const float peak = (float)(fabs(mean) + 8.0 * sqrt(var));
        if (peak > 0.f && peak < 3.0e38f && __float_as_int(peak) > __builtin_nontemporal_load(range_flag + 1 + layer))
            atomicMax(range_flag + 1 + layer, __float_as_int(peak));
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = rstd * gamma[c];
        ss[n * C + c] = make_float2(sc, beta[c] - (float)mean * sc);
    }
}

// ---------------------------------------------------------------------------------------------------
// InstanceNorm apply + Mish (+ MaxPool3d(2) into a second tensor), in place on the raw bf16 tensor
// ---------------------------------------------------------------------------------------------------
// P: the format the raw tensor is stored in; PO: the format of the activated value (the mixed 16-bit mode changes format between
// levels 0 and 1: DLV_PREC_BF16 keeps fp16 at full resolution, section 5 of DESIGN.md)
template <class P, class PO = P>
__device__ __forceinline__ uint4 norm_mish8(uint4 u, const float* sc, const float* sh, float* mx) {
    float v[8] = {P::lo(u.x), P::hi(u.x), P::lo(u.y), P::hi(u.y), P::lo(u.z), P::hi(u.z), P::lo(u.w), P::hi(u.w)};
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const f32x2_t m = mish_fast2(fma2(f32x2_t{v[k], v[k + 1]}, f32x2_t{sc[k], sc[k + 1]}, f32x2_t{sh[k], sh[k + 1]}));
        v[k] = m.x;
        v[k + 1] = m.y;
        if (mx) {
            mx[k] = fmaxf(mx[k], v[k]);
            mx[k + 1] = fmaxf(mx[k + 1], v[k + 1]);
        }
    }
    uint4 r;
    r.x = PO::pack2(v[0], v[1]);
    r.y = PO::pack2(v[2], v[3]);
    r.z = PO::pack2(v[4], v[5]);
    r.w = PO::pack2(v[6], v[7]);
    return r;
}

// WB: write the activated tensor back in place.  POOL && !WB: only the pooled tensor is produced - the full-resolution
// tensor stays raw and every consumer applies scale/shift + Mish while it loads (conv_zreg.hip's staging, the
// transposed conv below, the final 1x1x1 conv)
// PW: format of the written-back tensor, PQ: format of the pooled tensor (both P except at the format seam of the mixed mode)
template <class P, bool POOL, bool WB, bool NT = false, class PW = P, class PQ = P>
__global__ void __launch_bounds__(256) norm_mish_kernel(uint4* __restrict__ x, const float2* __restrict__ ss, int C,
                                                        int D, int H, int W, uint4* __restrict__ pooled) {
    const int c8 = blockIdx.y, n = blockIdx.z;
    float sc[8], sh[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float2 v = ss[n * C + c8 * 8 + k];
        sc[k] = v.x;
        sh[k] = v.y;
    }
    const long long vox = (long long)D * H * W;
    uint4* p = x + ((long long)n * (C / 8) + c8) * vox;
    if (!POOL) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vox; i += (long long)gridDim.x * 256)
            dlv_st16<NT>(p + i, norm_mish8<P, PW>(dlv_ld16<NT>(p + i), sc, sh, nullptr));
    } else {
        const int d2 = D / 2, h2 = H / 2, w2 = W / 2;
        const long long pv = (long long)d2 * h2 * w2;
        uint4* q = pooled + ((long long)n * (C / 8) + c8) * pv;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pv; i += (long long)gridDim.x * 256) {
            const int xx = (int)(i % w2), yy = (int)((i / w2) % h2), zz = (int)(i / ((long long)w2 * h2));
            float mx[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) mx[k] = -INFINITY;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const long long o = ((long long)(2 * zz + a) * H + (2 * yy + b)) * W + 2 * xx;
                    // (default cache policy here: a wave's two loads / stores each touch every other 16 bytes of the same lines -
                    // with `nt` the second one misses again: 1060 -> 1340 us per forward)
                    const uint4 r0 = norm_mish8<P, PW>(p[o], sc, sh, mx), r1 = norm_mish8<P, PW>(p[o + 1], sc, sh, mx);
                    if (WB) {
                        p[o] = r0;
                        p[o + 1] = r1;
                    }
                }
            uint4 r;
            r.x = PQ::pack2(mx[0], mx[1]);
            r.y = PQ::pack2(mx[2], mx[3]);
            r.z = PQ::pack2(mx[4], mx[5]);
            r.w = PQ::pack2(mx[6], mx[7]);
            q[i] = r;
        }
    }
}

// The pooling pass by full lines (W % 64 == 0: levels 0 and 1): a wave owns 64 consecutive fine voxels of the four rows
// (2 planes x 2 rows) under 32 pooled voxels - every load / store instruction covers one contiguous KiB (the kernel above reads
// every other 16 bytes per instruction and needs the lines to survive in cache between its two loads), so the non-temporal policy
// applies; the x pair is reduced with one DPP max per value, even lanes store the pooled voxel.  Same values bit for bit (max and
// the 16-bit rounding commute).
template <class P, bool WB, bool NT, class PQ = P>
__global__ void __launch_bounds__(256) norm_mish_pool_rows_kernel(uint4* __restrict__ x, const float2* __restrict__ ss, int C, int D, int H,
                                                                  int W, uint4* __restrict__ pooled) {
    const int c8 = blockIdx.y, n = blockIdx.z;
    float sc[8], sh[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float2 v = ss[n * C + c8 * 8 + k];
        sc[k] = v.x;
        sh[k] = v.y;
    }
    const long long vox = (long long)D * H * W;
    const int d2 = D / 2, h2 = H / 2, w2 = W / 2, nseg = W / 64;
    uint4* p = x + ((long long)n * (C / 8) + c8) * vox;
    uint4* q = pooled + ((long long)n * (C / 8) + c8) * ((long long)d2 * h2 * w2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long items = (long long)d2 * h2 * nseg;
    for (long long it = (long long)blockIdx.x * 4 + wave; it < items; it += (long long)gridDim.x * 4) {
        const int xs = (int)(it % nseg), yy = (int)((it / nseg) % h2), zz = (int)(it / ((long long)nseg * h2));
        uint4 u[4];
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) u[ab] = dlv_ld16<NT>(p + ((long long)(2 * zz + (ab >> 1)) * H + (2 * yy + (ab & 1))) * W + xs * 64 + lane);
        float mx[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) mx[k] = -INFINITY;
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const uint4 r = norm_mish8<P>(u[ab], sc, sh, mx);
            if (WB) dlv_st16<NT>(p + ((long long)(2 * zz + (ab >> 1)) * H + (2 * yy + (ab & 1))) * W + xs * 64 + lane, r);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)  // the neighbour of the x pair: quad_perm [1,0,3,2]
            mx[k] = fmaxf(mx[k], __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, mx[k]), 0xB1, 0xf, 0xf, true)));
        if (!(lane & 1)) {
            uint4 r;
            r.x = PQ::pack2(mx[0], mx[1]);
            r.y = PQ::pack2(mx[2], mx[3]);
            r.z = PQ::pack2(mx[4], mx[5]);
            r.w = PQ::pack2(mx[6], mx[7]);
            dlv_st16<NT>(q + ((long long)zz * h2 + yy) * w2 + xs * 32 + (lane >> 1), r);
        }
    }
}

}  // namespace
