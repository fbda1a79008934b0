// unet16_final.h - the final 1x1x1 conv: logits, or blended straight into the accumulator.
// A fragment of unet_bf16.hip, which alone includes it (after common.h, prec16.h and its Mish helpers): one translation unit,
// one object, the flags of that file.
#pragma once
namespace {

// ---------------------------------------------------------------------------------------------------
// final: InstanceNorm + Mish of the last block, Conv3d(C5 -> 1, k1), then either plain logits or
// the blend accumulate of inference/sliding_window_inferer.py:232-251 (acc[window] += logit, un-flipped)
// ---------------------------------------------------------------------------------------------------
template <class P, bool BLEND>
__global__ void __launch_bounds__(256) final_conv_kernel(const uint4* __restrict__ x, const float2* __restrict__ ss,
                                                         const float* __restrict__ wf, const float* __restrict__ bf,
                                                         float* __restrict__ logits, const int* __restrict__ starts,
                                                         int flip_dim, int Yp, int Xp, float scale, float* __restrict__ acc,
                                                         int D, int H, int W, const float* __restrict__ bw, float bmin,
                                                         float* __restrict__ wsum, int* __restrict__ range_flag) {
    const int n = blockIdx.y;
    bool bad = false;  // range guard of the last block's raw tensor (no later InstanceNorm would see it): a non-finite logit
    // per-sample scale/shift and the 32 weights are uniform over the workgroup: scalar loads, SGPR operands
    f32x2_t sc[16], sh[16], ww[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float2 v0 = ss[n * 32 + 2 * c], v1 = ss[n * 32 + 2 * c + 1];
        sc[c] = f32x2_t{v0.x, v1.x};
        // 96 uniform values exceed the SGPR file, and a packed FMA reads at most ONE scalar pair (constant bus): the scales stay
        // in SGPRs, shifts and weights live in VGPRs - no per-use v_mov_b64 / v_readlane of a spilled pair in the loop
        float h0 = v0.y, h1 = v1.y;
        asm volatile("" : "+v"(h0), "+v"(h1));
        sh[c] = f32x2_t{h0, h1};
        float w0 = wf[2 * c], w1 = wf[2 * c + 1];
        asm volatile("" : "+v"(w0), "+v"(w1));
        ww[c] = f32x2_t{w0, w1};
    }
    const long long vox = (long long)D * H * W;
    const float b0 = bf[0];
    int z0 = 0, y0 = 0, x0 = 0;
    if (BLEND) {
        z0 = starts[3 * n];
        y0 = starts[3 * n + 1];
        x0 = starts[3 * n + 2];
    }
    // Software pipeline: the four chunk words and (plain blend) the accumulator word of iteration i + 1 are in flight while the 32
    // Mish evaluations of iteration i run.  Without it a wave alternates between waiting for its loads and ~1700 cycles of
    // arithmetic, and neither the VALU (408 us of work per 16 windows) nor HBM (420 us) is kept busy: 588 us
    // (profiles/microbench/final_probe.hip: 447 us pipelined at 8 iterations per thread).
    // (32-bit voxel indices - the launcher refuses windows of 2^31 voxels - and the window coordinates advanced by the grid
    // stride with carries instead of three 64-bit divisions per voxel: those were a third of the loop's instructions)
    const unsigned nvox = (unsigned)vox, step = gridDim.x * 256u;
    const unsigned sx = step % (unsigned)W, sy = (step / (unsigned)W) % (unsigned)H, sz = step / ((unsigned)W * (unsigned)H);
    unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < nvox) {
        unsigned xx = i % (unsigned)W, yy = (i / (unsigned)W) % (unsigned)H, zz = i / ((unsigned)W * (unsigned)H);
        auto out_index = [&](unsigned z, unsigned y, unsigned xc) -> long long {
            const int zf = flip_dim == 2 ? D - 1 - (int)z : (int)z, yf = flip_dim == 3 ? H - 1 - (int)y : (int)y,
                      xf = flip_dim == 4 ? W - 1 - (int)xc : (int)xc;
            return ((long long)(z0 + zf) * Yp + (y0 + yf)) * Xp + (x0 + xf);
        };
        const bool plain = BLEND && !bw;  // (Gaussian weights: two read-modify-writes per voxel, not prefetched)
        const uint4* xb = x + (long long)n * 4 * vox;
        uint4 u[4];
#pragma unroll
        for (int c8 = 0; c8 < 4; ++c8) u[c8] = dlv_ld16<true>(xb + (long long)c8 * vox + i);  // (read once, 64 B per voxel)
        long long o = BLEND ? out_index(zz, yy, xx) : 0;
        float av = plain ? acc[o] : 0.f;
        for (; i < nvox; i += step) {
            uint4 un[4] = {u[0], u[1], u[2], u[3]};
            long long on = o;
            float avn = 0.f;
            const unsigned zc = zz, yc = yy, xc = xx;  // this iteration's coordinates (Gaussian weights)
            const unsigned in = i + step;
            if (in < nvox && in > i) {
                xx += sx;
                const unsigned cx = xx >= (unsigned)W ? 1u : 0u;
                xx -= cx ? (unsigned)W : 0u;
                yy += sy + cx;
                const unsigned cy = yy >= (unsigned)H ? 1u : 0u;
                yy -= cy ? (unsigned)H : 0u;
                zz += sz + cy;
#pragma unroll
                for (int c8 = 0; c8 < 4; ++c8) un[c8] = dlv_ld16<true>(xb + (long long)c8 * vox + in);
                if (BLEND) on = out_index(zz, yy, xx);
                if (plain) avn = acc[on];
            }
            f32x2_t a2 = {b0, 0.f};
#pragma unroll
            for (int c8 = 0; c8 < 4; ++c8) {
                const unsigned uu[4] = {u[c8].x, u[c8].y, u[c8].z, u[c8].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f32x2_t v = {P::lo(uu[k]), P::hi(uu[k])};
                    a2 = fma2(mish_fast2(fma2(v, sc[4 * c8 + k], sh[4 * c8 + k])), ww[4 * c8 + k], a2);
                }
            }
            const float a = a2.x + a2.y;
            bad |= !(fabsf(a) <= 3.0e38f);
            if (!BLEND) {
                logits[(long long)n * vox + i] = a;
            } else if (bw) {  // Gaussian importance map, indexed in volume orientation (after the un-flip)
                const int zf = flip_dim == 2 ? D - 1 - (int)zc : (int)zc, yf = flip_dim == 3 ? H - 1 - (int)yc : (int)yc,
                          xf = flip_dim == 4 ? W - 1 - (int)xc : (int)xc;
                const float wgt = fmaxf(bw[zf] * bw[D + yf] * bw[D + H + xf], bmin) * scale;
                acc[o] += wgt * a;
                if (wsum) wsum[o] += wgt;
            } else {
                acc[o] = av + scale * a;
            }
#pragma unroll
            for (int c8 = 0; c8 < 4; ++c8) u[c8] = un[c8];
            o = on;
            av = avn;
            if (in <= i) break;  // (32-bit wrap-around of the index)
        }
    }
    if (bad) atomicMax(range_flag, 100 - 18);
}

}  // namespace
