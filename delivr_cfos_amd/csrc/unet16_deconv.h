// unet16_deconv.h - the four transposed-conv kernels (k2, s2): per parity, by rows, register-resident and stationary weights.
// A fragment of unet_bf16.hip, which alone includes it (after common.h, prec16.h and its Mish helpers): one translation unit,
// one object, the flags of that file.
#pragma once
namespace {

// ---------------------------------------------------------------------------------------------------
// ConvTranspose3d k2 s2 on MFMA: for each of the 8 output parities a (Cin x Cout) channel GEMM
//   wave: 32 consecutive input voxels (B fragments straight from HBM, no LDS), all parities/couts
// ---------------------------------------------------------------------------------------------------
template <class P, int KP>  // Cin / 16
__global__ void __launch_bounds__(256) deconv2_mfma_kernel(const uint4* __restrict__ in, const uint4* __restrict__ wpk,
                                                           const float* __restrict__ bias, uint4* __restrict__ out,
                                                           int cout, int D, int H, int W) {
    const int n = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const long long vox = (long long)D * H * W;
    const long long v = ((long long)blockIdx.x * 4 + wave) * 32 + col;
    const bool ok = v < vox;
    const long long vc = ok ? v : 0;
    uint4 b[KP];
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
        uint4 u = in[((long long)n * (2 * KP) + 2 * kp + h) * vox + vc];
        if (!ok) u = make_uint4(0, 0, 0, 0);
        b[kp] = AS_FRAG(u);
    }
    const int x = (int)(vc % W), y = (int)((vc / W) % H), z = (int)(vc / ((long long)W * H));
    const int CB = cout / 32, cout8 = cout / 8;
    const int OH = 2 * H, OW = 2 * W;
    const long long ovox = vox * 8;
    for (int par = 0; par < 8; ++par) {
        const long long o = ((long long)(2 * z + (par >> 2)) * OH + (2 * y + ((par >> 1) & 1))) * OW + 2 * x + (par & 1);
        for (int cb = 0; cb < CB; ++cb) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bias[cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
#pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                const uint4 u = wpk[(((long long)par * CB + cb) * KP + kp) * 64 + lane];
                acc = P::mfma(AS_FRAG(u), b[kp], acc, 0, 0, 0);
            }
            if (ok) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 u;
                    u.x = P::pack2(acc[4 * g + 0], acc[4 * g + 1]);
                    u.y = P::pack2(acc[4 * g + 2], acc[4 * g + 3]);
                    uint2* dst = reinterpret_cast<uint2*>(out + ((long long)n * cout8 + cb * 4 + g) * ovox + o);
                    dst[h] = u;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// ConvTranspose3d k2 s2, row-contiguous form: the 32 MFMA columns are 32 CONSECUTIVE OUTPUT voxels of one
// output row (input voxel = column >> 1, x-parity = column & 1).  The parity-dependent weights are applied
// with two MFMAs per k-step on parity-masked copies of the input fragment, and permlane32_swap joins the
// two half-wave channel quads, so that every store is 16 bytes per lane and 512 contiguous bytes per
// half-wave (the per-parity form above writes 8-byte halves at a stride of two voxels).
// ---------------------------------------------------------------------------------------------------
template <class P, int KP>
__global__ void __launch_bounds__(256) deconv2_rows_kernel(const uint4* __restrict__ in, const uint4* __restrict__ wpk,
                                                           const float* __restrict__ bias, uint4* __restrict__ out,
                                                           int cout, int D, int H, int W, int segs,
                                                           const float2* __restrict__ ss) {
    const int n = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const long long vox = (long long)D * H * W;
    const long long item = (long long)blockIdx.x * 4 + wave;  // (z, y, x-segment of 16 input voxels)
    const long long nitems = (long long)D * H * segs;
    if (item >= nitems) return;
    const int sg = (int)(item % segs), y = (int)((item / segs) % H), z = (int)(item / ((long long)segs * H));
    const int xi = sg * 16 + (col >> 1);
    const bool ok = xi < W;
    const bool odd = col & 1;
    const long long vin = ((long long)z * H + y) * W + (ok ? xi : 0);
    uint4 b0[KP], b1[KP];
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
        uint4 u = in[((long long)n * (2 * KP) + 2 * kp + h) * vox + vin];
        if (ss) {  // the input is the raw output of a conv: its InstanceNorm + Mish are applied here (wave-uniform branch)
            float sc[8], sh[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float2 v = ss[n * (16 * KP) + (2 * kp + h) * 8 + k];
                sc[k] = v.x;
                sh[k] = v.y;
            }
            u = norm_mish8<P>(u, sc, sh, nullptr);
        }
        b0[kp] = AS_FRAG((ok && !odd) ? u : zero4);
        b1[kp] = AS_FRAG((ok && odd) ? u : zero4);
    }
    const int CB = cout / 32, cout8 = cout / 8;
    const int OH = 2 * H, OW = 2 * W;
    const long long ovox = vox * 8;
    const int ox = 2 * sg * 16 + col;
    for (int ab = 0; ab < 4; ++ab) {
        const long long o = ((long long)(2 * z + (ab >> 1)) * OH + (2 * y + (ab & 1))) * OW + ox;
        for (int cb = 0; cb < CB; ++cb) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bias[cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
#pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                const uint4 w0 = wpk[(((long long)(ab * 2 + 0) * CB + cb) * KP + kp) * 64 + lane];
                const uint4 w1 = wpk[(((long long)(ab * 2 + 1) * CB + cb) * KP + kp) * 64 + lane];
                acc = P::mfma(AS_FRAG(w0), b0[kp], acc, 0, 0, 0);
                acc = P::mfma(AS_FRAG(w1), b1[kp], acc, 0, 0, 0);
            }
            unsigned px[4], py[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                px[g] = P::pack2(acc[4 * g + 0], acc[4 * g + 1]);
                py[g] = P::pack2(acc[4 * g + 2], acc[4 * g + 3]);
            }
#pragma unroll
            for (int gp = 0; gp < 4; gp += 2) {
                // lanes 0-31 end up with all 8 channels of chunk gp, lanes 32-63 with chunk gp+1
                const auto sx = __builtin_amdgcn_permlane32_swap(px[gp], px[gp + 1], false, false);
                const auto sy = __builtin_amdgcn_permlane32_swap(py[gp], py[gp + 1], false, false);
                if (ok) out[((long long)n * cout8 + cb * 4 + gp + h) * ovox + o] = make_uint4(sx[0], sy[0], sx[1], sy[1]);
            }
        }
    }
}

// The same op for the two large levels (Cout = 32, Cin <= 64: 2.1 GB of output per 16 windows at the top level, an
// HBM-write-bound kernel): all 8 taps' weights stay in registers (32 x KP VGPRs), every wave walks DC_IPW consecutive
// row segments and fetches the next segment's input while the MFMAs and stores of the current one are in flight - the
// per-segment kernel above re-reads 16 KB of weights through L1 for 8 KB of output and exposes every load latency.
constexpr int DC_IPW = DLV_DC_IPW;  // row segments (16 input voxels -> 4 x 32 output voxels x 32 channels = 8 KB) per wave

template <class P, int KP>
__global__ void __launch_bounds__(256) deconv2_regw_kernel(const uint4* __restrict__ in, const uint4* __restrict__ wpk,
                                                           const float* __restrict__ bias, uint4* __restrict__ out, int D,
                                                           int H, int W, int segs, const float2* __restrict__ ss) {
    const int n = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (wave-uniform by construction: lets z / y /
                                                                                 // the row offsets live in SGPRs)
    const int h = lane >> 5, col = lane & 31;
    const long long vox = (long long)D * H * W;
    const unsigned nitems = (unsigned)D * (unsigned)H * (unsigned)segs;  // row segments of one window: 32-bit index math
    const unsigned item0 = ((unsigned)blockIdx.x * 4u + (unsigned)wave) * (unsigned)DC_IPW;
    if (item0 >= nitems) return;
    const bool odd = col & 1;
    uint4 w0[4][KP], w1[4][KP];
#pragma unroll
    for (int ab = 0; ab < 4; ++ab)
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            w0[ab][kp] = wpk[((long long)(ab * 2 + 0) * KP + kp) * 64 + lane];
            w1[ab][kp] = wpk[((long long)(ab * 2 + 1) * KP + kp) * 64 + lane];
        }
    f32x16 bsv;  // the bias is the C operand of each parity's first MFMA (no 16 moves per parity to seed an accumulator)
#pragma unroll
    for (int r = 0; r < 16; ++r) bsv[r] = bias[(r & 3) + 8 * (r >> 2) + 4 * h];
    float sc[KP][8], sh[KP][8];
    if (ss) {
#pragma unroll
        for (int kp = 0; kp < KP; ++kp)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float2 v = ss[n * (16 * KP) + (2 * kp + h) * 8 + k];
                sc[kp][k] = v.x;
                sh[kp][k] = v.y;
            }
    }
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const int OH = 2 * H, OW = 2 * W;
    const long long ovox = vox * 8;
    // output through a buffer resource over this sample's four chunks (4 * ovox * 16 B < 2^32: the launcher checks): the
    // chunk part of an address is an SGPR offset, the voxel part a 32-bit lane offset; lanes beyond the row end carry an
    // out-of-range offset and the hardware drops their store
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(out + (long long)n * 4 * ovox, 0, (int)(unsigned)(4 * ovox * 16), 0x00020000);
    const unsigned chunk_b = (unsigned)ovox * 16u;
    const uint4* inb = in + ((long long)n * (2 * KP) + h) * vox;
    auto fetch = [&](unsigned item, uint4 (&u)[KP]) __attribute__((always_inline)) {
        const int sg = (int)(item % (unsigned)segs);
        const unsigned zy = item / (unsigned)segs;  // z * H + y
        const int xi = sg * 16 + (col >> 1);
        const long long vin = (long long)zy * W + (xi < W ? xi : 0);
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) u[kp] = inb[(long long)(2 * kp) * vox + vin];
    };
    uint4 cur[KP], nxt[KP];
    fetch(item0, cur);
#pragma unroll 1
    for (int it = 0; it < DC_IPW; ++it) {
        const unsigned item = item0 + (unsigned)it;
        if (item >= nitems) break;
        if (item + 1 < nitems && it + 1 < DC_IPW) fetch(item + 1, nxt);
        const int sg = (int)(item % (unsigned)segs), y = (int)((item / (unsigned)segs) % (unsigned)H), z = (int)(item / ((unsigned)segs * (unsigned)H));
        const bool ok = sg * 16 + (col >> 1) < W;
        uint4 b0[KP], b1[KP];
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            uint4 u = cur[kp];
            if (ss) u = norm_mish8<P>(u, sc[kp], sh[kp], nullptr);  // the input is a raw conv output (wave-uniform branch)
            b0[kp] = AS_FRAG((ok && !odd) ? u : zero4);
            b1[kp] = AS_FRAG((ok && odd) ? u : zero4);
        }
        const unsigned ox = (unsigned)(2 * sg * 16 + col);
        const unsigned lane_b = ok ? (ox + (unsigned)h * (unsigned)ovox) * 16u : 0xfffffff0u;  // chunk gp + h: h in the lane part
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const unsigned row_b = (unsigned)(((2 * z + (ab >> 1)) * OH + (2 * y + (ab & 1))) * OW) * 16u;  // wave-uniform
            f32x16 acc = P::mfma(AS_FRAG(w0[ab][0]), b0[0], bsv, 0, 0, 0);
            acc = P::mfma(AS_FRAG(w1[ab][0]), b1[0], acc, 0, 0, 0);
#pragma unroll
            for (int kp = 1; kp < KP; ++kp) {
                acc = P::mfma(AS_FRAG(w0[ab][kp]), b0[kp], acc, 0, 0, 0);
                acc = P::mfma(AS_FRAG(w1[ab][kp]), b1[kp], acc, 0, 0, 0);
            }
            unsigned px[4], py[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                px[g] = P::pack2(acc[4 * g + 0], acc[4 * g + 1]);
                py[g] = P::pack2(acc[4 * g + 2], acc[4 * g + 3]);
            }
#pragma unroll
            for (int gp = 0; gp < 4; gp += 2) {
                // lanes 0-31 end up with all 8 channels of chunk gp, lanes 32-63 with chunk gp+1
                const auto sx = __builtin_amdgcn_permlane32_swap(px[gp], px[gp + 1], false, false);
                const auto sy = __builtin_amdgcn_permlane32_swap(py[gp], py[gp + 1], false, false);
                typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
                __builtin_amdgcn_raw_buffer_store_b128(u32x4v{sx[0], sy[0], sx[1], sy[1]}, ors, (int)lane_b,
                                                       (int)(row_b + (unsigned)gp * chunk_b), 0);
            }
        }
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) cur[kp] = nxt[kp];
    }
}

// The deep levels (Cin >= 128): few voxels, many weights - the per-segment kernel re-reads all 8 x Cin x Cout weights for
// every 16 input voxels (524 KB per wave at 256 -> 128).  Here a wave keeps the fragments of ONE (output parity pair ab,
// 32-channel output block cb) in registers (2 x KP) and walks DW_IPW row segments with them; grid.y enumerates (ab, cb).
constexpr int DW_IPW = 4;

template <class P, int KP>
__global__ void __launch_bounds__(256) deconv2_wst_kernel(const uint4* __restrict__ in, const uint4* __restrict__ wpk,
                                                          const float* __restrict__ bias, uint4* __restrict__ out, int cout,
                                                          int D, int H, int W, int segs, const float2* __restrict__ ss) {
    const int n = blockIdx.z;
    const int CB = cout / 32, cout8 = cout / 8;
    const int ab = blockIdx.y / CB, cb = blockIdx.y % CB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const long long vox = (long long)D * H * W;
    const long long nitems = (long long)D * H * segs;
    const long long item0 = ((long long)blockIdx.x * 4 + wave) * DW_IPW;
    if (item0 >= nitems) return;
    const bool odd = col & 1;
    uint4 w0[KP], w1[KP];
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
        w0[kp] = wpk[(((long long)(ab * 2 + 0) * CB + cb) * KP + kp) * 64 + lane];
        w1[kp] = wpk[(((long long)(ab * 2 + 1) * CB + cb) * KP + kp) * 64 + lane];
    }
    float bs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bs[r] = bias[cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const int OH = 2 * H, OW = 2 * W;
    const long long ovox = vox * 8;
    const uint4* inb = in + ((long long)n * (2 * KP) + h) * vox;
#pragma unroll 1
    for (int it = 0; it < DW_IPW; ++it) {
        const long long item = item0 + it;
        if (item >= nitems) break;
        const int sg = (int)(item % segs), y = (int)((item / segs) % H), z = (int)(item / ((long long)segs * H));
        const int xi = sg * 16 + (col >> 1);
        const bool ok = xi < W;
        const long long vin = ((long long)z * H + y) * W + (ok ? xi : 0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bs[r];
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            uint4 u = inb[(long long)(2 * kp) * vox + vin];
            if (ss) {  // the input is the raw output of a conv: its InstanceNorm + Mish are applied here (wave-uniform branch)
                float sc[8], sh[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float2 v = ss[n * (16 * KP) + (2 * kp + h) * 8 + k];
                    sc[k] = v.x;
                    sh[k] = v.y;
                }
                u = norm_mish8<P>(u, sc, sh, nullptr);
            }
            acc = P::mfma(AS_FRAG(w0[kp]), AS_FRAG((ok && !odd) ? u : zero4), acc, 0, 0, 0);
            acc = P::mfma(AS_FRAG(w1[kp]), AS_FRAG((ok && odd) ? u : zero4), acc, 0, 0, 0);
        }
        const long long o = ((long long)(2 * z + (ab >> 1)) * OH + (2 * y + (ab & 1))) * OW + 2 * sg * 16 + col;
        unsigned px[4], py[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            px[g] = P::pack2(acc[4 * g + 0], acc[4 * g + 1]);
            py[g] = P::pack2(acc[4 * g + 2], acc[4 * g + 3]);
        }
#pragma unroll
        for (int gp = 0; gp < 4; gp += 2) {
            const auto sx = __builtin_amdgcn_permlane32_swap(px[gp], px[gp + 1], false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(py[gp], py[gp + 1], false, false);
            if (ok) out[((long long)n * cout8 + cb * 4 + gp + h) * ovox + o] = make_uint4(sx[0], sy[0], sx[1], sy[1]);
        }
    }
}

}  // namespace
