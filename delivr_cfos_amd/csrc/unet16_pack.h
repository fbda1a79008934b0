// unet16_pack.h - weight packers of the 16-bit U-Net path (device side, once per dlv_unet_load).
// A fragment of unet_bf16.hip, which alone includes it (after common.h, prec16.h and its Mish helpers): one translation unit,
// one object, the flags of that file.
#pragma once
namespace {

// ---------------------------------------------------------------------------------------------------
// weight packing (device side, once per dlv_unet_load)
// ---------------------------------------------------------------------------------------------------
// conv:   out[((cb*27 + t)*KP + kp)*64 + lane][j] = W[cout = cb*32 + (lane&31)][cin = kp*16 + 8*(lane>>5) + j][t]
template <class P>
__global__ void pack_conv_w_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int cout, int cin, float wscale) {
    const int KP = cin / 16;
    const long long n = (long long)cout * cin * 27;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int kp = (int)(r % KP);
        r /= KP;
        const int t = (int)(r % 27);
        const int cb = (int)(r / 27);
        const int co = cb * 32 + (lane & 31);
        const int ci = kp * 16 + 8 * (lane >> 5) + j;
        const float v = w[((long long)co * cin + ci) * 27 + t] * wscale;  // (2^-shift: exact)
        out[i] = (uint16_t)(P::pack2(v, 0.f) & 0xffffu);
    }
}
// stem (Cin = 1, Cout = 32): K = 64 = {hi byte, lo byte} x 32 tap slots (27 used).  The uint16 input is split
// exactly into x = 256*hi + lo (both exact in bf16), the weights carry the factor 256 for the hi half:
//   out[(s*64 + lane)*8 + j]: tap = 8 s + 4 (lane>>5) + (j>>1), part = j&1 (0: lo byte, 1: hi byte), cout = lane&31
template <class P>
__global__ void pack_stem_w_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, float wscale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * 64 * 8) return;
    const int j = i & 7, lane = (i >> 3) & 63, s = i >> 9;
    const int co = lane & 31;
    float v = 0.f;
    // k-step s, lane half h: taps 8s + 4h + (j >> 1), low byte (j even) then high byte (j odd) of the same tap - the
    // (lo, hi) pair of one tap is one 32-bit word of the staged tile, i.e. one register of the MFMA operand
    const int tap = 8 * s + 4 * (lane >> 5) + (j >> 1);
    if (tap < 27) v = w[co * 27 + tap] * ((j & 1) ? 256.f : 1.f) * P::STEM_SCALE * wscale;
    out[i] = (uint16_t)(P::pack2(v, 0.f) & 0xffffu);
}
__global__ void scale_copy_kernel(const float* __restrict__ in, float* __restrict__ out, int n, float f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] * f;
}
// deconv: out[((par*CB + cb)*KP + kp)*64 + lane][j] = W[cin = kp*16 + 8*(lane>>5) + j][cout = cb*32 + (lane&31)][par]
template <class P>
__global__ void pack_deconv_w_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int cin, int cout) {
    const int KP = cin / 16, CB = cout / 32;
    const long long n = (long long)cin * cout * 8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int kp = (int)(r % KP);
        r /= KP;
        const int cb = (int)(r % CB);
        const int par = (int)(r / CB);
        const int co = cb * 32 + (lane & 31);
        const int ci = kp * 16 + 8 * (lane >> 5) + j;
        const float v = w[((long long)ci * cout + co) * 8 + par];
        out[i] = (uint16_t)(P::pack2(v, 0.f) & 0xffffu);
    }
}

}  // namespace
