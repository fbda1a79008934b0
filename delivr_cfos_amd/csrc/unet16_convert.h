// unet16_convert.h - replicate padding and the fp32 NCDHW <-> chunk-planar conversions of the test hooks.
// A fragment of unet_bf16.hip, which alone includes it (after common.h, prec16.h and its Mish helpers): one translation unit,
// one object, the flags of that file.
#pragma once
namespace {

// ---------------------------------------------------------------------------------------------------
// debug / test conversions: fp32 NCDHW <-> bf16 chunk-planar
// ---------------------------------------------------------------------------------------------------
// MONAI UpCat's replicate padding (monai/networks/nets/basic_unet.py, UpCat.forward, is_pad=True; call site
// inference/inference.py:190-197): a level whose skip tensor has an ODD size gets an up-sampled tensor that is one voxel short in
// that dimension (2 * floor(n / 2) = n - 1); it is padded by one at the far end with the edge value.  Windows whose dimensions
// are multiples of 16 never come here.  Chunk-planar tensors: [n][C/8][D][H][W] of uint4.
__global__ void __launch_bounds__(256) replicate_pad_cp_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, int Di, int Hi, int Wi,
                                                               int Do, int Ho, int Wo) {
    const long long vo = (long long)Do * Ho * Wo, vi = (long long)Di * Hi * Wi;
    const long long plane = blockIdx.y;  // (n, chunk)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vo; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), z = (int)(i / ((long long)Wo * Ho));
        out[plane * vo + i] = in[plane * vi + ((long long)min(z, Di - 1) * Hi + min(y, Hi - 1)) * Wi + min(x, Wi - 1)];
    }
}

template <class P>
__global__ void f32_to_cp_kernel(const float* __restrict__ in, uint4* __restrict__ out, int C, long long vox) {
    const int c8 = blockIdx.y, n = blockIdx.z;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vox; i += (long long)gridDim.x * 256) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = in[((long long)n * C + c8 * 8 + k) * vox + i];
        uint4 r;
        r.x = P::pack2(v[0], v[1]);
        r.y = P::pack2(v[2], v[3]);
        r.z = P::pack2(v[4], v[5]);
        r.w = P::pack2(v[6], v[7]);
        out[((long long)n * (C / 8) + c8) * vox + i] = r;
    }
}
template <class P>
__global__ void cp_to_f32_kernel(const uint4* __restrict__ in, float* __restrict__ out, int C, long long vox) {
    const int c8 = blockIdx.y, n = blockIdx.z;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vox; i += (long long)gridDim.x * 256) {
        const uint4 u = in[((long long)n * (C / 8) + c8) * vox + i];
        const float v[8] = {P::lo(u.x), P::hi(u.x), P::lo(u.y), P::hi(u.y), P::lo(u.z), P::hi(u.z), P::lo(u.w), P::hi(u.w)};
#pragma unroll
        for (int k = 0; k < 8; ++k) out[((long long)n * C + c8 * 8 + k) * vox + i] = v[k];
    }
}

}  // namespace
