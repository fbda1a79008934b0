// unet16_conv.h - the generic 3x3x3 MFMA conv kernel.
// A fragment of unet_bf16.hip, which alone includes it (after common.h, prec16.h and its Mish helpers): one translation unit,
// one object, the flags of that file.
#pragma once
namespace {

// ---------------------------------------------------------------------------------------------------
// generic 3x3x3 convolution, implicit GEMM on MFMA
//   workgroup: 256 output voxels (4 z-slices x 64 voxels) x 32*NCB output channels
//   wave w   : z-slice w, two 32-voxel blocks, NCB cout blocks  -> 2*NCB accumulator tiles
//   loop     : input channels in slabs of 32 (halo tile staged in LDS) x 27 taps x 2 k-steps
// ---------------------------------------------------------------------------------------------------
template <int TX>
struct ConvTile {
    static constexpr int TZ = 4;
    static constexpr int TY = 64 / TX;       // 4 (TX=16) or 8 (TX=8)
    static constexpr int HZ = TZ + 2, HY = TY + 2, HX = TX + 2;
    static constexpr int SLAB = 4 * HZ * HY * HX;  // uint4 elements per 32-channel slab
    static constexpr int RV = 32 / TX;       // rows per 32-voxel block
};

template <class P, int NCB, int TX, bool WLDS>
__global__ void __launch_bounds__(256) conv3_mfma_kernel(const uint4* __restrict__ in1, int c1_8,
                                                         const uint4* __restrict__ in2, int c2_8,
                                                         const uint4* __restrict__ wpk, const float* __restrict__ bias,
                                                         uint4* __restrict__ out, float* __restrict__ partials, int cout,
                                                         int D, int H, int W, int tilesY, int tilesX) {
    using T = ConvTile<TX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4* slab = reinterpret_cast<uint4*>(smem_raw);
    uint4* wlds = slab + T::SLAB;  // WLDS: this slab's weights, [cb][tap][k-step][lane]
    const int n = blockIdx.z;
    const int tile = dlv_xcd_tile(blockIdx.x, gridDim.x);
    const int tx = tile % tilesX, ty = (tile / tilesX) % tilesY, tz = tile / (tilesX * tilesY);
    const int z0 = tz * T::TZ, y0 = ty * T::TY, x0 = tx * TX;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const int vr = col / TX, vx = col % TX;  // row / x of this lane's voxel inside a 32-voxel block
    const int cin8 = c1_8 + c2_8;
    const int KP = cin8 / 2;
    const int cbg0 = blockIdx.y * NCB;
    const long long vox = (long long)D * H * W;

    f32x16 acc[NCB][2];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][v][r] = 0.f;

    // per-lane LDS element offset of tap (0,0,0) for the two voxel blocks, chunk h of k-step 0
    int lbase[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) lbase[v] = ((h * T::HZ + wave) * T::HY + (v * T::RV + vr)) * T::HX + vx;

    const int nslab = cin8 / 4;
    // staging map of one 32-channel slab (the same for every slab: only the base pointer moves): element i of the
    // halo tile <- chunk c, voxel (gz,gy,gx).  The next slab is fetched into registers while the current one is being
    // multiplied (issue early / write late), so the HBM/L2 latency of the staging no longer sits between two MFMA phases.
    constexpr int NPF = (T::SLAB + 255) / 256;
    int poff[NPF];
    unsigned pvalid = 0;
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
        const int i = threadIdx.x + 256 * j;
        poff[j] = 0;
        if (i < T::SLAB) {
            const int xh = i % T::HX;
            int r = i / T::HX;
            const int yh = r % T::HY;
            r /= T::HY;
            const int zh = r % T::HZ;
            const int c = r / T::HZ;
            const int gz = z0 + zh - 1, gy = y0 + yh - 1, gx = x0 + xh - 1;
            if ((unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
                poff[j] = (int)((long long)c * vox + ((long long)gz * H + gy) * W + gx);
                pvalid |= 1u << j;
            }
        }
    }
    uint4 pf[NPF];
    auto fetch_slab = [&](int sl) __attribute__((always_inline)) {
        const int cg = sl * 4;  // a 32-channel slab lies entirely in one of the two sources (c1 % 32 == 0)
        const uint4* src = cg < c1_8 ? in1 + ((long long)n * c1_8 + cg) * vox : in2 + ((long long)n * c2_8 + (cg - c1_8)) * vox;
#pragma unroll
        for (int j = 0; j < NPF; ++j) pf[j] = src[poff[j]];
    };
    fetch_slab(0);
    // weight fragments straight from L2 (!WLDS) run through a rolling queue PD k-steps deep that continues across slab
    // boundaries: the load of step g + PD is issued when step g's fragments are consumed, so an L2 round trip is covered
    // by PD groups of MFMAs instead of sitting in front of each group (128^3 windows, 16 per launch: 128+128->64 at 32^3
    // 357 -> 296 us, 256->128 at 16^3 196 -> 166 us).  The same queue for the LDS operand made it slower (registers).
    constexpr int PD = WLDS ? 1 : (NCB >= 4 ? 2 : 6);  // 54 k-steps per slab: PD divides 54 (NCB 4: 256 VGPRs allow no more)
    uint4 aq[PD][NCB];
    const long long nsteps = (long long)nslab * 54;
    auto wfetch = [&](long long g, uint4 (&dst)[NCB]) __attribute__((always_inline)) {
        const int sl2 = (int)(g / 54), st = (int)(g % 54);
        const int t = st >> 1, kp = sl2 * 2 + (st & 1);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) dst[cb] = wpk[(((long long)(cbg0 + cb) * 27 + t) * KP + kp) * 64 + lane];
    };
    if (!WLDS) {
#pragma unroll
        for (int q = 0; q < PD; ++q)
            if (q < nsteps) wfetch(q, aq[q]);
    }
    for (int sl = 0; sl < nslab; ++sl) {
        __syncthreads();  // previous slab fully consumed
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < T::SLAB) slab[i] = ((pvalid >> j) & 1u) ? pf[j] : make_uint4(0, 0, 0, 0);
        }
        if (WLDS) {
            // the slab's weights are fetched cooperatively in one coalesced sweep (deep levels have few
            // workgroups: per-k-step fragment loads from L2 are latency-bound there)
            for (int i = threadIdx.x; i < NCB * 27 * 2 * 64; i += 256) {
                const int l = i & 63, ks = (i >> 6) & 1, r = i >> 7;
                const int t = r % 27, cb = r / 27;
                wlds[i] = wpk[(((long long)(cbg0 + cb) * 27 + t) * KP + sl * 2 + ks) * 64 + l];
            }
        }
        __syncthreads();
        if (sl + 1 < nslab) fetch_slab(sl + 1);  // in flight during this slab's MFMAs
#pragma unroll
        for (int kz = 0; kz < 3; ++kz)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int t = (kz * 3 + ky) * 3 + kx;
                    const int toff = (kz * T::HY + ky) * T::HX + kx;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const int st = t * 2 + ks;
                        uint4 a[NCB];
#pragma unroll
                        for (int cb = 0; cb < NCB; ++cb)
                            a[cb] = AS_FRAG(WLDS ? wlds[((cb * 27 + t) * 2 + ks) * 64 + lane] : aq[st % PD][cb]);
                        if (!WLDS) {
                            const long long g = (long long)sl * 54 + st + PD;
                            if (g < nsteps) wfetch(g, aq[st % PD]);
                        }
                        uint4 b[2];
#pragma unroll
                        for (int v = 0; v < 2; ++v) {
                            const uint4 u = slab[lbase[v] + toff + ks * 2 * T::HZ * T::HY * T::HX];
                            b[v] = AS_FRAG(u);
                        }
#pragma unroll
                        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                            for (int v = 0; v < 2; ++v)
                                acc[cb][v] = P::mfma(a[cb], b[v], acc[cb][v], 0, 0, 0);
                    }
                }
    }

    // ---- epilogue: bias, bf16 store, InstanceNorm partial sums -------------------------------------
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem_raw);  // [4 waves][NCB*32][2]
    const int oz = z0 + wave;
    const int cout8 = cout / 8;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        float bs[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bs[r] = bias[(cbg0 + cb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
        float s[16], q[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = q[r] = 0.f;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int oy = y0 + v * T::RV + vr, ox = x0 + vx;
            const bool ok = oz < D && oy < H && ox < W;
            float val[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                val[r] = acc[cb][v][r] + bs[r];
                if (ok) {
                    s[r] += val[r];
                    q[r] = fmaf(val[r], val[r], q[r]);
                }
            }
            if (ok) {
                const long long o = ((long long)oz * H + oy) * W + ox;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 u;
                    u.x = P::pack2(val[4 * g + 0], val[4 * g + 1]);
                    u.y = P::pack2(val[4 * g + 2], val[4 * g + 3]);
                    uint2* dst = reinterpret_cast<uint2*>(out + ((long long)n * cout8 + (cbg0 + cb) * 4 + g) * vox + o);
                    dst[h] = u;
                }
            }
        }
        // reduce over the 32 voxels (lanes with equal h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float a = s[r], b = q[r];
            a = dlv_half_sum32(a);  // DPP adds; totals valid in lanes 16-31 / 48-63
            b = dlv_half_sum32(b);
            if (col == 31) {
                const int co = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                red[(wave * NCB * 32 + co) * 2] = a;
                red[(wave * NCB * 32 + co) * 2 + 1] = b;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < NCB * 32 * 2) {
        const int i = threadIdx.x;
        const float v = red[i] + red[NCB * 64 + i] + red[2 * NCB * 64 + i] + red[3 * NCB * 64 + i];
        const int co = cbg0 * 32 + (i >> 1);
        partials[(((long long)n * gridDim.x + tile) * cout + co) * 2 + (i & 1)] = v;
    }
}

}  // namespace
