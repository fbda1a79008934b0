// unet16_stem.h - the two stem kernels (Conv3d 1 -> 32): fp32 on the VALU and the MFMA kernel on the uint16 volume.
// A fragment of unet_bf16.hip, which alone includes it (after common.h, prec16.h and its Mish helpers): one translation unit,
// one object, the flags of that file.
#pragma once
namespace {

// ---------------------------------------------------------------------------------------------------
// stem: Conv3d(1 -> C0, k3, p1) in fp32 on the VALU, straight from the uint16 volume window
// (gather + cast + flip of inference/sliding_window_inferer.py:181-195,218-219 fused in) or from an
// fp32 patch.  Writes raw (pre-norm) bf16 + per-block partial sums for the InstanceNorm.
// ---------------------------------------------------------------------------------------------------
constexpr int STEM_ZR = 4;  // z-run per thread

template <class P, bool FROM_VOLUME>
__global__ void __launch_bounds__(256) stem_conv_kernel(const float* __restrict__ xf, const uint16_t* __restrict__ vol,
                                                        int Yp, int Xp, const int* __restrict__ starts, int flip_dim,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        uint4* __restrict__ out, float* __restrict__ partials, int D,
                                                        int H, int W, float oscale) {
    __shared__ float wl[27 * 32];
    __shared__ float red[4][64];
    for (int i = threadIdx.x; i < 27 * 32; i += 256) {
        const int t = i >> 5, co = i & 31;
        wl[i] = w[co * 27 + t];
    }
    __syncthreads();
    const int n = blockIdx.z;
    const int hw = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool pvalid = p < hw;
    const int y = pvalid ? p / W : 0, x = pvalid ? p % W : 0;
    const int zb = blockIdx.y * STEM_ZR;
    int z0 = 0, y0 = 0, x0 = 0;
    if (FROM_VOLUME) {
        z0 = starts[3 * n];
        y0 = starts[3 * n + 1];
        x0 = starts[3 * n + 2];
    }
    auto fetch = [&](int zz, int yy, int xx) -> float {
        if ((unsigned)zz >= (unsigned)D || (unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) return 0.f;
        if (FROM_VOLUME) {
            if (flip_dim == 2) zz = D - 1 - zz;
            if (flip_dim == 3) yy = H - 1 - yy;
            if (flip_dim == 4) xx = W - 1 - xx;
            return (float)vol[((long long)(z0 + zz) * Yp + (y0 + yy)) * Xp + (x0 + xx)];
        }
        return xf[(long long)n * D * hw + ((long long)zz * H + yy) * W + xx];
    };
    float s[32], q[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) s[c] = q[c] = 0.f;
#pragma unroll 1
    for (int zi = 0; zi < STEM_ZR; ++zi) {
        const int z = zb + zi;
        if (z >= D || !pvalid) continue;
        float acc[32];
#pragma unroll
        for (int c = 0; c < 32; ++c) acc[c] = bias[c];
#pragma unroll 1
        for (int dz = 0; dz < 3; ++dz)
#pragma unroll 1
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = fetch(z + dz - 1, y + dy - 1, x + dx - 1);
                    const float4* wr = reinterpret_cast<const float4*>(wl + ((dz * 3 + dy) * 3 + dx) * 32);
#pragma unroll
                    for (int c4 = 0; c4 < 8; ++c4) {
                        const float4 ww = wr[c4];
                        acc[4 * c4 + 0] = fmaf(v, ww.x, acc[4 * c4 + 0]);
                        acc[4 * c4 + 1] = fmaf(v, ww.y, acc[4 * c4 + 1]);
                        acc[4 * c4 + 2] = fmaf(v, ww.z, acc[4 * c4 + 2]);
                        acc[4 * c4 + 3] = fmaf(v, ww.w, acc[4 * c4 + 3]);
                    }
                }
        if (oscale != 1.0f) {  // (STEM_SCALE * 2^-shift of layer 0)
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] *= oscale;
        }
        const long long vox = (long long)D * hw;
        const long long o = (long long)z * hw + p;
#pragma unroll
        for (int c8 = 0; c8 < 4; ++c8) {
            uint4 u;
            u.x = P::pack2(acc[8 * c8 + 0], acc[8 * c8 + 1]);
            u.y = P::pack2(acc[8 * c8 + 2], acc[8 * c8 + 3]);
            u.z = P::pack2(acc[8 * c8 + 4], acc[8 * c8 + 5]);
            u.w = P::pack2(acc[8 * c8 + 6], acc[8 * c8 + 7]);
            out[((long long)n * 4 + c8) * vox + o] = u;
        }
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            s[c] += acc[c];
            q[c] = fmaf(acc[c], acc[c], q[c]);
        }
    }
    // block reduction -> partials[n][block][32][2]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
        float a = s[c], b = q[c];
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
        }
        if (lane == 0) {
            red[wave][2 * c] = a;
            red[wave][2 * c + 1] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
        const long long nblk = (long long)gridDim.x * gridDim.y;
        partials[((long long)n * nblk + blk) * 64 + threadIdx.x] = v;
    }
}

// ---------------------------------------------------------------------------------------------------
// MFMA stem for the fused sliding-window path: the uint16 window is staged (with flip and the
// zero padding of the window border) as a halo tile in LDS, every voxel already split into its (lo, hi) bytes as a
// pair of 16-bit floats (exact in bf16 and fp16); every lane gathers the taps of its voxel - one ds_read_b32 per tap
// is one register of the operand, no VALU - and feeds 4 MFMAs (K = 64) per 32-voxel block.
//   workgroup: 4 (z) x 8 (y) x 32 (x) output voxels; wave w = z-slice w, 8 row blocks
// ---------------------------------------------------------------------------------------------------
constexpr int SM_TZ = 4, SM_TY = 8, SM_TX = 32, SM_HZ = 6, SM_HY = 10, SM_HX = 34;
constexpr int SM_ZC = 8;                                   // z-chunks of SM_TZ planes one workgroup walks
constexpr int SM_NT = SM_HZ * SM_HY * SM_HX;               // halo tile voxels
constexpr int SM_NS = (SM_NT + 255) / 256;                 // staged voxels per thread

// MODE 0: store raw + statistics; MODE 1: statistics only (first pass of the two-pass stem); MODE 2: recompute,
// apply InstanceNorm scale/shift + Mish and store the ACTIVATED tensor (no raw tensor, no separate norm pass:
// the K = 64 MFMA work is cheap next to 268 MB of avoided traffic per 128^3 window).
// A workgroup owns an 8 x 32 (y, x) column and walks SM_ZC chunks of 4 planes: the per-thread staging addresses, the
// weights and the statistics registers are set up once per 8192 voxels, the halo tile is double-buffered (the loads of
// the next chunk fly during the MFMAs of this one, one barrier per chunk), one reduction at the end.
template <class P, int MODE>
__global__ void __launch_bounds__(256) stem_mfma_kernel(const uint16_t* __restrict__ vol, int Yp, int Xp,
                                                        const int* __restrict__ starts, int flip_dim,
                                                        const uint4* __restrict__ wpk, const float* __restrict__ bias,
                                                        uint4* __restrict__ out, float* __restrict__ partials,
                                                        const float2* __restrict__ ss, int D, int H, int W, int tilesY,
                                                        int tilesX) {
    // the halo tile, already split: word = (lo byte, hi byte) of the voxel as two 16-bit floats (exact in bf16 and fp16)
    __shared__ unsigned tile[2][SM_NT];
    __shared__ float red[4 * 64];
    const int n = blockIdx.z;
    const int t = dlv_xcd_tile(blockIdx.x, gridDim.x);
    const int tx = t % tilesX, ty = (t / tilesX) % tilesY, tg = t / (tilesX * tilesY);
    const int zbase = tg * (SM_ZC * SM_TZ), y0 = ty * SM_TY, x0 = tx * SM_TX;
    const int nzc = min(SM_ZC, (D - zbase + SM_TZ - 1) / SM_TZ);
    const int wz = starts[3 * n], wy = starts[3 * n + 1], wx = starts[3 * n + 2];
    // this thread's staged voxels: in-plane offset into the volume (window origin, flip and y/x validity folded in) and
    // the halo plane; only the z coordinate moves from chunk to chunk
    int soff[SM_NS], szh[SM_NS];
#pragma unroll
    for (int k = 0; k < SM_NS; ++k) {
        const int i = threadIdx.x + 256 * k;
        const int xh = i % SM_HX, yh = (i / SM_HX) % SM_HY, zh = i / (SM_HX * SM_HY);
        int gy = y0 + yh - 1, gx = x0 + xh - 1;
        const bool ok = i < SM_NT && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        if (flip_dim == 3) gy = H - 1 - gy;
        if (flip_dim == 4) gx = W - 1 - gx;
        soff[k] = ok ? (wy + gy) * Xp + (wx + gx) : -1;
        szh[k] = zh - 1;
    }
    const long long plane = (long long)Yp * Xp;
    unsigned sv[SM_NS];
    auto stage_load = [&](int zc) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < SM_NS; ++k) {
            int gz = zbase + zc * SM_TZ + szh[k];
            const bool ok = soff[k] >= 0 && (unsigned)gz < (unsigned)D;
            if (flip_dim == 2) gz = D - 1 - gz;
            sv[k] = ok ? (unsigned)vol[(long long)(wz + gz) * plane + soff[k]] : 0u;
        }
    };
    auto stage_store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < SM_NS; ++k) {
            const int i = threadIdx.x + 256 * k;
            if (i < SM_NT) tile[buf][i] = P::pack2((float)(sv[k] & 255u), (float)(sv[k] >> 8));
        }
    };
    stage_load(0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    uint4 a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = AS_FRAG(wpk[s * 64 + lane]);
    // No conv bias: the InstanceNorm that follows removes it, and statistics summed in fp32 without it stay exact where the
    // raw output is (nearly) constant - a background window's raw output is the bias alone, whose E[x^2] - E[x]^2 in fp32
    // left a variance of ~1e-6 b^2 (the scale 1.5e-3 off at eps 1e-5: tests/test_gpu_conv_kernels.py)
    const f32x16 bsv = {};
    float ssum[16], ssq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ssum[r] = ssq[r] = 0.f;
    float nsc[16], nsh[16];
    if (MODE == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float2 v = ss[n * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
            nsc[r] = v.x;
            nsh[r] = v.y;
        }
    }
    stage_store(0);
    __syncthreads();
    const long long vox = (long long)D * H * W;
    // per-lane LDS offsets of this lane's 16 taps (k-step s, register q: tap 8s + 4h + q), row 0 of buffer 0; the row
    // loop is unrolled so that the row offset is an immediate of the ds_read_b32
    int tap_off[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int tp = 8 * (i >> 2) + 4 * h + (i & 3);
        const int tt = tp < 27 ? tp : 0;  // padding slots: any finite value (their weights are 0)
        tap_off[i] = (wave * SM_HY * SM_HX + col) + ((tt / 9) * SM_HY + (tt / 3) % 3) * SM_HX + tt % 3;
    }
#pragma unroll 1
    for (int zc = 0; zc < nzc; ++zc) {
        if (zc + 1 < nzc) stage_load(zc + 1);
        const unsigned* tl = tile[zc & 1];
        const int oz = zbase + zc * SM_TZ + wave;
#pragma unroll
        for (int row = 0; row < SM_TY; ++row) {
            unsigned b[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) b[i] = tl[tap_off[i] + row * SM_HX];
            f32x16 acc = P::mfma(a[0], AS_FRAG(make_uint4(b[0], b[1], b[2], b[3])), bsv, 0, 0, 0);
            acc = P::mfma(a[1], AS_FRAG(make_uint4(b[4], b[5], b[6], b[7])), acc, 0, 0, 0);
            acc = P::mfma(a[2], AS_FRAG(make_uint4(b[8], b[9], b[10], b[11])), acc, 0, 0, 0);
            acc = P::mfma(a[3], AS_FRAG(make_uint4(b[12], b[13], b[14], b[15])), acc, 0, 0, 0);
            const int oy = y0 + row, ox = x0 + col;
            const bool ok = oz < D && oy < H && ox < W;
            float val[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) val[r] = acc[r];
            if (MODE != 2 && ok) {  // one exec-masked block (per-element selects cost two v_cndmask per value)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    ssum[r] += val[r];
                    ssq[r] = fmaf(val[r], val[r], ssq[r]);
                }
            }
            if (MODE == 2) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const f32x2_t m = mish_fast2(fma2(f32x2_t{val[r], val[r + 1]}, f32x2_t{nsc[r], nsc[r + 1]}, f32x2_t{nsh[r], nsh[r + 1]}));
                    val[r] = m.x;
                    val[r + 1] = m.y;
                }
            }
            if (MODE != 1 && ok) {
                const long long o = ((long long)oz * H + oy) * W + ox;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 u;
                    u.x = P::pack2(val[4 * g + 0], val[4 * g + 1]);
                    u.y = P::pack2(val[4 * g + 2], val[4 * g + 3]);
                    uint2* dst = reinterpret_cast<uint2*>(out + ((long long)n * 4 + g) * vox + o);
                    dlv_st8<true>(dst + h, u);
                }
            }
        }
        if (zc + 1 < nzc) stage_store((zc + 1) & 1);
        __syncthreads();
    }
    if (MODE == 2) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float sa = ssum[r], sb = ssq[r];
        sa = dlv_half_sum32(sa);  // DPP adds; totals valid in lanes 16-31 / 48-63
        sb = dlv_half_sum32(sb);
        if (col == 31) {
            const int co = (r & 3) + 8 * (r >> 2) + 4 * h;
            red[(wave * 32 + co) * 2] = sa;
            red[(wave * 32 + co) * 2 + 1] = sb;
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int i = threadIdx.x;
        partials[((long long)n * gridDim.x + t) * 64 + i] = red[i] + red[64 + i] + red[128 + i] + red[192 + i];
    }
}

}  // namespace
