// conv_zmarch.hip - the LDS-resident-weights 3x3x3 convolution (Cin = 32 or 64 = 32+32, Cout a multiple of 32) as a
// z-marching, input-stationary implicit GEMM on v_mfma_f32_32x32x16_{f16,bf16}.  layer_plan.h (plan_conv) gives it the
// layers of the <= 32768-voxel level that the deep-level kernels leave, and every z-reg layer under the A/B switch
// zm_variant = 51.
//
// One workgroup (8 waves, one output row each) owns an (8 rows x 32 columns) in-plane tile of one sample and marches
// along z ("z-major slabs"): for every input plane p it
//     - has the halo plane (10 x 34 voxels x Cin channels) in LDS, staged through registers from the
//       coalesced chunk-planar tensor while the previous plane is being computed (issue-early /
//       write-late),
//     - multiplies it with ALL 27 taps: the kz = 0/1/2 slices of the weights feed three rotating
//       accumulators (output planes p+1, p, p-1), so each input fragment read from LDS is used by
//       three MFMAs and only ONE plane has to be resident,
//     - emits output plane p-1 (bias, 16-bit store, InstanceNorm partial sums kept per lane and
//       reduced once per 16 planes).
// The complete weight set (27 x Cin x 32 x 16 bit = 54 / 108 KiB) is LDS-resident in MFMA A-fragment
// order.  LDS reads per MFMA: 1.33 x ds_read_b128 (one plane fragment + three weight fragments per three MFMAs).
#include <algorithm>

#include "common.h"
#include "prec16.h"

namespace {

constexpr int ZM_TY = 8, ZM_TX = 32, ZM_HX = 34;  // tile rows (one per wave) and columns, halo-plane row length

template <int CIN>
struct ZmCfg {
    static constexpr int HY = ZM_TY + 2;
    static constexpr int PLANE = HY * ZM_HX;     // halo plane voxels
    static constexpr int C8 = CIN / 8;           // chunks
    static constexpr int KP = CIN / 16;          // k-steps per tap
    static constexpr int WELEMS = 27 * KP * 64;  // uint4 elements of weights in LDS
    static constexpr int PELEMS = C8 * PLANE; // uint4 elements of one halo plane
    static constexpr size_t LDS_BYTES = (size_t)(WELEMS + PELEMS) * 16 + 2048;  // + 8x64 floats for the stats flush
};

template <class P, int CIN>
__global__ void __launch_bounds__(64 * ZM_TY, 2) conv3_zmarch_kernel(const uint4* __restrict__ in1, int c1_8,
                                                           const uint4* __restrict__ in2, int c2_8,
                                                           const uint4* __restrict__ wpk, const float* __restrict__ bias,
                                                           uint4* __restrict__ out, float* __restrict__ partials, int D,
                                                           int H, int W, int tilesY, int tilesX, int zseg, int nseg, int cout8) {
    using C = ZmCfg<CIN>;
    constexpr int NT = 64 * ZM_TY;               // threads: one wave per tile row
    constexpr int NPRE = (C::PELEMS + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4* lds_w = reinterpret_cast<uint4*>(smem_raw);
    uint4* lds_p = lds_w + C::WELEMS;
    float* red = reinterpret_cast<float*>(lds_p + C::PELEMS);  // [8 waves][32][2]

    const int n = blockIdx.z;
    // blockIdx.y = z segment + nseg * output-channel block (32 channels each; Cout = 64 layers run two blocks
    // over the same input)
    const int seg = blockIdx.y % nseg, cb = blockIdx.y / nseg;
    const int tile = dlv_xcd_tile(blockIdx.x, gridDim.x);
    const int tx = tile % tilesX, ty = tile / tilesX;
    const int y0 = ty * ZM_TY, x0 = tx * ZM_TX;
    const int zs = seg * zseg, ze = min(zs + zseg, D);  // output planes [zs, ze)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;
    const long long plane = (long long)H * W;
    const long long vox = (long long)D * plane;

    // ---- weights -> LDS (A-fragment order, lane-linear) ------------------------------------------------
    for (int i = threadIdx.x; i < C::WELEMS; i += NT) lds_w[i] = wpk[(size_t)cb * C::WELEMS + i];

    // ---- per-thread staging map of the halo plane (constant along z) ----------------------------------
    long long goff[NPRE];
    unsigned valid = 0;
#pragma unroll
    for (int j = 0; j < NPRE; ++j) {
        const int i = threadIdx.x + NT * j;
        goff[j] = -1;
        if (i < C::PELEMS) {
            const int xh = i % ZM_HX, yh = (i / ZM_HX) % C::HY, c = i / C::PLANE;
            const int gy = y0 + yh - 1, gx = x0 + xh - 1;
            if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
                const long long base = c < c1_8 ? ((long long)n * c1_8 + c) * vox : ((long long)n * c2_8 + (c - c1_8)) * vox;
                goff[j] = base + (long long)gy * W + gx;
                valid |= 1u << j;
            }
        }
    }
    auto src_of = [&](int j) -> const uint4* {
        const int c = (threadIdx.x + NT * j) / C::PLANE;
        return c < c1_8 ? in1 : in2;
    };
    uint4 pre[NPRE];
    // loads are unconditional (invalid lanes read element 0 of their source and are zeroed by a select):
    // no exec-masked branch per load, all of a plane's loads are in flight together
    auto issue_loads = [&](int p) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const bool ok = (valid >> j) & 1u;
            const uint4* src = ok ? src_of(j) : in1;  // lanes without an element read (and discard) in1[0]
            pre[j] = src[ok ? goff[j] + (long long)p * plane : 0];
        }
    };
    // the zero-select of out-of-window lanes happens here, at the first use of the loaded registers, so
    // that the wait for the loads sits in front of the LDS write and not in front of the MFMAs
    auto write_plane = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int i = threadIdx.x + NT * j;
            const bool ok = (valid >> j) & 1u;
            if (i < C::PELEMS) lds_p[i] = ok ? pre[j] : make_uint4(0, 0, 0, 0);
        }
    };

    // per-lane LDS offset: this lane's voxel (row = wave, column col), chunk half h
    const int lb = (h * C::HY + wave) * ZM_HX + col;

    f32x16 fzero;
#pragma unroll
    for (int r = 0; r < 16; ++r) fzero[r] = 0.f;
    f32x16 a0, a1, a2;
#pragma unroll
    for (int r = 0; r < 16; ++r) a0[r] = a1[r] = a2[r] = 0.f;
    float bs[16], ssum[16], ssq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        bs[r] = bias[cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
        ssum[r] = ssq[r] = 0.f;
    }

    // InstanceNorm partial sums are flushed every 16 output planes (absolute z / 16), so that their
    // grouping - and with it every bit of the statistics - does not depend on zseg or the batch size
    const int nzc = (D + 15) / 16;
    auto flush_stats = [&](int zc) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float a = ssum[r], b = ssq[r];
            a = dlv_half_sum32(a);  // DPP adds; totals valid in lanes 16-31 / 48-63
            b = dlv_half_sum32(b);
            if (col == 31) {
                const int co = (r & 3) + 8 * (r >> 2) + 4 * h;
                red[(wave * 32 + co) * 2] = a;
                red[(wave * 32 + co) * 2 + 1] = b;
            }
            ssum[r] = ssq[r] = 0.f;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int i = threadIdx.x;
            float v = 0.f;
#pragma unroll
            for (int w8 = 0; w8 < ZM_TY; ++w8) v += red[w8 * 64 + i];
            const long long nparts = (long long)gridDim.x * nzc;
            const long long part = (long long)zc * gridDim.x + tile;
            partials[(((long long)n * nparts + part) * (cout8 * 8) + cb * 32 + (i >> 1)) * 2 + (i & 1)] = v;
        }
        __syncthreads();
    };

    // output plane oz from its finished accumulator: bias, statistics, 16-bit store
    auto epilogue = [&](f32x16& acc, int oz) __attribute__((always_inline)) {
        const bool emit = oz >= zs && oz < ze;
        const int oy = y0 + wave, ox = x0 + col;
        const bool ok = emit && oy < H && ox < W;
        float val[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            val[r] = acc[r] + bs[r];
            if (ok) {
                ssum[r] += val[r];
                ssq[r] = fmaf(val[r], val[r], ssq[r]);
            }
        }
        if (ok) {
            const long long o = (long long)oz * plane + (long long)oy * W + ox;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 u;
                u.x = P::pack2(val[4 * g + 0], val[4 * g + 1]);
                u.y = P::pack2(val[4 * g + 2], val[4 * g + 3]);
                uint2* dst = reinterpret_cast<uint2*>(out + ((long long)n * cout8 + cb * 4 + g) * vox + o);
                dst[h] = u;
            }
        }
    };

    // one z step: plane p is in LDS (when 0 <= p < D).  kz=2 -> accA (out[p-1]), kz=1 -> accB (out[p]),
    // kz=0 -> accC (out[p+1], started here).  Then out[p-1] is emitted from accA.
    auto step = [&](int p, f32x16& accA, f32x16& accB, f32x16& accC) __attribute__((always_inline)) {
        const bool next_needed = (p + 1 <= ze) && (p + 1 >= 0) && (p + 1 < D);
        if (next_needed) issue_loads(p + 1);
        if (p >= 0 && p < D && p <= ze) {
            // software-pipelined over the 9*KP (ky,kx,ks) groups: the 4 LDS fragment reads of group g+1
            // are issued before the 3 MFMAs of group g
            constexpr int NG = 9 * C::KP;
            uint4 fb[2], fw[2][3];
            auto load_group = [&](int g, uint4& b, uint4(&w)[3]) __attribute__((always_inline)) {
                const int ks = g % C::KP, kx = (g / C::KP) % 3, ky = g / (3 * C::KP);
                b = lds_p[lb + (ks * 2 * C::HY + ky) * ZM_HX + kx];
#pragma unroll
                for (int kz = 0; kz < 3; ++kz) w[kz] = lds_w[(((kz * 3 + ky) * 3 + kx) * C::KP + ks) * 64 + lane];
            };
            load_group(0, fb[0], fw[0]);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int cur = g % 2;
                if (g + 1 < NG) load_group(g + 1, fb[(g + 1) % 2], fw[(g + 1) % 2]);
                // pin the order: left alone, hipcc sinks every ds_read next to its MFMA (read, wait, mfma),
                // which exposes the full LDS latency on each MFMA
                __builtin_amdgcn_sched_barrier(0);
                const uint4 bv = fb[cur];
                // accC starts a new output plane: its first MFMA takes a zero C operand
                accC = P::mfma(fw[cur][0], bv, g == 0 ? fzero : accC, 0, 0, 0);
                accB = P::mfma(fw[cur][1], bv, accB, 0, 0, 0);
                accA = P::mfma(fw[cur][2], bv, accA, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            accC = fzero;
        }
        epilogue(accA, p - 1);
        const int ozf = p - 1;
        if (ozf >= zs && ozf < ze && ((ozf & 15) == 15 || ozf == ze - 1)) flush_stats(ozf >> 4);
        __syncthreads();  // every wave is done reading plane p
        if (next_needed) write_plane();
        __syncthreads();
    };

    // prologue: first input plane of the segment (zs-1, or zs when zs == 0)
    {
        const int p0 = zs - 1;
        if (p0 >= 0) {
            issue_loads(p0);
            write_plane();
        }
        __syncthreads();
    }
    // steps beyond ze are no-ops (compute, loads and emit are all guarded), so the triple needs no branches
    for (int p = zs - 1; p <= ze; p += 3) {
        step(p, a0, a1, a2);
        step(p + 1, a1, a2, a0);
        step(p + 2, a2, a0, a1);
    }
}

// one instantiation: the attribute that lets a workgroup take more than 64 KiB of LDS is set once per device
template <class P, int CIN>
int launch(dlv_ctx* ctx, dim3 grid, const void* in1, int c1, const void* in2, int c2, const void* wpk, const float* bias, void* out,
           float* partials, int D, int H, int W, int tilesY, int tilesX, int zseg, int nseg, int cout) {
    static dlv_attr_bits attr_set{0};  // bit per device
    if (!dlv_attr_is_set(attr_set, ctx->device)) {
        DLV_HIP(ctx, hipFuncSetAttribute((const void*)conv3_zmarch_kernel<P, CIN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)ZmCfg<CIN>::LDS_BYTES));
        dlv_attr_mark(attr_set, ctx->device);
    }
    hipLaunchKernelGGL((conv3_zmarch_kernel<P, CIN>), grid, dim3(64 * ZM_TY), ZmCfg<CIN>::LDS_BYTES, ctx->stream, (const uint4*)in1,
                       c1 / 8, (const uint4*)in2, c2 / 8, (const uint4*)wpk, bias, (uint4*)out, partials, D, H, W, tilesY, tilesX, zseg,
                       nseg, cout / 8);
    DLV_LAUNCH_CHECK(ctx, "conv3_zmarch_kernel");
    return DLV_OK;
}

}  // namespace

// *nparts: the number of partial-sum rows per sample; returns DLV_OK or a negative error
int dlv_conv3_zmarch_launch(dlv_ctx* ctx, bool f16, int cin, int cout, const void* in1, int c1, const void* in2, int c2,
                            const void* wpk, const float* bias, void* out, float* partials, int B, int D, int H, int W,
                            int* nparts) {
    if (cout % 32 || cout <= 0) return dlv_fail(ctx, DLV_EUNSUP, "z-march conv: Cout must be a multiple of 32");
    const int ncb = cout / 32;
    const int tilesY = dlv_cdiv(H, ZM_TY), tilesX = dlv_cdiv(W, ZM_TX);
    // split long columns (in multiples of 16 planes) so that small batches still fill 256 CUs
    int zseg = ((D + 15) / 16) * 16;
    while ((long long)B * tilesY * tilesX * ncb * dlv_cdiv(D, zseg) < 512 && zseg > 16) zseg = std::max(16, ((zseg / 2 + 15) / 16) * 16);
    const int nseg = dlv_cdiv(D, zseg);
    dim3 grid(tilesY * tilesX, nseg * ncb, B);
    *nparts = tilesY * tilesX * ((D + 15) / 16);
    ctx->ran.conv = DLV_PLAN_ZMARCH;
    ctx->ran.ncb = ncb;
    ctx->ran.grid = (int)(grid.x * grid.y * grid.z);
    if (cin != 32 && cin != 64) return dlv_fail(ctx, DLV_EUNSUP, "z-march conv: Cin must be 32 or 64");
    const auto fn = f16 ? (cin == 32 ? launch<PF16, 32> : launch<PF16, 64>) : (cin == 32 ? launch<PBf16, 32> : launch<PBf16, 64>);
    return fn(ctx, grid, in1, c1, in2, c2, wpk, bias, out, partials, D, H, W, tilesY, tilesX, zseg, nseg, cout);
}
