// unet_bf16.hip - bf16 MFMA U-Net forward for gfx950: the throughput path.
//
// Same arithmetic as unet_f32.hip / MONAI BasicUNet.forward (inference/sliding_window_inferer.py:222,
// ctor inference/inference.py:190-197) with bf16 activations + weights, fp32 MFMA accumulation and
// fp32 InstanceNorm statistics taken from the un-rounded accumulators.
//
// Data layout in HBM ("chunk-planar", z-major slabs per 8-channel chunk):
//     act[n][C/8][D][H][W] of uint4  (one uint4 = 8 consecutive channels of one voxel, bf16)
// so that (a) consecutive x voxels of a chunk are consecutive 16-byte elements (coalesced 1 KiB
// wave loads/stores), and (b) an MFMA B-operand fragment (8 input channels of one voxel per lane)
// is exactly one ds_read_b128 / global_load_dwordx4.
//
// 3x3x3 convolutions are implicit GEMMs on v_mfma_f32_32x32x16_bf16 with
//     A = weights  (rows = 32 output channels, k = 16 input channels of one tap)
//     B = input    (cols = 32 voxels,          k = same 16 channels, shifted by the tap)
//     D[row = cout][col = voxel]  ->  each lane ends up with 4 consecutive output channels of its
//                                     voxel per register quad = one 8-byte bf16 store.
// K runs over 27 taps x Cin/16.  Weights are pre-packed in A-fragment order (one coalesced 1 KiB
// load per fragment, L2-resident); the input halo tile is staged through LDS.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "prec16.h"

namespace {

#define AS_FRAG(x) (x)

__device__ __forceinline__ float mish_fast(float y) {
    // y * tanh(softplus(y)) = y * t / (t + 2) = y - 2y / d,  d = t + 2 = n (n + 2) + 2,  n = e^y.
    // In this form nothing has to be clamped: for large y, n and d overflow to +inf, 1/d = 0 and the result is y exactly (torch's
    // softplus threshold does the same from y = 20).  For very negative y the difference y - 2y/d cancels: its absolute error is
    // |y| * 2^-23 (about 1e-6 at y = -10, where the exact value is -4.5e-4 and fp16's half ulp 2.4e-7: a relative 2e-3 of a value
    // that is itself 5e-4 of the tensor's scale - inside the 1e-3 rel. RMS the 16-bit forward is held to, not below the store's
    // rounding as an earlier comment claimed).  One v_exp_f32 + one v_rcp_f32 (1 ulp) and four plain
    // VALU ops; __fdividef would expand to the 10-instruction IEEE division sequence.
    const float n = __builtin_amdgcn_exp2f(y * 1.44269504f);
    const float d = fmaf(n, n + 2.f, 2.f);
    return fmaf(-2.f * y, __builtin_amdgcn_rcpf(d), y);
}

// two values at once: the plain operations become packed-f32 instructions (v_pk_mul/add/fma_f32, two lanes' worth of
// work per issue slot); element for element the same operations as mish_fast, i.e. the same bits
__device__ __forceinline__ f32x2_t mish_fast2(f32x2_t y) {
    const f32x2_t l2e = {1.44269504f, 1.44269504f}, two = {2.f, 2.f}, m2 = {-2.f, -2.f};
    const f32x2_t e = y * l2e;
    const f32x2_t n = {__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
    const f32x2_t d = __builtin_elementwise_fma(n, n + two, two);
    const f32x2_t r = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    return __builtin_elementwise_fma(m2 * y, r, y);
}
__device__ __forceinline__ f32x2_t fma2(f32x2_t a, f32x2_t b, f32x2_t c) { return __builtin_elementwise_fma(a, b, c); }

}  // namespace

// the kernels (each header opens the anonymous namespace again)
#include "unet16_pack.h"
#include "unet16_stem.h"
#include "unet16_conv.h"
#include "unet16_norm.h"
#include "unet16_deconv.h"
#include "unet16_final.h"
#include "unet16_convert.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
struct Dims {
    int D, H, W;
    long long vox() const { return (long long)D * H * W; }
};

template <class P>
const uint16_t* wpack(const DlvConvLayer& L) { return P::IS_F16 ? L.w_f16 : L.w_bf16; }
template <class P>
const uint16_t* wpack(const DlvDeconvLayer& L) { return P::IS_F16 ? L.w_f16 : L.w_bf16; }

// a tensor of the forward: chunk-planar data + the scale/shift it still awaits (nullptr: final values)
struct Act16 {
    uint4* p;
    int C;
    const float2* ss;
};

template <class P>
struct Net16 {
    dlv_ctx* ctx;
    int B;
    float* partials;
    size_t partials_floats;
    float2* ss_base;  // [DLV_N_CONV][B][256]: scale/shift of every conv layer of this forward (skip tensors stay raw)
    float2* ss_of(int li) const { return ss_base + (size_t)li * B * 256; }
    static size_t ss_bytes(int B) { return (size_t)DLV_N_CONV * B * 256 * sizeof(float2); }

    using Act = Act16;

    int grid1d(long long n) const { return (int)std::min<long long>((n + 255) / 256, 256LL * 16); }

    // InstanceNorm + Mish in place (the tensor becomes final); PW: the format the activated tensor is written in (P, except
    // where the mixed mode hands a bf16 level-1 tensor to the fp16 level 0)
    template <class PW = P>
    int materialise(Act& t, Dims d) {
        if (!t.ss) return DLV_OK;
        DLV_TRY((norm_mish<PW, P>(t.p, t.C, d, nullptr, t.ss, true)));
        t.ss = nullptr;
        return DLV_OK;
    }

    int stats(int nparts, int li, Dims d) {
        const DlvConvLayer& L = ctx->conv[li];
        // the fp16 format stores the raw stem output scaled by 2^-8: eps scales with its square (same normalised value)
        // ... and a layer stored 2^-shift times smaller (dlv_unet_set_conv_shift) with 4^-shift
        const float eps = (li == 0 ? 1e-5f * P::STEM_SCALE * P::STEM_SCALE : 1e-5f) * exp2f(-2.f * (float)L.shift);
        hipLaunchKernelGGL(stats_finalize_kernel, dim3(B * L.cout), dim3(64), 0, ctx->stream, partials, nparts, L.cout,
                           1.0 / (double)d.vox(), eps, L.gamma, L.beta, ss_of(li), ctx->range_flag, li);
        DLV_LAUNCH_CHECK(ctx, "stats_finalize_kernel");
        return DLV_OK;
    }

    // The plans (layer_plan.h) say which kernel runs a layer and what has to happen to its inputs first; the methods below
    // execute them.  plan_of: conv block li on [a1, a2]; a1 may still await its activation (a1.ss)
    DlvConvPlan plan_of(int li, const Act& a1, int c2, Dims d) const {
        const DlvConvLayer& L = ctx->conv[li];
        return plan_conv(ctx->sw, li, L.cin, L.cout, a1.C, c2, a1.ss != nullptr, B, d.D, d.H, d.W);
    }
    // is conv `li` (the first conv of an UpCat block) run as skip-half conv + folded up half?
    bool plan_fold(int li, int cskip, Dims d) const {
        return plan_folds_up(ctx->sw, ctx->conv[li].up_corr != nullptr, cskip, ctx->conv[li].cout, d.D, d.H, d.W);
    }

    // raw conv output + its InstanceNorm scale/shift into ss_of(li).  An input that still awaits its activation is either
    // activated by the kernel while it stages it (conv_zreg.hip) or made final by a normalisation pass first.
    int conv(int li, Act& a1, Act* a2, uint4* out, Dims d) {
        const DlvConvLayer& L = ctx->conv[li];
        const int c1 = a1.C, c2 = a2 ? a2->C : 0;
        if (c1 + c2 != L.cin) return dlv_fail(ctx, DLV_ESTATE, "conv %d: %d+%d input channels, expected %d", li, c1, c2, L.cin);
        if (c1 % 32 || c2 % 32) return dlv_fail(ctx, DLV_EUNSUP, "conv %d: concat parts must be multiples of 32 channels", li);
        const DlvConvPlan plan = plan_of(li, a1, c2, d);
        if (a2) DLV_TRY(materialise(*a2, d));
        if (plan.norm_first) DLV_TRY(materialise(a1, d));
        return run_conv(plan, li, a1, a2 ? a2->p : nullptr, c2, nullptr, out, d);
    }
    // upcat_1.conv_0 folded with its transposed conv (upconv.hip): P from the ACTIVATED coarse tensor, then the 32-channel conv
    // of the skip half with P as its addend
    int conv_folded(int li, Act& sk, Act& coarse, uint4* pbuf, uint4* out, Dims d, Dims dc) {
        const DlvConvLayer& L = ctx->conv[li];
        const DlvConvPlan plan = plan_conv_folded(ctx->sw, li, L.cout, sk.ss != nullptr, d.D, d.H, d.W);
        DLV_TRY(materialise(coarse, dc));
        if (plan.norm_first) DLV_TRY(materialise(sk, d));
        if (coarse.C != 32) return dlv_fail(ctx, DLV_ESTATE, "folded conv %d: %d coarse channels, expected 32", li, coarse.C);
        const DlvLabel lb = dlv_label_upconv(dlv_upconv2_persistent(ctx, dc.D, dc.H, dc.W), P::IS_F16, B, d.D, d.H, d.W);
        DlvProf pr(ctx, lb.name, lb.flops, lb.bytes);
        DLV_TRY(dlv_upconv2_launch(ctx, P::IS_F16, coarse.p, P::IS_F16 ? L.wup_f16 : L.wup_bf16, L.up_corr, pbuf, B, dc.D, dc.H, dc.W, coarse.C / 8, 0));
        pr.end();
        return run_conv(plan, li, sk, nullptr, 0, pbuf, out, d);
    }

    template <int NCB, int TX, bool WLDS>
    int launch_generic(const DlvConvLayer& L, const uint4* in1, int c1, const uint4* in2, int c2, uint4* out, Dims d) {
        const int tY = dlv_cdiv(d.H, 64 / TX), tX = dlv_cdiv(d.W, TX);
        const size_t lds = std::max<size_t>((size_t)ConvTile<TX>::SLAB * 16 + (WLDS ? (size_t)NCB * 27 * 2 * 64 * 16 : 0), (size_t)4 * NCB * 32 * 2 * 4);
        static dlv_attr_bits attr_done{0};  // bit per device
        if (!dlv_attr_is_set(attr_done, ctx->device)) {
            DLV_HIP(ctx, hipFuncSetAttribute((const void*)conv3_mfma_kernel<P, NCB, TX, WLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            dlv_attr_mark(attr_done, ctx->device);
        }
        ctx->ran.conv = DLV_PLAN_GENERIC;
        ctx->ran.tx = TX;
        ctx->ran.ncb = NCB;
        ctx->ran.wlds = WLDS;
        hipLaunchKernelGGL((conv3_mfma_kernel<P, NCB, TX, WLDS>), dim3(dlv_cdiv(d.D, 4) * tY * tX, L.cout / (32 * NCB), B), dim3(256), lds, ctx->stream, in1,
                           c1 / 8, in2, c2 / 8, reinterpret_cast<const uint4*>(wpack<P>(L)), L.bias16, out, partials, L.cout, d.D, d.H, d.W, tY, tX);
        DLV_LAUNCH_CHECK(ctx, "conv3_mfma_kernel");
        return DLV_OK;
    }
    template <int TX, bool WLDS>
    int launch_generic_ncb(int ncb, const DlvConvLayer& L, const uint4* in1, int c1, const uint4* in2, int c2, uint4* out, Dims d) {
        if (ncb == 1) return launch_generic<1, TX, WLDS>(L, in1, c1, in2, c2, out, d);
        if (ncb == 2 || WLDS) return launch_generic<2, TX, WLDS>(L, in1, c1, in2, c2, out, d);
        return launch_generic<WLDS ? 2 : 4, TX, WLDS>(L, in1, c1, in2, c2, out, d);
    }

    // one planned conv: bound check, kernel timer, launch, statistics.  a1: first input (a1.ss: activated on load); addend: P
    int run_conv(const DlvConvPlan& plan, int li, const Act& a1, const uint4* in2, int c2, const uint4* addend, uint4* out, Dims d) {
        const DlvConvLayer& L = ctx->conv[li];
        static const char* const family[4] = {" (zreg)", " (deep)", " (zmarch)", ""};
        if ((size_t)B * plan.max_parts * L.cout * 2 > partials_floats) return dlv_fail(ctx, DLV_ESTATE, "partials buffer too small%s", family[plan.kernel]);
        const DlvLabel lb = dlv_label_conv(plan, P::IS_F16, B, d.D, d.H, d.W);
        DlvProf pr(ctx, lb.name, lb.flops, lb.bytes);
        const uint4* in1 = a1.p;
        const uint16_t* w16 = plan.folded ? (P::IS_F16 ? L.wskip_f16 : L.wskip_bf16) : (P::IS_F16 ? L.w16_f16 : L.w16_bf16);
        int np = (int)plan.max_parts;
        switch (plan.kernel) {
            case DLV_PLAN_ZREG:
                DLV_TRY(dlv_conv3_zreg_launch(ctx, P::IS_F16, plan.cin, L.cout, in1, a1.C, a1.ss, in2, c2, nullptr, w16, out, partials, B, d.D, d.H, d.W,
                                              &np, addend));
                break;
            case DLV_PLAN_DEEP:
                DLV_TRY(dlv_conv3_deep_launch(ctx, P::IS_F16, L.cin, L.cout, in1, a1.C, in2, c2, w16, out, partials, B, d.D, d.H, d.W, &np));
                break;
            case DLV_PLAN_ZMARCH:
                DLV_TRY(dlv_conv3_zmarch_launch(ctx, P::IS_F16, L.cin, L.cout, in1, a1.C, in2, c2, wpack<P>(L), L.bias16, out, partials, B, d.D, d.H, d.W, &np));
                break;
            default:  // DLV_PLAN_GENERIC: one partial row per tile
                if (plan.wlds) DLV_TRY(plan.tx == 16 ? (launch_generic_ncb<16, true>(plan.ncb, L, in1, a1.C, in2, c2, out, d))
                                                     : (launch_generic_ncb<8, true>(plan.ncb, L, in1, a1.C, in2, c2, out, d)));
                else DLV_TRY(plan.tx == 16 ? (launch_generic_ncb<16, false>(plan.ncb, L, in1, a1.C, in2, c2, out, d))
                                           : (launch_generic_ncb<8, false>(plan.ncb, L, in1, a1.C, in2, c2, out, d)));
                break;
        }
        pr.end();
        if (np > plan.max_parts) return dlv_fail(ctx, DLV_ESTATE, "partials buffer too small%s", family[plan.kernel]);  // (what the launcher wrote)
        return stats(np, li, d);
    }

    // InstanceNorm apply + Mish (+ MaxPool into `pooled`); writeback = false (pool only): x stays raw for consumers that
    // activate while loading
    // PW / PQ: formats of the written-back and of the pooled tensor (norm_mish_kernel)
    template <class PW = P, class PQ = P>
    int norm_mish(uint4* x, int C, Dims d, uint4* pooled, const float2* ss, bool writeback) {
        const DlvNormPlan plan = plan_norm_pass(ctx->sw, pooled != nullptr, B, C, d.D, d.H, d.W);
        const bool nt = plan.nt;
        constexpr bool seam = !std::is_same<PW, P>::value || !std::is_same<PQ, P>::value;  // (the mixed mode's format change)
        const DlvLabel lb = dlv_label_norm(pooled != nullptr, writeback, P::IS_F16, seam, B, C, d.D, d.H, d.W);
        DlvProf pr(ctx, lb.name, lb.flops, lb.bytes);
        ctx->ran.norm = DLV_DBG_NM_RAN | (plan.rows ? DLV_DBG_NM_ROWS : 0) | (pooled ? DLV_DBG_NM_POOLED : 0) | (writeback ? DLV_DBG_NM_WRITEBACK : 0) |
                        (nt ? DLV_DBG_NM_NT : 0) | (seam ? DLV_DBG_NM_SEAM : 0);
        ++ctx->ran.norm_passes;
        if (plan.rows) {
            const long long items = (long long)(d.D / 2) * (d.H / 2) * (d.W / 64);
            dim3 g2((unsigned)std::max<long long>(1, std::min<long long>((items + 3) / 4, 4096)), C / 8, B);  // (one item per wave: 4 / 8 / 16 items per workgroup 902 / 914 / 939 us)
#define DLV_NP_LAUNCH(WB_, NT_) \
    hipLaunchKernelGGL((norm_mish_pool_rows_kernel<P, WB_, NT_, PQ>), g2, dim3(256), 0, ctx->stream, x, ss, C, d.D, d.H, d.W, pooled)
            if (writeback && nt) DLV_NP_LAUNCH(true, true);
            else if (writeback) DLV_NP_LAUNCH(true, false);
            else if (nt) DLV_NP_LAUNCH(false, true);
            else DLV_NP_LAUNCH(false, false);
#undef DLV_NP_LAUNCH
        } else {
            // two grid-stride iterations per thread under the non-temporal policy (profiles/microbench/nt_probe.hip: 2.15 GB in
            // place 743 us at 2048 x default, 642 us at 4096 x nt)
            const long long work = pooled ? d.vox() / 8 : d.vox();
            dim3 grid(std::max(1, std::min(grid1d(work), nt && !pooled ? 4096 : 2048)), C / 8, B);
#define DLV_NM_LAUNCH(POOL_, WB_)                                                                                                  \
    do {                                                                                                                           \
        if (nt)                                                                                                                    \
            hipLaunchKernelGGL((norm_mish_kernel<P, POOL_, WB_, true, PW, PQ>), grid, dim3(256), 0, ctx->stream, x, ss, C, d.D, d.H, d.W, pooled); \
        else                                                                                                                       \
            hipLaunchKernelGGL((norm_mish_kernel<P, POOL_, WB_, false, PW, PQ>), grid, dim3(256), 0, ctx->stream, x, ss, C, d.D, d.H, d.W, pooled); \
    } while (0)
            if (pooled && writeback) DLV_NM_LAUNCH(true, true);
            else if (pooled) DLV_NM_LAUNCH(true, false);
            else DLV_NM_LAUNCH(false, true);
#undef DLV_NM_LAUNCH
        }
        pr.end();
        DLV_LAUNCH_CHECK(ctx, "norm_mish_kernel");
        return DLV_OK;
    }

    // the transposed conv of an UpCat block into `out` with the SKIP tensor's dimensions `dskip`: where they are 2 x the input's,
    // straight into it; where the skip tensor is odd (windows that are not multiples of 16), into `tmp` and from there
    // replicate-padded by one voxel at the far end (MONAI's UpCat)
    int deconv_to(int j, Act& a, uint4* out, uint4* tmp, Dims din, Dims dskip) {
        const Dims du{2 * din.D, 2 * din.H, 2 * din.W};
        if (du.D == dskip.D && du.H == dskip.H && du.W == dskip.W) return deconv(j, a, out, din);
        if (dskip.D - du.D > 1 || dskip.H - du.H > 1 || dskip.W - du.W > 1 || dskip.D < du.D || dskip.H < du.H || dskip.W < du.W)
            return dlv_fail(ctx, DLV_ESTATE, "deconv %d: skip tensor %dx%dx%d against an up-sampled %dx%dx%d", j, dskip.D, dskip.H, dskip.W, du.D, du.H, du.W);
        DLV_TRY(deconv(j, a, tmp, din));
        const int cout = ctx->deconv[j].cout;
        const DlvLabel lb = dlv_label_pad(P::IS_F16, cout, B, du.vox(), dskip.vox());
        DlvProf pr(ctx, lb.name, lb.flops, lb.bytes);
        ctx->ran.pad = 1;
        hipLaunchKernelGGL(replicate_pad_cp_kernel, dim3(std::max(1, std::min(grid1d(dskip.vox()), 1024)), B * (cout / 8)), dim3(256), 0, ctx->stream,
                           tmp, out, du.D, du.H, du.W, dskip.D, dskip.H, dskip.W);
        pr.end();
        DLV_LAUNCH_CHECK(ctx, "replicate_pad_cp_kernel");
        return DLV_OK;
    }

    template <int KP>
    int launch_deconv(int kernel, const DlvDeconvLayer& L, const uint4* in, const float2* ssin, uint4* out, Dims din) {
        const uint4* w = reinterpret_cast<const uint4*>(wpack<P>(L));
        const int segs = dlv_cdiv(din.W, 16);
        const long long rowsegs = (long long)din.D * din.H * segs;
        if constexpr (KP <= 4) {
            if (kernel == DLV_PLAN_DC_REGW) {
                ctx->ran.deconv = DLV_PLAN_DC_REGW;
                hipLaunchKernelGGL((deconv2_regw_kernel<P, KP>), dim3(dlv_cdiv(rowsegs, 4 * DC_IPW), B), dim3(256), 0, ctx->stream, in, w, L.bias, out, din.D,
                                   din.H, din.W, segs, ssin);
                return DLV_OK;
            }
        } else {
            if (kernel == DLV_PLAN_DC_WST) {
                ctx->ran.deconv = DLV_PLAN_DC_WST;
                hipLaunchKernelGGL((deconv2_wst_kernel<P, KP>), dim3(dlv_cdiv(rowsegs, 4 * DW_IPW), 4 * (L.cout / 32), B), dim3(256), 0, ctx->stream, in, w,
                                   L.bias, out, L.cout, din.D, din.H, din.W, segs, ssin);
                return DLV_OK;
            }
        }
        if (kernel == DLV_PLAN_DC_ROWS) {
            ctx->ran.deconv = DLV_PLAN_DC_ROWS;
            hipLaunchKernelGGL((deconv2_rows_kernel<P, KP>), dim3(dlv_cdiv(rowsegs, 4), B), dim3(256), 0, ctx->stream, in, w, L.bias, out, L.cout, din.D, din.H,
                               din.W, segs, ssin);
        } else {  // DLV_PLAN_DC_PARITY (no activation on load: the plan made the input final)
            ctx->ran.deconv = DLV_PLAN_DC_PARITY;
            hipLaunchKernelGGL((deconv2_mfma_kernel<P, KP>), dim3(dlv_cdiv(din.vox(), 128), B), dim3(256), 0, ctx->stream, in, w, L.bias, out, L.cout, din.D,
                               din.H, din.W);
        }
        return DLV_OK;
    }

    int deconv(int j, Act& a, uint4* out, Dims din) {
        const DlvDeconvLayer& L = ctx->deconv[j];
        const DlvDeconvPlan plan = plan_deconv(ctx->sw, L.cin, L.cout, a.ss != nullptr, din.D, din.H, din.W);
        if (plan.kernel == DLV_PLAN_NONE) return dlv_fail(ctx, DLV_EUNSUP, "deconv %d: Cin=%d not in {32,64,128,256}", j, L.cin);
        if (plan.norm_first) DLV_TRY(materialise(a, din));
        const DlvLabel lb = dlv_label_deconv(plan, P::IS_F16, L.cin, L.cout, B, din.D, din.H, din.W);
        DlvProf pr(ctx, lb.name, lb.flops, lb.bytes);
        if (plan.kernel == DLV_PLAN_DC_DEEP) {  // `in` holds final values
            DLV_TRY(dlv_deconv2_deep_launch(ctx, P::IS_F16, L.cin, L.cout, a.p, P::IS_F16 ? L.w16_f16 : L.w16_bf16, L.bias, out, B, din.D, din.H, din.W));
            pr.end();
            return DLV_OK;
        }
        switch (L.cin / 16) {
            case 2: DLV_TRY(launch_deconv<2>(plan.kernel, L, a.p, a.ss, out, din)); break;
            case 4: DLV_TRY(launch_deconv<4>(plan.kernel, L, a.p, a.ss, out, din)); break;
            case 8: DLV_TRY(launch_deconv<8>(plan.kernel, L, a.p, a.ss, out, din)); break;
            default: DLV_TRY(launch_deconv<16>(plan.kernel, L, a.p, a.ss, out, din)); break;
        }
        pr.end();
        DLV_LAUNCH_CHECK(ctx, "deconv2 kernel");
        return DLV_OK;
    }

    // the final 1x1x1 conv on the raw output of the last block (activated on load): plain logits, or (acc) blended into the
    // accumulator at the windows' places
    int final_conv(const Act& cur, Dims d, float* logits, float* acc, const int* starts_dev, int flip_dim, int Yp, int Xp, float scale) {
        if (!cur.ss || cur.C != 32) return dlv_fail(ctx, DLV_ESTATE, "final conv: a raw 32-channel tensor with its scale/shift expected");
        dim3 grid(std::min(grid1d(d.vox()), 512), B);  // (16 iterations per thread at 128^3 - the software pipeline wants a long loop: 1024 / 512 / 256 workgroups 515 / 487 / 484 us)
        const DlvLabel lb = dlv_label_final(acc != nullptr, B, d.D, d.H, d.W);
        DlvProf pr(ctx, lb.name, lb.flops, lb.bytes);
        if (acc)
            hipLaunchKernelGGL((final_conv_kernel<P, true>), grid, dim3(256), 0, ctx->stream, cur.p, cur.ss, ctx->final_w,
                               ctx->final_b, nullptr, starts_dev, flip_dim, Yp, Xp, scale, acc, d.D, d.H, d.W, ctx->blend_w, ctx->blend_min,
                               ctx->blend_wsum, ctx->range_flag);
        else
            hipLaunchKernelGGL((final_conv_kernel<P, false>), grid, dim3(256), 0, ctx->stream, cur.p, cur.ss, ctx->final_w,
                               ctx->final_b, logits, nullptr, -1, 0, 0, 1.f, nullptr, d.D, d.H, d.W, nullptr, 0.f, nullptr, ctx->range_flag);
        pr.end();
        DLV_LAUNCH_CHECK(ctx, "final_conv_kernel");
        return DLV_OK;
    }
};

// the whole forward; the stem reads either xf (fp32 patches) or the uint16 volume windows, the final
// layer writes either logits or blends into acc
// workspace of one 16-bit forward of B windows (one pipeline lane): the activations (4 buffers per level), the InstanceNorm partial
// sums + scale/shift tables.  Shared by forward_16 and dlv_unet_reserve_16 (the same arithmetic, or the reservation is useless).
struct Ws16 {
    size_t act, stats, pfloats;
};
static Ws16 ws16_bytes(const int* f, int B, int d, int h, int w, size_t (*offs)[4]) {
    const int lvlC[5] = {32, f[1], f[2], f[3], f[4]};
    size_t off = 0;
    for (int l = 0; l < 5; ++l)
        for (int k = 0; k < 4; ++k) {
            if (offs) offs[l][k] = off;
            off += (size_t)B * lvlC[l] * ((size_t)(d >> l) * (h >> l) * (w >> l)) * 2;
            off = (off + 255) & ~(size_t)255;
        }
    // partial sums: the level-0 convs have the most tiles (256 voxels each); the stem has fewer blocks
    const long long max_tiles = (long long)dlv_cdiv(d, 4) * dlv_cdiv(h, 4) * dlv_cdiv(w, 8) + 64;
    const size_t pfloats = (size_t)B * max_tiles * 64 * 2;
    return Ws16{off, pfloats * 4 + (size_t)DLV_N_CONV * B * 256 * sizeof(float2) + 256, pfloats};
}

// P0: the format of level 0 (full resolution: stem, conv_0, upcat_1, final conv), PD: of levels 1-4.  P0 = PD: one format
// throughout (fp16 / bf16 everywhere); P0 = fp16 with PD = bf16 is the mixed mode DLV_PREC_BF16 stands for (DESIGN section 5:
// the 8 bits of bf16 are lost at full resolution - fp16 there lifts the margin-free mask IoU from 0.998 to 0.9994).  The
// format changes in two normalisation passes: the pooling pass 0 -> 1 (raw fp16 in, pooled bf16 out) and the pass that
// activates the level-1 decoder output for upcat_1 (raw bf16 in, activated fp16 out).
template <class P0, class PD = P0>
int forward_16(dlv_ctx* ctx, const float* xf, const uint16_t* vol, int Yp, int Xp, const int* starts_dev, int flip_dim,
                 float scale, float* logits, float* acc, int B, int d, int h, int w) {
    const int* f = ctx->features;
    if (f[0] != 32 || f[5] != 32)
        return dlv_fail(ctx, DLV_EUNSUP, "bf16 path: features[0] and features[5] must be 32 (got %d, %d)", f[0], f[5]);
    // the stem, the final conv and the norm passes index a window's voxels with 32 bits (whatever conv kernel runs in between)
    if ((long long)d * h * w >= (1ll << 31)) return dlv_fail(ctx, DLV_EUNSUP, "16-bit path: a window of %d x %d x %d voxels exceeds the 2^31 voxel index range", d, h, w);
    Dims dm[5];
    for (int l = 0; l < 5; ++l) dm[l] = Dims{d >> l, h >> l, w >> l};
    size_t offs[5][4];
    Ws16 wsz = ws16_bytes(f, B, d, h, w, offs);
    const size_t off = wsz.act, pfloats = wsz.pfloats;
    char* base;
    DLV_TRY(dlv_ws_get(ctx, ctx->lane ? WS_LANE_ACT0 + (ctx->lane - 1) : WS_BF16_ACT, off, (void**)&base));
    char* sbase;
    DLV_TRY(dlv_ws_get(ctx, ctx->lane ? WS_LANE_STATS0 + (ctx->lane - 1) : WS_STATS, wsz.stats, (void**)&sbase));
    Net16<P0> net{ctx, B, (float*)sbase, pfloats, (float2*)(sbase + ((pfloats * 4 + 255) & ~(size_t)255))};  // level 0
    Net16<PD> netd{ctx, B, net.partials, pfloats, net.ss_base};                                                // levels 1-4
    constexpr bool mixed = !std::is_same<P0, PD>::value;
    using P = P0;
    using Act = Act16;
    auto buf = [&](int l, int k) { return (uint4*)(base + offs[l][k]); };
    enum { A = 0, Bf = 1, S = 2, U = 3 };

    // stem
    Act x0{buf(0, A), 32, nullptr};
    {
        dim3 grid(dlv_cdiv((long long)h * w, 256), dlv_cdiv(d, STEM_ZR), B);
        int nblk = grid.x * grid.y;
        bool two_pass_stem = false;
        if ((size_t)B * nblk * 64 > pfloats) return dlv_fail(ctx, DLV_ESTATE, "partials buffer too small (stem)");
        const DlvConvLayer& L = ctx->conv[0];
        const bool stem_mfma = plan_stem_mfma(ctx->sw, vol != nullptr);
        const DlvLabel lb = dlv_label_stem(stem_mfma, B, d, h, w);
        DlvProf pr(ctx, lb.name, lb.flops, lb.bytes);
        if (stem_mfma) {
            const int tY = dlv_cdiv(h, SM_TY), tX = dlv_cdiv(w, SM_TX), tZ = dlv_cdiv(d, SM_TZ * SM_ZC);
            grid = dim3(tZ * tY * tX, 1, B);
            nblk = grid.x;
            if ((size_t)B * nblk * 64 > pfloats) return dlv_fail(ctx, DLV_ESTATE, "partials buffer too small (stem)");
            const uint4* wst = reinterpret_cast<const uint4*>(wpack<P>(L));
            hipLaunchKernelGGL((stem_mfma_kernel<P, 1>), grid, dim3(256), 0, ctx->stream, vol, Yp, Xp, starts_dev, flip_dim, wst,
                               L.bias16, buf(0, A), net.partials, (const float2*)nullptr, d, h, w, tY, tX);
            DLV_LAUNCH_CHECK(ctx, "stem_mfma_kernel<1>");
            DLV_TRY(net.stats(nblk, 0, dm[0]));
            hipLaunchKernelGGL((stem_mfma_kernel<P, 2>), grid, dim3(256), 0, ctx->stream, vol, Yp, Xp, starts_dev, flip_dim, wst,
                               L.bias16, buf(0, A), net.partials, (const float2*)net.ss_of(0), d, h, w, tY, tX);
            two_pass_stem = true;
        } else if (vol)
            hipLaunchKernelGGL((stem_conv_kernel<P, true>), grid, dim3(256), 0, ctx->stream, nullptr, vol, Yp, Xp, starts_dev,
                               flip_dim, L.w_f32, L.bias, buf(0, A), net.partials, d, h, w, P::STEM_SCALE * exp2f(-(float)L.shift));
        else
            hipLaunchKernelGGL((stem_conv_kernel<P, false>), grid, dim3(256), 0, ctx->stream, xf, nullptr, 0, 0, nullptr, -1,
                               L.w_f32, L.bias, buf(0, A), net.partials, d, h, w, P::STEM_SCALE * exp2f(-(float)L.shift));
        pr.end();
        DLV_LAUNCH_CHECK(ctx, "stem_conv_kernel");
        if (!two_pass_stem) {
            DLV_TRY(net.stats(nblk, 0, dm[0]));
            x0.ss = net.ss_of(0);  // raw: the first conv activates it while staging, or it is made final first
        }
    }
    const int encC[5] = {32, f[1], f[2], f[3], f[4]};
    // encoder.  skip[l] = output of level l (consumed pooled by level l+1 and, as the skip connection, by upcat_{l+1}).
    // Where both consumers of a raw tensor activate on load, no normalised copy of it is ever written: only the pooled
    // tensor is produced (levels 0 and 1 of the default windows); elsewhere the normalisation pass writes it back.
    Act skip[5];
    {
        Act s0{buf(0, S), 32, nullptr};
        DLV_TRY(net.conv(1, x0, nullptr, s0.p, dm[0]));
        s0.ss = net.ss_of(1);
        skip[0] = s0;
    }
    for (int l = 1; l <= 4; ++l) {
        // pool level l-1 into the input of level l
        Act& up = skip[l - 1];
        const int li_cat = 18 - 2 * l;  // upcat conv that takes skip[l-1]: 16, 14, 12, 10
        const int c_up = ctx->deconv[4 - l].cout;
        // does the UpCat conv that takes this skip tensor activate it on load?  (what its plan will say of the raw tensor)
        const DlvConvLayer& Lcat = ctx->conv[li_cat];
        const bool keep_raw = plan_conv(ctx->sw, li_cat, Lcat.cin, Lcat.cout, up.C, c_up, true, B, dm[l - 1].D, dm[l - 1].H, dm[l - 1].W).act_on_load;
        const bool odd = ((dm[l - 1].D | dm[l - 1].H | dm[l - 1].W) & 1) != 0;
        // a level with an odd size (windows that are not multiples of 16): MaxPool3d(2) drops its last plane / row / column, so the
        // pooling pass - which writes back only what it pools - cannot be the pass that makes the tensor final: pool only, then a
        // full normalisation pass (unless every consumer activates on load)
        if (l == 1) {  // (level 0 stays P0, pooled: PD)
            DLV_TRY((net.template norm_mish<P0, PD>(up.p, up.C, dm[0], buf(1, A), up.ss, !keep_raw && !odd)));
            if (odd && !keep_raw) DLV_TRY(net.norm_mish(up.p, up.C, dm[0], nullptr, up.ss, true));
        } else {
            DLV_TRY(netd.norm_mish(up.p, up.C, dm[l - 1], buf(l, A), up.ss, !keep_raw && !odd));
            if (odd && !keep_raw) DLV_TRY(netd.norm_mish(up.p, up.C, dm[l - 1], nullptr, up.ss, true));
        }
        if (!keep_raw) up.ss = nullptr;
        Act a{buf(l, A), encC[l - 1], nullptr};
        Act b{buf(l, Bf), encC[l], nullptr};
        DLV_TRY(netd.conv(2 * l, a, nullptr, b.p, dm[l]));
        b.ss = net.ss_of(2 * l);
        Act s{buf(l, S), encC[l], nullptr};
        DLV_TRY(netd.conv(2 * l + 1, b, nullptr, s.p, dm[l]));
        s.ss = net.ss_of(2 * l + 1);
        skip[l] = s;
    }
    // decoder: transposed conv (activates its input on load), concat [skip, up], two convs
    Act cur = skip[4];
    for (int j = 0; j < 4; ++j) {
        const int l = 3 - j;
        const int li = 10 + 2 * j;
        Act b{buf(l, Bf), ctx->conv[li].cout, nullptr};
        if (l >= 1) {
            DLV_TRY(netd.deconv_to(j, cur, buf(l, U), buf(l, A), dm[l + 1], dm[l]));  // (buf(l, A): free until this block's second conv writes it)
            Act u{buf(l, U), ctx->deconv[j].cout, nullptr};
            DLV_TRY(netd.conv(li, skip[l], &u, b.p, dm[l]));
            b.ss = net.ss_of(li);
            Act o{buf(l, A), ctx->conv[li + 1].cout, nullptr};
            DLV_TRY(netd.conv(li + 1, b, nullptr, o.p, dm[l]));
            o.ss = net.ss_of(li + 1);
            cur = o;
            continue;
        }
        // level 0.  Mixed mode: the level-1 output is activated here and WRITTEN in the level-0 format (one pass either way: the
        // folded conv below needs the activated tensor, and the plain transposed conv then finds nothing left to activate)
        if (mixed) DLV_TRY((netd.template materialise<P0>(cur, dm[1])));
        if (net.plan_fold(li, skip[l].C, dm[l])) {
            // upcat_1: the transposed conv folded into the conv (upconv.hip): P from the activated coarse tensor, then the
            // 32-channel conv of the skip half with P as its addend - no up-sampled tensor, 8 coarse taps instead of 27 fine ones
            DLV_TRY(net.conv_folded(li, skip[l], cur, buf(l, U), b.p, dm[l], dm[l + 1]));
        } else {
            DLV_TRY(net.deconv_to(j, cur, buf(l, U), buf(l, A), dm[l + 1], dm[l]));  // (buf(0, A): the stem's output, consumed)
            Act u{buf(l, U), ctx->deconv[j].cout, nullptr};
            DLV_TRY(net.conv(li, skip[l], &u, b.p, dm[l]));
        }
        b.ss = net.ss_of(li);
        Act o{buf(l, A), ctx->conv[li + 1].cout, nullptr};
        DLV_TRY(net.conv(li + 1, b, nullptr, o.p, dm[l]));
        o.ss = net.ss_of(li + 1);
        cur = o;
    }
    DLV_TRY(net.final_conv(cur, dm[0], logits, acc, starts_dev, flip_dim, Yp, Xp, scale));
    return DLV_OK;
}

template <class P>
int pack_weights_16(dlv_ctx* ctx) {
    auto dst = [](auto& L) { return const_cast<uint16_t*>(wpack<P>(L)); };
    hipLaunchKernelGGL(pack_stem_w_kernel<P>, dim3(8), dim3(256), 0, ctx->stream, ctx->conv[0].w_f32, dst(ctx->conv[0]), exp2f(-(float)ctx->conv[0].shift));
    DLV_LAUNCH_CHECK(ctx, "pack_stem_w_kernel");
    for (int i = 0; i < DLV_N_CONV; ++i) {  // the bias the 16-bit kernels add: scaled like the weights
        const DlvConvLayer& L = ctx->conv[i];
        hipLaunchKernelGGL(scale_copy_kernel, dim3(dlv_cdiv(L.cout, 256)), dim3(256), 0, ctx->stream, L.bias, L.bias16, L.cout, exp2f(-(float)L.shift));
        DLV_LAUNCH_CHECK(ctx, "scale_copy_kernel");
    }
    for (int i = 1; i < DLV_N_CONV; ++i) {
        const DlvConvLayer& L = ctx->conv[i];
        if (L.cin % 32 || L.cout % 32) return dlv_fail(ctx, DLV_EUNSUP, "conv %d: %d->%d not multiples of 32", i, L.cin, L.cout);
        const float ws = exp2f(-(float)L.shift);
        hipLaunchKernelGGL(pack_conv_w_kernel<P>, dim3(256), dim3(256), 0, ctx->stream, L.w_f32, dst(ctx->conv[i]), L.cout, L.cin, ws);
        DLV_LAUNCH_CHECK(ctx, "pack_conv_w_kernel");
        DLV_TRY(dlv_pack_conv_w16(ctx, P::IS_F16, L.w_f32, P::IS_F16 ? L.w16_f16 : L.w16_bf16, L.cout, L.cin, 0, 0, ws));
        if (L.up_corr) {  // upcat_1.conv_0: skip half as a 32-channel pack, up half folded with the transposed conv (upconv.hip)
            const DlvDeconvLayer& Dl = ctx->deconv[3];
            DLV_TRY(dlv_pack_conv_w16(ctx, P::IS_F16, L.w_f32, P::IS_F16 ? L.wskip_f16 : L.wskip_bf16, L.cout, 32, L.cin, 0, ws));
            DLV_TRY(dlv_pack_upconv(ctx, P::IS_F16, L.w_f32, L.cin, 32, Dl.w_f32, Dl.bias, P::IS_F16 ? L.wup_f16 : L.wup_bf16, L.up_corr, 0, 1, ws));
        }
    }
    for (int j = 0; j < DLV_N_DECONV; ++j) {
        const DlvDeconvLayer& L = ctx->deconv[j];
        if (L.cin % 32 || L.cout % 32) return dlv_fail(ctx, DLV_EUNSUP, "deconv %d: %d->%d not multiples of 32", j, L.cin, L.cout);
        hipLaunchKernelGGL(pack_deconv_w_kernel<P>, dim3(64), dim3(256), 0, ctx->stream, L.w_f32, dst(ctx->deconv[j]), L.cin, L.cout);
        DLV_LAUNCH_CHECK(ctx, "pack_deconv_w_kernel");
        if (L.w16_f16) DLV_TRY(dlv_pack_deconv_w16(ctx, P::IS_F16, L.w_f32, P::IS_F16 ? L.w16_f16 : L.w16_bf16, L.cin, L.cout));
    }
    return DLV_OK;
}

template <class P>
int debug_layer_16(dlv_ctx* ctx, dlv_debug_layer_args& a) {
    const int B = a.B, D = a.D, H = a.H, W = a.W;
    const Dims d{D, H, W};
    const long long vox = d.vox();
    a.ran_zreg = a.ran_upconv = a.ran_stem = a.drops_bias = a.drops_fold_const = 0;
    a.raw_scale = 1.f;
    ctx->ran_zreg = ctx->ran_upconv = 0;
    ctx->ran = dlv_ctx::Ran{};
    // what the launchers recorded (the launches are queued by then: host state)
    const auto report = [&] {
        const dlv_ctx::Ran& r = ctx->ran;
        a.ran_zreg = ctx->ran_zreg;
        a.ran_upconv = ctx->ran_upconv;
        a.ran_conv = r.conv;
        a.ran_tx = r.tx;
        a.ran_ncb = r.ncb;
        a.ran_wlds = r.wlds;
        a.ran_grid = r.grid;
        a.ran_items = r.items;
        a.ran_deconv = r.deconv;
        a.ran_gpw = r.gpw;
        a.ran_pad = r.pad;
        a.ran_norm = r.norm;
        a.ran_norm_passes = r.norm_passes;
    };
    report();
    if (B < 1 || D < 1 || H < 1 || W < 1) return dlv_fail(ctx, DLV_EINVAL, "debug layer: empty shape");
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const int kind = a.kind;
    if (a.op == DLV_DBG_NORM || a.op == DLV_DBG_FINAL) {
        const int C = a.c1;
        const bool fin = a.op == DLV_DBG_FINAL, seam = a.fmt_out != 0;
        if (!a.in1 || !a.ss1 || C < 8 || C % 8 || (fin && C != 32)) return dlv_fail(ctx, DLV_EINVAL, "norm / final op: raw in1 (C a multiple of 8; final: 32) with ss1");
        if (fin && (a.out2 || seam)) return dlv_fail(ctx, DLV_EINVAL, "final op: no second output, no format seam");
        // the two seams of the mixed mode: fp16 raw -> bf16 pooled (the pooling pass 0 -> 1), bf16 raw -> fp16 activated (upcat_1's input)
        if (seam && (P::IS_F16 ? !a.out2 : a.out2 != nullptr)) return dlv_fail(ctx, DLV_EINVAL, "norm op: the seam is fp16 -> pooled bf16 or bf16 -> activated fp16");
        if (a.out2 && (D < 2 || H < 2 || W < 2)) return dlv_fail(ctx, DLV_EINVAL, "norm op: nothing to pool");
        const long long pv = (long long)(D / 2) * (H / 2) * (W / 2);
        const size_t bx = (size_t)B * C * vox * 2, bq = a.out2 ? (size_t)B * C * pv * 2 : 0;
        char* base;
        DLV_TRY(dlv_ws_get(ctx, WS_BF16_ACT, al(bx) + al(bq) + 1024, (void**)&base));
        uint4 *x = (uint4*)base, *q = a.out2 ? (uint4*)(base + al(bx)) : nullptr;
        Net16<P> net{ctx, B, nullptr, 0, nullptr};
        const float2* ss = reinterpret_cast<const float2*>(a.ss1);
        hipLaunchKernelGGL(f32_to_cp_kernel<P>, dim3(net.grid1d(vox), C / 8, B), dim3(256), 0, ctx->stream, a.in1, x, C, vox);
        DLV_LAUNCH_CHECK(ctx, "debug layer: f32_to_cp_kernel");
        if (fin) {
            typename Net16<P>::Act cur{x, C, ss};
            if (!a.acc) {
                DLV_TRY(net.final_conv(cur, d, a.out, nullptr, nullptr, -1, 0, 0, 1.f));
                report();
                return DLV_OK;
            }
            // the blend instantiation, as a pass launches it: B windows at `starts` of an accumulator of Yp x Xp planes
            const float scale = a.scale != 0.f ? a.scale : 1.f;
            if (!a.starts) return dlv_fail(ctx, DLV_EINVAL, "final op (blend): the windows' starts expected");
            if (!(a.flip_dim == -1 || (a.flip_dim >= 2 && a.flip_dim <= 4))) return dlv_fail(ctx, DLV_EINVAL, "final op (blend): flip_dim must be -1, 2, 3 or 4");
            if (!(fabsf(scale) <= 3.0e38f) || !(a.bmin >= 0.f && a.bmin <= 3.0e38f)) return dlv_fail(ctx, DLV_EINVAL, "final op (blend): scale and bmin must be finite, bmin >= 0");
            if (a.wsum && !a.bw) return dlv_fail(ctx, DLV_EINVAL, "final op (blend): wsum collects the factors bw");
            for (int n = 0; n < B; ++n) {
                const int z0 = a.starts[3 * n], y0 = a.starts[3 * n + 1], x0 = a.starts[3 * n + 2];
                if (z0 < 0 || y0 < 0 || x0 < 0 || (long long)y0 + H > a.Yp || (long long)x0 + W > a.Xp)
                    return dlv_fail(ctx, DLV_EINVAL, "final op (blend): window %d at (%d, %d, %d) leaves the %d x %d planes", n, z0, y0, x0, a.Yp, a.Xp);
            }
            int* starts_dev;
            DLV_TRY(dlv_ws_get(ctx, WS_TILE_META, (size_t)B * 3 * sizeof(int), (void**)&starts_dev));
            DLV_HIP(ctx, hipMemcpyAsync(starts_dev, a.starts, (size_t)B * 3 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's array)
            const float* keep_w = ctx->blend_w;
            const float keep_min = ctx->blend_min;
            float* keep_wsum = ctx->blend_wsum;
            ctx->blend_w = a.bw;
            ctx->blend_min = a.bmin;
            ctx->blend_wsum = a.wsum;
            const int rc = net.final_conv(cur, d, nullptr, a.acc, starts_dev, a.flip_dim, a.Yp, a.Xp, scale);
            ctx->blend_w = keep_w;
            ctx->blend_min = keep_min;
            ctx->blend_wsum = keep_wsum;
            DLV_TRY(rc);
            report();
            return DLV_OK;
        }
        const bool wb = q ? a.writeback != 0 : true;
        bool out_f16 = P::IS_F16, q_f16 = P::IS_F16;
        if (!seam) DLV_TRY(net.norm_mish(x, C, d, q, ss, wb));
        else if constexpr (P::IS_F16) {
            DLV_TRY((net.template norm_mish<P, PBf16>(x, C, d, q, ss, wb)));
            q_f16 = false;
        } else {
            DLV_TRY((net.template norm_mish<PF16, P>(x, C, d, nullptr, ss, true)));
            out_f16 = true;
        }
        report();
        const dim3 g(net.grid1d(vox), C / 8, B);
        if (out_f16) hipLaunchKernelGGL(cp_to_f32_kernel<PF16>, g, dim3(256), 0, ctx->stream, x, a.out, C, vox);
        else hipLaunchKernelGGL(cp_to_f32_kernel<PBf16>, g, dim3(256), 0, ctx->stream, x, a.out, C, vox);
        if (q) {
            const dim3 gq(net.grid1d(pv), C / 8, B);
            if (q_f16) hipLaunchKernelGGL(cp_to_f32_kernel<PF16>, gq, dim3(256), 0, ctx->stream, q, a.out2, C, pv);
            else hipLaunchKernelGGL(cp_to_f32_kernel<PBf16>, gq, dim3(256), 0, ctx->stream, q, a.out2, C, pv);
        }
        DLV_LAUNCH_CHECK(ctx, "debug norm");
        return DLV_OK;
    }
    if (kind == 1) {
        if (a.op != DLV_DBG_CONV) return dlv_fail(ctx, DLV_EINVAL, "kind 1 (deconv) runs as op 0 only");
        const int index = a.index, c1 = a.c1;
        if (index < 0 || index >= DLV_N_DECONV) return dlv_fail(ctx, DLV_EINVAL, "deconv index must be 0..3");
        const DlvDeconvLayer& L = ctx->deconv[index];
        if (!a.in1 || c1 != L.cin || a.c2 != 0) return dlv_fail(ctx, DLV_EINVAL, "bad channels");
        const Dims du{2 * D, 2 * H, 2 * W};
        const Dims dskip = (a.sD | a.sH | a.sW) ? Dims{a.sD, a.sH, a.sW} : du;
        if (dskip.D < du.D || dskip.D > du.D + 1 || dskip.H < du.H || dskip.H > du.H + 1 || dskip.W < du.W || dskip.W > du.W + 1)
            return dlv_fail(ctx, DLV_EINVAL, "deconv: each skip dimension is 2 x the input's or one more");
        const size_t b1 = (size_t)B * c1 * vox * 2, bt = (size_t)B * L.cout * du.vox() * 2, bo = (size_t)B * L.cout * dskip.vox() * 2;
        char* base;
        DLV_TRY(dlv_ws_get(ctx, WS_BF16_ACT, al(b1) + al(bt) + al(bo) + 1024, (void**)&base));
        uint4 *i1 = (uint4*)base, *tmp = (uint4*)(base + al(b1)), *o = (uint4*)(base + al(b1) + al(bt));
        Net16<P> net{ctx, B, nullptr, 0, nullptr};
        hipLaunchKernelGGL(f32_to_cp_kernel<P>, dim3(net.grid1d(vox), c1 / 8, B), dim3(256), 0, ctx->stream, a.in1, i1, c1, vox);
        typename Net16<P>::Act t1{i1, c1, reinterpret_cast<const float2*>(a.ss1)};
        DLV_TRY(net.deconv_to(index, t1, o, tmp, d, dskip));
        report();
        hipLaunchKernelGGL(cp_to_f32_kernel<P>, dim3(net.grid1d(dskip.vox()), L.cout / 8, B), dim3(256), 0, ctx->stream, o, a.out,
                           L.cout, dskip.vox());
        DLV_LAUNCH_CHECK(ctx, "debug deconv");
        return DLV_OK;
    }
    if (kind != 0 && kind != 2 && kind != 3) return dlv_fail(ctx, DLV_EINVAL, "kind must be 0 (final), 1 (deconv), 2 (raw) or 3 (scale/shift)");
    // 2: raw conv output (no InstanceNorm / Mish), 3: the layer's scale/shift pairs
    const int li = a.op == DLV_DBG_STEM ? 0 : a.index;
    if (a.op == DLV_DBG_FOLDED && li != 16) return dlv_fail(ctx, DLV_EINVAL, "the folded conv is block 16");
    if (a.op == DLV_DBG_CONV && (li < 1 || li >= DLV_N_CONV)) return dlv_fail(ctx, DLV_EINVAL, "conv index must be 1..17");
    if (a.op < DLV_DBG_CONV || a.op > DLV_DBG_STEM) return dlv_fail(ctx, DLV_EINVAL, "op must be 0 (conv), 1 (folded) or 2 (stem)");
    const DlvConvLayer& L = ctx->conv[li];
    int c1 = a.c1, c2 = a.c2;
    long long vox2 = vox;  // voxels of in2 (the coarse tensor of the folded conv)
    if (a.op == DLV_DBG_STEM) {
        if (!a.vol) return dlv_fail(ctx, DLV_EINVAL, "the stem reads vol");
        if (a.flip_dim != -1 && (a.flip_dim < 2 || a.flip_dim > 4)) return dlv_fail(ctx, DLV_EINVAL, "flip_dim must be -1 or 2..4");
        c1 = c2 = 0;
    } else {
        if (!a.in1) return dlv_fail(ctx, DLV_EINVAL, "in1 missing");
        if (a.op == DLV_DBG_FOLDED) {
            if (c1 != 32 || c2 != 32 || !a.in2 || D % 2 || H % 2 || W % 2) return dlv_fail(ctx, DLV_EINVAL, "folded conv: 32 fine + 32 coarse channels, even sizes");
            vox2 = vox / 8;
        } else if (c1 + c2 != L.cin || c1 % 32 || c2 % 32 || (c2 && !a.in2)) {
            return dlv_fail(ctx, DLV_EINVAL, "bad channel split");
        }
    }
    const bool folded = a.op == DLV_DBG_FOLDED;
    const size_t b1 = (size_t)B * c1 * vox * 2, b2 = (size_t)B * c2 * vox2 * 2, bp = folded ? (size_t)B * 32 * vox * 2 : 0,
                 bo = (size_t)B * L.cout * vox * 2, bst = (size_t)B * 3 * sizeof(int);
    // partial sums: at most one row per 4 x 4 x 8 voxels (generic conv tiles; the z-march / z-reg / stem tiles are larger)
    const long long tiles = (long long)dlv_cdiv(D, 4) * dlv_cdiv(H, 4) * dlv_cdiv(W, 8) + 64;
    const size_t pf = (size_t)B * tiles * std::max(L.cout, 64) * 2;
    char* base;
    DLV_TRY(dlv_ws_get(ctx, WS_BF16_ACT, al(b1) + al(b2) + al(bp) + al(bo) + al(bst) + 1024, (void**)&base));
    char* sbase;
    DLV_TRY(dlv_ws_get(ctx, WS_STATS, al(pf * 4) + Net16<P>::ss_bytes(B) + 256, (void**)&sbase));
    uint4 *i1 = (uint4*)base, *i2 = (uint4*)(base + al(b1)), *pb = (uint4*)(base + al(b1) + al(b2)),
          *o = (uint4*)(base + al(b1) + al(b2) + al(bp));
    int* starts = (int*)(base + al(b1) + al(b2) + al(bp) + al(bo));
    Net16<P> net{ctx, B, (float*)sbase, pf, (float2*)(sbase + al(pf * 4))};
    const int g = net.grid1d(vox);
    if (c1) hipLaunchKernelGGL(f32_to_cp_kernel<P>, dim3(g, c1 / 8, B), dim3(256), 0, ctx->stream, a.in1, i1, c1, vox);
    if (c2) hipLaunchKernelGGL(f32_to_cp_kernel<P>, dim3(net.grid1d(vox2), c2 / 8, B), dim3(256), 0, ctx->stream, a.in2, i2, c2, vox2);
    DLV_LAUNCH_CHECK(ctx, "debug layer: f32_to_cp_kernel");
    bool final_written = false;  // (the activating stem pass stores the final tensor itself)
    if (a.op == DLV_DBG_STEM) {
        // B windows of one (B*D, H, W) volume: window n starts at plane n * D
        std::vector<int> st(3 * (size_t)B, 0);
        for (int n = 0; n < B; ++n) st[3 * n] = n * D;
        DLV_HIP(ctx, hipMemcpyAsync(starts, st.data(), bst, hipMemcpyHostToDevice, ctx->stream));
        DLV_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (st is a host temporary)
        const int tY = dlv_cdiv(H, SM_TY), tX = dlv_cdiv(W, SM_TX), tZ = dlv_cdiv(D, SM_TZ * SM_ZC);
        const dim3 grid(tZ * tY * tX, 1, B);
        if ((size_t)B * grid.x * 64 > pf) return dlv_fail(ctx, DLV_ESTATE, "partials buffer too small (stem)");
        const uint4* wst = reinterpret_cast<const uint4*>(wpack<P>(L));
        const uint16_t* vol = reinterpret_cast<const uint16_t*>(a.vol);
        if (kind == 2)  // raw tensor + statistics in one pass (the kernel's MODE 0)
            hipLaunchKernelGGL((stem_mfma_kernel<P, 0>), grid, dim3(256), 0, ctx->stream, vol, H, W, starts, a.flip_dim, wst,
                               L.bias16, o, net.partials, (const float2*)nullptr, D, H, W, tY, tX);
        else  // what a forward runs: statistics pass, then (kind 0) the activating pass
            hipLaunchKernelGGL((stem_mfma_kernel<P, 1>), grid, dim3(256), 0, ctx->stream, vol, H, W, starts, a.flip_dim, wst,
                               L.bias16, o, net.partials, (const float2*)nullptr, D, H, W, tY, tX);
        DLV_LAUNCH_CHECK(ctx, "debug stem_mfma_kernel");
        DLV_TRY(net.stats((int)grid.x, 0, d));
        if (kind == 0) {
            hipLaunchKernelGGL((stem_mfma_kernel<P, 2>), grid, dim3(256), 0, ctx->stream, vol, H, W, starts, a.flip_dim, wst,
                               L.bias16, o, net.partials, (const float2*)net.ss_of(0), D, H, W, tY, tX);
            DLV_LAUNCH_CHECK(ctx, "debug stem_mfma_kernel<2>");
            final_written = true;
        }
        a.ran_stem = 1;
        a.drops_bias = 1;  // (stem_mfma_kernel adds no bias)
        a.raw_scale = P::STEM_SCALE * exp2f(-(float)L.shift);
    } else {
        typename Net16<P>::Act t1{i1, c1, reinterpret_cast<const float2*>(a.ss1)}, t2{i2, c2, nullptr};
        if (folded) {
            if (!net.plan_fold(16, 32, d)) return dlv_fail(ctx, DLV_EUNSUP, "debug layer: a forward does not fold block 16 at %dx%dx%d", D, H, W);
            DLV_TRY(net.conv_folded(16, t1, t2, pb, o, d, Dims{D / 2, H / 2, W / 2}));
            a.drops_fold_const = 1;
        } else {
            DLV_TRY(net.conv(li, t1, c2 ? &t2 : nullptr, o, d));
        }
        a.raw_scale = exp2f(-(float)L.shift);
    }
    report();
    // (the z-reg conv and conv_deep.hip store no conv bias: the InstanceNorm removes it)
    a.drops_bias |= a.ran_zreg != 0 || a.ran_conv == DLV_PLAN_DEEP;
    if (kind == 3) {
        DLV_HIP(ctx, hipMemcpyAsync(a.out, net.ss_of(li), (size_t)B * L.cout * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
        return DLV_OK;
    }
    if (kind == 0 && !final_written) DLV_TRY(net.norm_mish(o, L.cout, d, nullptr, net.ss_of(li), true));  // (not part of the report)
    hipLaunchKernelGGL(cp_to_f32_kernel<P>, dim3(g, L.cout / 8, B), dim3(256), 0, ctx->stream, o, a.out, L.cout, vox);
    DLV_LAUNCH_CHECK(ctx, "debug layer");
    return DLV_OK;
}

}  // namespace

int dlv_pack_weights_bf16(dlv_ctx* ctx) {
    DLV_TRY(pack_weights_16<PBf16>(ctx));
    return pack_weights_16<PF16>(ctx);
}

// the workspaces `lanes` pipeline lanes of a 16-bit forward of B windows of d x h x w will ask for (dlv_reserve_dev): a pass needs
// ~10 GB per lane, and a large hipMalloc that follows a release of device memory can take seconds (profiles/r06r_alloc_probe2.json)
int dlv_unet_reserve_16(dlv_ctx* ctx, int B, int d, int h, int w, int lanes) {
    if (!ctx->weights_loaded && ctx->features[1] == 0) return DLV_OK;  // (channel counts unknown before dlv_unet_load / alloc_blob)
    const Ws16 wsz = ws16_bytes(ctx->features, B, d, h, w, nullptr);
    void* p;
    for (int lane = 0; lane < std::max(1, std::min(lanes, DLV_MAX_LANES)); ++lane) {
        DLV_TRY(dlv_ws_get(ctx, lane ? WS_LANE_ACT0 + (lane - 1) : WS_BF16_ACT, wsz.act, &p));
        DLV_TRY(dlv_ws_get(ctx, lane ? WS_LANE_STATS0 + (lane - 1) : WS_STATS, wsz.stats, &p));
    }
    return DLV_OK;
}

int dlv_range_reset(dlv_ctx* ctx) {
    DLV_HIP(ctx, hipMemsetAsync(ctx->range_flag, 0, sizeof(int) * (1 + DLV_N_CONV), ctx->main_stream));
    return DLV_OK;
}

// after everything of the pass / forward has been ordered behind the main stream: read the guard word back
int dlv_range_check(dlv_ctx* ctx, int fmt16) {
    const bool f16 = fmt16 != 0;  // (the mixed mode: only its fp16 level 0 can leave the range)
    int words[1 + DLV_N_CONV] = {0};
    DLV_HIP(ctx, hipMemcpyAsync(words, ctx->range_flag, sizeof(words), hipMemcpyDeviceToHost, ctx->main_stream));
    DLV_HIP(ctx, hipStreamSynchronize(ctx->main_stream));
    const int flag = words[0];
    for (int i = 0; i < DLV_N_CONV; ++i) memcpy(&ctx->range_peak[i], &words[1 + i], sizeof(float));
    ctx->range_last = flag == 0 ? -1 : 100 - flag;
    if (flag == 0) {
        ctx->range_seq = false;  // a pass came to its end: the recovery sequence (if any) is over
        ctx->range_blind_layer = -1;
        return DLV_OK;
    }
    const int layer = 100 - flag;
    static const char* const names[DLV_N_CONV] = {"conv_0.conv_0", "conv_0.conv_1", "down_1.conv_0", "down_1.conv_1", "down_2.conv_0",
                                                  "down_2.conv_1", "down_3.conv_0", "down_3.conv_1", "down_4.conv_0", "down_4.conv_1",
                                                  "upcat_4.conv_0", "upcat_4.conv_1", "upcat_3.conv_0", "upcat_3.conv_1", "upcat_2.conv_0",
                                                  "upcat_2.conv_1", "upcat_1.conv_0", "upcat_1.conv_1"};
    if (layer >= 0 && layer < DLV_N_CONV)
        return dlv_fail(ctx, DLV_ERANGE, "%s range exceeded: the InstanceNorm sums of conv block %d (%s) are not finite - a value of its input "
                        "(the block before it or the transposed conv feeding it) left the format%s", fmt16 == 2 ? "fp16 (level 0 of DLV_PREC_BF16)" : (f16 ? "fp16" : "bf16"), layer, names[layer],
                        f16 ? "; use dlv_unet_set_conv_shift on the producing block (dlv_range_report) or DLV_PREC_BF16_ALL (8 exponent bits) for this checkpoint" : "");
    return dlv_fail(ctx, DLV_ERANGE, "%s range exceeded: non-finite logits (raw output of the last conv block, upcat_1.conv_1)%s",
                    fmt16 == 2 ? "fp16 (level 0 of DLV_PREC_BF16)" : (f16 ? "fp16" : "bf16"), f16 ? "; use dlv_unet_set_conv_shift on upcat_1.conv_1 (dlv_range_report) or DLV_PREC_BF16_ALL (8 exponent bits) for this checkpoint" : "");
}

int dlv_unet_forward_bf16(dlv_ctx* ctx, const float* x, float* logits, int B, int d, int h, int w, int fmt16) {
    DLV_TRY(dlv_range_reset(ctx));
    if (fmt16 == 1) DLV_TRY(forward_16<PF16>(ctx, x, nullptr, 0, 0, nullptr, -1, 1.f, logits, nullptr, B, d, h, w));
    else if (fmt16 == 2) DLV_TRY((forward_16<PF16, PBf16>(ctx, x, nullptr, 0, 0, nullptr, -1, 1.f, logits, nullptr, B, d, h, w)));
    else DLV_TRY(forward_16<PBf16>(ctx, x, nullptr, 0, 0, nullptr, -1, 1.f, logits, nullptr, B, d, h, w));
    return dlv_range_check(ctx, fmt16);  // (dlv_unet_forward_dev is synchronous)
}

int dlv_unet_tiles_bf16(dlv_ctx* ctx, const uint16_t* vol, int Yp, int Xp, const int* starts_dev, int B, int d, int h,
                        int w, int flip_dim, float scale, float* acc, int fmt16) {
    if (fmt16 == 1) return forward_16<PF16>(ctx, nullptr, vol, Yp, Xp, starts_dev, flip_dim, scale, nullptr, acc, B, d, h, w);
    if (fmt16 == 2) return forward_16<PF16, PBf16>(ctx, nullptr, vol, Yp, Xp, starts_dev, flip_dim, scale, nullptr, acc, B, d, h, w);
    return forward_16<PBf16>(ctx, nullptr, vol, Yp, Xp, starts_dev, flip_dim, scale, nullptr, acc, B, d, h, w);
}

// test hook (include/delivr_hip_diag.h): one layer of the 16-bit path on fp32 NCDHW tensors (converted on the device) in the
// format of dlv_debug_set_format
extern "C" int dlv_debug_layer16(dlv_ctx* ctx, dlv_debug_layer_args* args) {
    if (!ctx || !args || (!args->out && !(args->op == DLV_DBG_FINAL && args->acc))) return DLV_EINVAL;  // (the blend writes no `out`)
    if (!ctx->weights_loaded) return dlv_fail(ctx, DLV_ESTATE, "no weights");
    DLV_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->debug_f16) return debug_layer_16<PF16>(ctx, *args);
    return debug_layer_16<PBf16>(ctx, *args);
}
