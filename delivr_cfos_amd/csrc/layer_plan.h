// layer_plan.h - which kernel runs each layer of the 16-bit U-Net forward, decided in one place.
//
// Pure host code (C++17, no HIP header, nothing of dlv_ctx): the forward (unet_bf16.hip: Net16 executes these plans), the
// weight blob layout (api.hip), the launchers' guards and dlv_diag_plan - the same decisions on a machine without a GPU -
// all read them here.  DESIGN section 4 lists the result for the default 128^3 window; tests/test_layer_plan_cpu.py holds
// that list against this file, tests/test_gpu_conv_kernels.py holds this file against what ran.
#pragma once
#include <cstdio>
#include <cstring>

#include "../../include/delivr_hip_diag.h"  // dlv_layer_plan and the DLV_PLAN_* kernel codes (plain C)

// Kernel-selection switches of tests and A/B runs (same results, other kernels).  The library takes NONE of them from the
// environment (a stray DLV_* in a user's shell must not change kernels): dlv_diag_set (include/delivr_hip_diag.h) sets them
// per context.
struct DlvPlanSwitches {
    bool no_zmarch = false;  // the generic conv kernel, the per-parity transposed conv and the VALU stem everywhere
    int zm_variant = 0;      // 0 / 50 = default; 51 = the LDS-weights z-march conv takes the z-reg layers too (A/B)
    int zreg_mask = 3;       // 1 = Cin 32, 2 = Cin 64 layers may take the register-resident-weights conv
    int deep_mask = 2;       // conv_deep.hip: bit 0 = the layers the LDS-weights z-march also takes, bit 1 = the others
    int deep_small = 1;      // 0 = levels smaller than a tile of conv_deep.hip and its 32-output-channel layers take the generic conv (A/B)
    int generic_ncb = 0;     // cout blocks per workgroup of the generic conv (0: its own choice)
    // bit li: conv block li applies the InstanceNorm + Mish of its first input itself while it stages the planes (no normalisation
    // pass over that tensor).  Default: block 17 (upcat_1.conv_1) only - the one site where it pays: -1.4...-1.7 % of a pass on every
    // workload, masks identical; block 16 (the raw skip tensor into the addend conv) +2.2 %, the level-1 sites +0.3...+0.9 %
    // (profiles/r06z_fuse_sites_ab.txt).  The level-wise switch of rounds 2-6 saw the two level-0 sites cancel.
    int fuse_layers = 1 << 17;
    int fuse_levels = 0;     // bit l: raw tensors of level l are activated by the z-reg conv that stages them (no norm pass)
    int fold_up = 1;         // fold the transposed conv into the first conv of upcat_1 (upconv.hip); "no_upconv": the unfolded path
    bool pool_rows_off = false;  // the pooling pass by pooled voxels instead of by full lines
};

// dlv_diag_set's names of the switches above.  REFUSED: the name is one of them and the value selects nothing - "zm_variant"
// takes 0, 50 and 51 only (the other numbers selected experiment builds of the z-march conv that were retired; profiles/README.md
// keeps their measurements).  The context and the host-only planner both come through here, so they refuse the same values.
enum DlvSwitchResult { DLV_SWITCH_UNKNOWN, DLV_SWITCH_SET, DLV_SWITCH_REFUSED };
inline DlvSwitchResult dlv_plan_switch_set(DlvPlanSwitches& s, const char* name, int value) {
    const auto is = [&](const char* n) { return strcmp(name, n) == 0; };
    if (is("no_zmarch")) s.no_zmarch = value != 0;
    else if (is("no_upconv")) s.fold_up = value ? 0 : 1;
    else if (is("zm_variant")) {
        if (value != 0 && value != 50 && value != 51) return DLV_SWITCH_REFUSED;
        s.zm_variant = value;
    } else if (is("fuse_levels")) s.fuse_levels = value;
    else if (is("fuse_layers")) s.fuse_layers = value;
    else if (is("zreg_mask")) s.zreg_mask = value;
    else if (is("deep_mask")) s.deep_mask = value;
    else if (is("generic_ncb")) s.generic_ncb = value;
    else if (is("deep_small")) s.deep_small = value;
    else if (is("pool_rows_off")) s.pool_rows_off = value != 0;
    else return DLV_SWITCH_UNKNOWN;
    return DLV_SWITCH_SET;
}

static inline int dlv_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- topology: MONAI BasicUNet with features f[0..5]; upcat_1 keeps its channels (halves=False) ---------------------------
constexpr int kDlvConvLevel[DLV_N_CONV] = {0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0};

inline void dlv_unet_channels(const int f[6], int cin[DLV_N_CONV], int cout[DLV_N_CONV], int dcin[DLV_N_DECONV], int dcout[DLV_N_DECONV]) {
    const int ci[DLV_N_CONV] = {1, f[0], f[0], f[1], f[1], f[2], f[2], f[3], f[3], f[4],
                                f[3] + f[4] / 2, f[3], f[2] + f[3] / 2, f[2], f[1] + f[2] / 2, f[1], f[0] + f[1], f[5]};
    const int co[DLV_N_CONV] = {f[0], f[0], f[1], f[1], f[2], f[2], f[3], f[3], f[4], f[4],
                                f[3], f[3], f[2], f[2], f[1], f[1], f[5], f[5]};
    const int di[DLV_N_DECONV] = {f[4], f[3], f[2], f[1]};
    const int dco[DLV_N_DECONV] = {f[4] / 2, f[3] / 2, f[2] / 2, f[1]};
    for (int i = 0; i < DLV_N_CONV; ++i) {
        cin[i] = ci[i];
        cout[i] = co[i];
    }
    for (int j = 0; j < DLV_N_DECONV; ++j) {
        dcin[j] = di[j];
        dcout[j] = dco[j];
    }
}
// every dimension at least 16 and more than one voxel at level 4: InstanceNorm3d has no statistics of a single value
inline bool dlv_window_supported(int d, int h, int w) {
    return d >= 16 && h >= 16 && w >= 16 && (long long)(d >> 4) * (h >> 4) * (w >> 4) >= 2;
}

// ---- which packs the weight blob holds (api.hip lays them out, the planner may only choose a kernel whose pack exists) ----
// conv block li gets the packs of the folded UpCat conv (32-channel skip half + transposed conv folded into the up half):
// upcat_1.conv_0 with a 32-channel skip and a 32 -> 32 transposed conv
inline bool dlv_conv_has_fold_pack(int li, int cin, int cout, int dcin3, int dcout3) {
    return li == 16 && cin == 64 && cout == 32 && dcin3 == 32 && dcout3 == 32;
}
// a transposed conv gets the 16-channel A-fragment pack of conv_deep.hip
inline bool dlv_deconv_has_w16_pack(int cin) { return cin >= 128; }

// ---- what each kernel family can run (the launchers call these as guards) ---------------------------------------------
inline bool dlv_conv3_zreg_supports(int cin, int cout, int c1, int c2, int W) {
    return cout % 32 == 0 && cout > 0 && W >= 32 &&
           ((cin == 32 && c1 == 32 && c2 == 0) || (cin == 64 && ((c1 == 32 && c2 == 32) || (c1 == 64 && c2 == 0))));
}
// z-reg tile height: 16 rows (Cin = 32 only) for windows large enough that 16 of them fill the chip with z-columns of at
// least 64 planes.  The choice depends on the window shape only, never on the batch size: the InstanceNorm partial
// sums are per tile, so a window's result must not depend on how many windows share its launch
inline int dlv_conv3_zreg_tile_rows(int cin, int cout, int D, int H, int W) {
    return (cin == 32 && H % 16 == 0 && (long long)(H / 16) * dlv_cdiv(W, 32) * (cout / 32) * dlv_cdiv(D, 64) >= 16) ? 16 : 8;
}
inline bool dlv_conv3_deep_supports(int cin, int cout, int c1, int c2, int D, int H, int W) {
    return cin % 32 == 0 && c1 % 32 == 0 && c2 % 32 == 0 && c1 + c2 == cin && cout % 32 == 0 && cout >= 32 && W >= 2 && H >= 2 && D >= 2 &&
           (long long)D * H * W <= 32768;
}
inline bool dlv_deconv2_deep_supports(int cin, int cout, int D, int H, int W) {
    return (cin == 128 || cin == 256) && cout % 64 == 0 && cout > 0 && (long long)D * H * W <= 32768 && W >= 1;
}
// the persistent upconv kernel (upconv.hip) walks whole 4 x 8 x 16 coarse tiles with 24-bit LDS-DMA and 31-bit store offsets
inline bool dlv_upconv2_persistent_shape(int Dc, int Hc, int Wc) {
    return Dc > 0 && Dc % 4 == 0 && Hc % 8 == 0 && Wc % 16 == 0 && ((long long)5 * Hc + 10) * Wc * 16 < (1 << 24) &&
           (long long)Dc * Hc * Wc * 8 * 16 * 2 < (1LL << 31);
}

// ---- conv blocks ------------------------------------------------------------------------------------------------------
struct DlvConvPlan {
    int kernel = DLV_PLAN_GENERIC;  // DLV_PLAN_ZREG / DEEP / ZMARCH / GENERIC
    int cin = 0, cout = 0;          // of the launch (a folded conv runs its 32-channel skip half)
    bool folded = false;            // skip half + addend P of the folded transposed conv (plan_conv_folded)
    int tile_rows = 0;              // ZREG: 8 or 16
    int tx = 0, ncb = 0;            // GENERIC: tile width (8 / 16), cout blocks per workgroup
    bool wlds = false;              // GENERIC: the slab's weights staged through LDS
    bool act_on_load = false;       // the first input is raw and the conv activates it while staging
    bool norm_first = false;        // the first input is raw and a normalisation pass makes it final first
    long long max_parts = 0;        // upper bound on the rows of InstanceNorm partial sums per sample (each cout x {sum, sum of squares})
};

// does the register-resident-weights conv run this layer?
inline bool dlv_plan_zreg_runs(const DlvPlanSwitches& sw, int cin, int cout, int c1, int c2, int D, int H, int W) {
    return (sw.zm_variant == 0 || sw.zm_variant == 50) && !sw.no_zmarch && (long long)D * H * W > 32768 &&
           dlv_conv3_zreg_supports(cin, cout, c1, c2, W) && ((cin == 32 ? 1 : 2) & sw.zreg_mask);
}
// Which raw tensors are activated by the consuming conv while it stages them: per conv block (fuse_layers) or per level
// (fuse_levels; A/B).  The Mish costs the staging conv issue cycles (one wave per SIMD), the separate pass costs HBM time: it
// pays where the pass it removes is a whole read + write of a level-0 tensor and nothing else changes; the transposed convs and
// the final 1x1x1 conv always activate on load.
inline bool dlv_plan_fuses_first_input(const DlvPlanSwitches& sw, int li, int cin, int cout, int c1, int c2, int D, int H, int W) {
    return (((sw.fuse_levels >> kDlvConvLevel[li]) & 1) || ((sw.fuse_layers >> li) & 1)) && c1 == 32 &&
           dlv_plan_zreg_runs(sw, cin, cout, c1, c2, D, H, W);
}

// conv block li (cin = c1 + c2 channels: the concatenation [first, second input]) on B windows of D x H x W; raw1: the first
// input still awaits its InstanceNorm + Mish
inline DlvConvPlan plan_conv(const DlvPlanSwitches& sw, int li, int cin, int cout, int c1, int c2, bool raw1, int B, int D, int H, int W) {
    DlvConvPlan p;
    p.cin = cin;
    p.cout = cout;
    p.act_on_load = raw1 && dlv_plan_fuses_first_input(sw, li, cin, cout, c1, c2, D, H, W);
    p.norm_first = raw1 && !p.act_on_load;
    const long long zm_parts = (long long)dlv_cdiv(H, 8) * dlv_cdiv(W, 32) * dlv_cdiv(D, 16);  // (8-row tiles: the 16-row ones are fewer)
    if (dlv_plan_zreg_runs(sw, cin, cout, c1, c2, D, H, W)) {
        p.kernel = DLV_PLAN_ZREG;
        p.tile_rows = dlv_conv3_zreg_tile_rows(cin, cout, D, H, W);
        p.max_parts = zm_parts;
        return p;
    }
    // deep levels (conv_deep.hip): weights shared through LDS, persistent workgroups.  deep_mask (A/B): bit 0 = the layers the
    // LDS-weights z-march takes (Cin, Cout <= 64 at the 32^3 level: 64->64 equal, 32->64 69 vs 78 us - they stay with the
    // z-march), bit 1 = the others (Cin or Cout >= 128: 1.4-1.5x the generic kernel's rate)
    const bool zmarch_ok = (cout == 32 || cout == 64) && (cin == 32 || cin == 64) && W >= 32;
    const bool deep_full = cout >= 64 && W >= 8 && H >= 8 && D >= 4;  // (what the kernel took before "deep_small")
    if (!sw.no_zmarch && ((zmarch_ok ? 1 : 2) & sw.deep_mask) && (deep_full || sw.deep_small) && dlv_conv3_deep_supports(cin, cout, c1, c2, D, H, W)) {
        p.kernel = DLV_PLAN_DEEP;
        p.max_parts = (long long)dlv_cdiv(D, 4) * dlv_cdiv(H, 8) * dlv_cdiv(W, 8);
        return p;
    }
    if (zmarch_ok && !sw.no_zmarch) {  // LDS-weights z-march (conv_zmarch.hip)
        p.kernel = DLV_PLAN_ZMARCH;
        p.max_parts = zm_parts;
        return p;
    }
    p.kernel = DLV_PLAN_GENERIC;
    p.tx = W >= 16 ? 16 : 8;
    const long long ntiles = (long long)dlv_cdiv(D, 4) * dlv_cdiv(H, 64 / p.tx) * dlv_cdiv(W, p.tx);
    // Two weight paths (A/B in profiles/README.md): fragments straight from L2 (levels 2-3: enough workgroups to
    // hide the latency; up to 4 cout blocks per workgroup) or the slab's weights staged through LDS in one
    // coalesced sweep (the 8^3 level: few workgroups, per-k-step fragment loads are latency-bound there).
    p.wlds = (long long)D * H * W <= 1024;
    p.ncb = p.wlds ? (cout >= 64 ? 2 : 1) : (cout >= 128 ? 4 : (cout >= 64 ? 2 : 1));
    while (p.ncb > 1 && (long long)B * ntiles * (cout / (32 * p.ncb)) < 512) p.ncb >>= 1;
    if (const int want = sw.generic_ncb)  // A/B switch (profiles/README.md)
        if ((want == 1 || want == 2 || (want == 4 && !p.wlds)) && cout % (32 * want) == 0) p.ncb = want;
    p.max_parts = ntiles;
    return p;
}

// is the first conv of an UpCat block (li, cout channels out of a cskip-channel skip tensor of D x H x W and an up-sampled
// one) run as skip-half conv + folded up half?  has_pack: the blob holds the folded packs (dlv_conv_has_fold_pack)
inline bool plan_folds_up(const DlvPlanSwitches& sw, bool has_pack, int cskip, int cout, int D, int H, int W) {
    return sw.fold_up && has_pack && cskip == 32 && (sw.zm_variant == 0 || sw.zm_variant == 50) && !sw.no_zmarch && (long long)D * H * W > 32768 &&
           dlv_conv3_zreg_supports(32, cout, 32, 0, W) && D % 2 == 0 && H % 2 == 0 && W % 2 == 0;
}
// ... and its conv: the 32-channel z-reg conv of the skip half with P as addend.  Whether it activates a raw skip tensor is
// decided as for the unfolded 32 + 32 conv (the pooling pass of level 0 must come to the same answer before it knows)
inline DlvConvPlan plan_conv_folded(const DlvPlanSwitches& sw, int li, int cout, bool raw1, int D, int H, int W) {
    DlvConvPlan p;
    p.kernel = DLV_PLAN_ZREG;
    p.folded = true;
    p.cin = 32;
    p.cout = cout;
    p.tile_rows = dlv_conv3_zreg_tile_rows(32, cout, D, H, W);
    p.act_on_load = raw1 && dlv_plan_fuses_first_input(sw, li, 64, cout, 32, 32, D, H, W);
    p.norm_first = raw1 && !p.act_on_load;
    p.max_parts = (long long)dlv_cdiv(H, 8) * dlv_cdiv(W, 32) * dlv_cdiv(D, 16);
    return p;
}

// ---- transposed convs (input D x H x W, output twice that) ----------------------------------------------------------------
struct DlvDeconvPlan {
    int kernel = DLV_PLAN_DC_PARITY;  // DLV_PLAN_DC_DEEP / REGW / WST / ROWS / PARITY, DLV_PLAN_NONE: Cin not in {32, 64, 128, 256}
    bool norm_first = false;          // the input is raw and a normalisation pass makes it final first (else: activated on load)
};
constexpr int DLV_DC_IPW = 8;  // deconv2_regw_kernel: row segments (16 input voxels -> 4 x 32 output voxels x 32 channels = 8 KB) per wave

inline DlvDeconvPlan plan_deconv(const DlvPlanSwitches& sw, int cin, int cout, bool raw, int D, int H, int W) {
    DlvDeconvPlan p;
    const bool rows = !sw.no_zmarch;
    // the per-parity kernel has no activation on load; the weight-stationary kernels of the deep levels (Cin >= 128) would
    // repeat it for every (parity, output block) they enumerate: there the (small) input is activated by one norm pass
    p.norm_first = raw && (!rows || cin >= 128);
    const long long segs = dlv_cdiv(W, 16), vox = (long long)D * H * W;
    // Cin 128 / 256 at the deep levels: weights shared through LDS (conv_deep.hip; deep_mask 0: the kernels before it)
    if (rows && sw.deep_mask != 0 && dlv_deconv_has_w16_pack(cin) && dlv_deconv2_deep_supports(cin, cout, D, H, W)) p.kernel = DLV_PLAN_DC_DEEP;
    else if (cin != 32 && cin != 64 && cin != 128 && cin != 256) p.kernel = DLV_PLAN_NONE;
    else if (!rows) p.kernel = DLV_PLAN_DC_PARITY;
    else if (cin >= 128) p.kernel = DLV_PLAN_DC_WST;
    // register-resident weights + segment pipeline where the weights fit (Cout = 32, Cin <= 64) and a window has enough
    // row segments (a property of the window shape, not of the batch); its stores address one sample's output with 32-bit offsets
    else if (cout == 32 && (long long)D * H * segs >= 4 * DLV_DC_IPW * 64 && vox * 8 * 4 * 16 < (1ll << 32)) p.kernel = DLV_PLAN_DC_REGW;
    else p.kernel = DLV_PLAN_DC_ROWS;
    return p;
}

// ---- InstanceNorm + Mish passes (pooled: with MaxPool3d(2) into a second tensor) -------------------------------------------
struct DlvNormPlan {
    bool rows = false;  // the pooling kernel that walks full lines (else: one (pooled) voxel per thread)
    bool nt = false;    // non-temporal loads / stores: a cache policy, the one plan field that follows the batch size
};
inline DlvNormPlan plan_norm_pass(const DlvPlanSwitches& sw, bool pooled, int B, int C, int D, int H, int W) {
    DlvNormPlan p;
    // a tensor far beyond L2 + MALL is streamed with the non-temporal policy (profiles/microbench/nt_probe.hip); the small
    // levels keep the default policy - their tensors are still on chip when the consumer starts
    p.nt = (double)D * H * W * B * C * 2 > 768.0 * (1 << 20);
    p.rows = pooled && W % 64 == 0 && !sw.pool_rows_off;
    return p;
}
// the stem of a forward that reads the uint16 volume: the MFMA kernel (two passes, writes final values), else the VALU one
inline bool plan_stem_mfma(const DlvPlanSwitches& sw, bool from_volume) { return from_volume && !sw.no_zmarch; }

// ---- labels: the DlvProf name with the algorithmic FLOPs and bytes of a launch (profiles/make_traffic.py and bench.py's
// kernel table match on the names) ----------------------------------------------------------------------------------------
struct DlvLabel {
    char name[48];
    double flops, bytes;
};
inline const char* dlv_fmt_name(bool f16) { return f16 ? "f16" : "bf16"; }

inline DlvLabel dlv_label_conv(const DlvConvPlan& p, bool f16, int B, int D, int H, int W) {
    static const char* const family[4] = {"zreg", "deep", "zmarch", "mfma"};
    DlvLabel l;
    const double vox = (double)((long long)D * H * W);
    snprintf(l.name, sizeof(l.name), "conv3_%s_%s_c%dx%d_d%d%s%s", family[p.kernel], dlv_fmt_name(f16), p.cin, p.cout, D, p.folded ? "_add" : "",
             p.act_on_load ? "_act" : "");
    l.flops = 2.0 * 27 * p.cin * p.cout * vox * B;
    l.bytes = 2.0 * vox * B * (p.cin + (p.folded ? 2 : 1) * p.cout);  // (folded: + the addend)
    if (p.kernel == DLV_PLAN_DEEP) l.bytes += 2.0 * 27 * p.cin * p.cout;  // (the weights once: at these levels 10-50 % of the activations)
    return l;
}
// the folded up half: P (B, 32, D, H, W) from the activated coarse tensor of half that size
inline DlvLabel dlv_label_upconv(bool persistent, bool f16, int B, int D, int H, int W) {
    DlvLabel l;
    const double vox = (double)((long long)D * H * W), voxc = (double)((long long)(D / 2) * (H / 2) * (W / 2));
    snprintf(l.name, sizeof(l.name), "upconv2%s_%s_c32x32_d%d", persistent ? "m" : "", dlv_fmt_name(f16), D / 2);
    l.flops = 2.0 * 8 * 32 * 32 * vox * B;
    l.bytes = 2.0 * 32 * (voxc + vox) * B;
    return l;
}
inline DlvLabel dlv_label_deconv(const DlvDeconvPlan& p, bool f16, int cin, int cout, int B, int D, int H, int W) {
    DlvLabel l;
    const double vox = (double)((long long)D * H * W);
    snprintf(l.name, sizeof(l.name), "deconv2_%s_%s_c%dx%d_d%d", p.kernel == DLV_PLAN_DC_DEEP ? "deep" : "mfma", dlv_fmt_name(f16), cin, cout, D);
    l.flops = 2.0 * 8 * cin * cout * vox * B;
    l.bytes = 2.0 * vox * B * (cin + 8.0 * cout);
    return l;
}
// f16: the format of the tensor read; seam: the written-back or the pooled tensor has the other format (mixed mode)
inline DlvLabel dlv_label_norm(bool pooled, bool writeback, bool f16, bool seam, int B, int C, int D, int H, int W) {
    DlvLabel l;
    const double vox = (double)((long long)D * H * W);
    snprintf(l.name, sizeof(l.name), "%s", pooled ? (writeback ? (f16 ? (seam ? "norm_mish_pool_f16_to_bf16" : "norm_mish_pool_f16") : "norm_mish_pool_bf16")
                                                               : (f16 ? "pool_act_f16" : "pool_act_bf16"))
                                                  : (f16 ? "norm_mish_f16" : (seam ? "norm_mish_bf16_to_f16" : "norm_mish_bf16")));
    l.flops = 0.0;
    l.bytes = vox * B * C * 2 * (writeback ? 2 : 1) + (pooled ? vox / 8 * B * C * 2 : 0.0);
    return l;
}
// UpCat's replicate padding of an up-sampled tensor (2D x 2H x 2W) to the skip tensor's odd size
inline DlvLabel dlv_label_pad(bool f16, int cout, int B, long long vox_up, long long vox_skip) {
    DlvLabel l;
    snprintf(l.name, sizeof(l.name), "%s", f16 ? "replicate_pad_f16" : "replicate_pad_bf16");
    l.flops = 0.0;
    l.bytes = 16.0 * B * (cout / 8) * ((double)vox_up + (double)vox_skip);
    return l;
}
inline DlvLabel dlv_label_stem(bool mfma, int B, int D, int H, int W) {
    DlvLabel l;
    const double vox = (double)((long long)D * H * W);
    snprintf(l.name, sizeof(l.name), "%s", mfma ? "stem_mfma_u16" : "stem_conv_f32");
    l.flops = 2.0 * 27 * 32 * vox * B;
    l.bytes = vox * B * (2 + 64);
    return l;
}
inline DlvLabel dlv_label_final(bool blend, int B, int D, int H, int W) {
    DlvLabel l;
    const double vox = (double)((long long)D * H * W);
    snprintf(l.name, sizeof(l.name), "%s", blend ? "final_conv_blend" : "final_conv_logits");
    l.flops = 2.0 * 32 * vox * B;
    l.bytes = vox * B * (64 + (blend ? 8 : 4));
    return l;
}

// ---- one forward of the sliding-window pass (stem from the uint16 volume, final conv blending), as forward_16 walks it ----
// fmt16: 0 = bf16 everywhere, 1 = fp16 everywhere, 2 = fp16 at level 0 + bf16 below.  false: window or features unsupported.
inline bool dlv_plan_forward(const DlvPlanSwitches& sw, bool upconv_simple, const int f[6], int fmt16, int B, int d, int h, int w, dlv_layer_plan* out) {
    memset(out, 0, sizeof(*out));
    if (f[0] != 32 || f[5] != 32 || B < 1 || !dlv_window_supported(d, h, w)) return false;
    for (int i = 0; i < 6; ++i)
        if (f[i] <= 0 || f[i] % 32 || f[i] > 256) return false;
    int cin[DLV_N_CONV], cout[DLV_N_CONV], dcin[DLV_N_DECONV], dcout[DLV_N_DECONV];
    dlv_unet_channels(f, cin, cout, dcin, dcout);
    struct Dm {
        int D, H, W;
        long long vox() const { return (long long)D * H * W; }
    } dm[5];
    for (int l = 0; l < 5; ++l) dm[l] = Dm{d >> l, h >> l, w >> l};
    const bool mixed = fmt16 == 2;
    const auto f16_at = [&](int level) { return level == 0 ? fmt16 != 0 : fmt16 == 1; };
    const auto emit = [&](const DlvLabel& l) {
        if (out->n_labels >= DLV_PLAN_MAX_LABELS) return;
        memcpy(out->labels[out->n_labels], l.name, sizeof(l.name));
        out->flops[out->n_labels] = l.flops;
        out->bytes[out->n_labels] = l.bytes;
        ++out->n_labels;
    };
    struct T {
        int C;
        bool raw;
    };
    // fl: the level whose format the pass reads (the level-0 net also touches level-1 tensors in upcat_1)
    const auto materialise = [&](T& t, int level, int fl, bool seam) {
        if (!t.raw) return;
        emit(dlv_label_norm(false, true, f16_at(fl), seam, B, t.C, dm[level].D, dm[level].H, dm[level].W));
        t.raw = false;
    };
    const auto record = [&](int li, const DlvConvPlan& p, int level) {
        dlv_plan_conv& c = out->conv[li];
        c.kernel = p.kernel;
        c.level = level;
        c.cin = p.cin;
        c.cout = p.cout;
        c.folded = p.folded;
        c.tile_rows = p.tile_rows;
        c.act_on_load = p.act_on_load;
        c.tx = p.tx;
        c.ncb = p.ncb;
        c.wlds = p.wlds;
        c.max_parts = p.max_parts;
        emit(dlv_label_conv(p, f16_at(level), B, dm[level].D, dm[level].H, dm[level].W));
    };
    const auto conv = [&](int li, T& a1, int c2, int level) {
        const DlvConvPlan p = plan_conv(sw, li, cin[li], cout[li], a1.C, c2, a1.raw, B, dm[level].D, dm[level].H, dm[level].W);
        if (p.norm_first) materialise(a1, level, level, false);
        record(li, p, level);
        return T{cout[li], true};
    };
    // transposed conv j of a tensor of level l + 1 into level l, by the net of level `fl`
    const auto deconv_to = [&](int j, T& a, int l, int fl) {
        const Dm din = dm[l + 1], sk = dm[l];
        const DlvDeconvPlan p = plan_deconv(sw, dcin[j], dcout[j], a.raw, din.D, din.H, din.W);
        if (p.norm_first) materialise(a, l + 1, fl, false);
        out->deconv[j].kernel = p.kernel;
        out->deconv[j].norm_first = p.norm_first;
        emit(dlv_label_deconv(p, f16_at(fl), dcin[j], dcout[j], B, din.D, din.H, din.W));
        out->deconv[j].padded = 2 * din.D != sk.D || 2 * din.H != sk.H || 2 * din.W != sk.W;
        if (out->deconv[j].padded) emit(dlv_label_pad(f16_at(fl), dcout[j], B, 8 * din.vox(), sk.vox()));
    };

    const bool stem_mfma = plan_stem_mfma(sw, true);
    out->conv[0].kernel = stem_mfma ? DLV_PLAN_STEM_MFMA : DLV_PLAN_STEM_VALU;
    out->conv[0].cin = 1;
    out->conv[0].cout = 32;
    emit(dlv_label_stem(stem_mfma, B, d, h, w));
    T x0{32, !stem_mfma};
    T skip[5];
    skip[0] = conv(1, x0, 0, 0);
    for (int l = 1; l <= 4; ++l) {
        T& up = skip[l - 1];
        const int li_cat = 18 - 2 * l, c_up = dcout[4 - l];
        const Dm dp = dm[l - 1];
        const bool keep_raw = plan_conv(sw, li_cat, cin[li_cat], cout[li_cat], up.C, c_up, true, B, dp.D, dp.H, dp.W).act_on_load;
        const bool odd = ((dp.D | dp.H | dp.W) & 1) != 0;
        const DlvNormPlan np = plan_norm_pass(sw, true, B, up.C, dp.D, dp.H, dp.W);
        dlv_plan_pool& pl = out->pool[l - 1];
        pl.rows = np.rows;
        pl.nt = np.nt;
        pl.writeback = !keep_raw && !odd;
        pl.norm_after = odd && !keep_raw;
        emit(dlv_label_norm(true, pl.writeback, f16_at(l - 1), l == 1 && mixed, B, up.C, dp.D, dp.H, dp.W));
        if (pl.norm_after) emit(dlv_label_norm(false, true, f16_at(l - 1), false, B, up.C, dp.D, dp.H, dp.W));
        up.raw = keep_raw;
        T a{l == 1 ? 32 : f[l - 1], false};
        T b = conv(2 * l, a, 0, l);
        skip[l] = conv(2 * l + 1, b, 0, l);
    }
    T cur = skip[4];
    for (int j = 0; j < 4; ++j) {
        const int l = 3 - j, li = 10 + 2 * j;
        T b;
        if (l == 0 && mixed) materialise(cur, 1, 1, true);  // (level-1 output activated and written in the level-0 format)
        if (l == 0 && plan_folds_up(sw, dlv_conv_has_fold_pack(li, cin[li], cout[li], dcin[3], dcout[3]), skip[0].C, cout[li], d, h, w)) {
            const DlvConvPlan p = plan_conv_folded(sw, li, cout[li], skip[0].raw, d, h, w);
            materialise(cur, 1, 0, false);
            if (p.norm_first) materialise(skip[0], 0, 0, false);
            emit(dlv_label_upconv(!upconv_simple && dlv_upconv2_persistent_shape(dm[1].D, dm[1].H, dm[1].W), f16_at(0), B, d, h, w));
            record(li, p, 0);
            out->deconv[j].kernel = DLV_PLAN_NONE;
            b = T{cout[li], true};
        } else {
            deconv_to(j, cur, l, l);
            b = conv(li, skip[l], dcout[j], l);
        }
        cur = conv(li + 1, b, 0, l);
    }
    emit(dlv_label_final(true, B, d, h, w));
    return true;
}
