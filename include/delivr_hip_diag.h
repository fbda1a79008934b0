/* delivr_hip_diag.h - test hooks and A/B switches of libdelivr_hip.so.  NOT part of the drop-in boundary (include/delivr_hip.h):
 * nothing here replaces a reference interface; tests/ and profiles/ use these to run one layer in isolation or to select another
 * kernel for the same result.  Nothing in the library is switched through the environment. */
#ifndef DELIVR_HIP_DIAG_H
#define DELIVR_HIP_DIAG_H
#include "delivr_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Kernel-selection switches of one context (same results up to the 16-bit rounding of one store, other kernels):
 *   "no_zmarch" 1         the generic conv kernel for every layer (and the VALU stem)
 *   "no_upconv" 1         upcat_1 as transposed conv + 64-channel conv instead of the folded form (upconv.hip)
 *   "upconv_simple" 1     the one-tile-per-workgroup upconv kernel for every shape
 *   "fuse_levels" mask    bit l: raw tensors of level l are activated by the z-reg conv that stages them (no normalisation pass)
 *   "fuse_layers" mask    bit li: conv block li activates its first input itself (default 1 << 17: upcat_1.conv_1, the one site that
 *                         pays; 0 = a normalisation pass in front of every conv)
 *   "zreg_mask" mask      1 = Cin 32, 2 = Cin 64 layers may take the register-resident-weights conv (default 3)
 *   "deep_mask" mask      conv_deep.hip: bit 0 = the layers the LDS-weights z-march also takes, bit 1 = the others (default 2)
 *   "generic_ncb" n       cout blocks per workgroup of the generic conv (0: its own choice)
 *   "zm_variant" v        0 / 50: default; 51: the LDS-weights z-march conv (conv_zmarch.hip) for every layer the
 *                         register-resident-weights conv would take (an A/B that gives the same results).  Every other value
 *                         selected an experiment build of the z-march conv; they were retired and are refused with DLV_EUNSUP.
 *   "zreg_dbg" 1          edge-step code on every plane of the z-reg conv
 *   "deep_small" 0        levels smaller than a tile of conv_deep.hip, and its 32-output-channel layers, take the generic conv
 *   "pool_rows_off" 1     the pooling pass by pooled voxels instead of by full lines
 *   "erode_xy_split" 1, "erode_z_two_sweeps" 1, "ccl_simple" 1, "resample_simple" 1, "resample_run16" 1
 *                         the earlier kernels of finalize / CCL / the resamplers (cross-checks in tests/test_gpu_parity.py)
 *   "ccl_init_grid" n     at most n workgroups for ccl_init_kernel (0: its own choice): a workgroup that owns 2048 chunks or more
 *                         flushes its chunk buffer inside its loop (tests/test_gpu_ccl_kernels.py); no other kernel, same labels
 *   "tiff_chunk" n        planes per pinned staging chunk of dlv_tiff_stack_to_device (0: ~256 MB): the hand-over between the two
 *                         staging buffers on stacks of small planes (tests/test_gpu_pipeline.py)
 * DLV_EINVAL for an unknown name. */
int dlv_diag_set(dlv_ctx* ctx, const char* name, int value);

/* What the last dlv_ccl26_dev of this context launched, recorded at its launch sites:
 *   aligned      mask and labels both start on a 16-byte boundary (16-byte loads and stores)
 *   merge_rows   1: ccl_merge_list_kernel<true> (row windows; aligned and X % 16 == 0), 0: the per-voxel merge
 *   relabel      0: ccl_relabel_list_kernel (memset + listed chunks), 1: ccl_relabel_lines_kernel, 2: ccl_relabel_kernel ("ccl_simple")
 *   init_grid    workgroups of ccl_init_kernel, init_per: the 16-voxel chunks each of them owns (a multiple of 256)
 *   blocks       4096-voxel blocks of the renumbering, groups: the 1024-block groups of its two-level scan
 *   list_n       chunks with foreground that ccl_init_kernel listed (read back with the number of labels)
 * All 0 before the first labelling. */
typedef struct dlv_ccl_ran {
    int aligned, merge_rows, relabel, init_grid;
    uint64_t init_per, blocks, groups, list_n;
} dlv_ccl_ran;
int dlv_diag_ccl_ran(dlv_ctx* ctx, dlv_ccl_ran* out);

/* What the last dlv_finalize_dev / dlv_finalize_slab_dev of this context launched, recorded at its launch sites (reset at the
 * start of every call; all 0 after a call that was refused before its first launch, and before the first call):
 *   xy_form   0: erode_xy_kernel (x and y fused), 1: erode_x_bits_kernel + erode_y_kernel, 2: erode_x_kernel (log-step) +
 *             erode_y_kernel
 *   nc        8-voxel chunks per thread of erode_xy_kernel (1 / 2 / 4; 0 when not fused)
 *   y_v       voxels per thread of erode_y_kernel (4 / 1; 0 when fused)
 *   z_form    0: erode_z_shift_kernel (one sweep), 1: erode_z_final_kernel (two sweeps); z_v: its voxels per thread (4 / 1)
 *   nblk      z-blocks the z kernel walks, zphase: absolute plane of the first local plane modulo the block size
 *   raw_vec   the kernel that reads the raw volume takes whole 8-voxel chunks with 16-byte loads (Xp % 8 == 0 and the volume on a
 *             16-byte boundary: every row then starts on one; always 0 for the log-step kernel)
 *   dist_vec  ... and stores their distances with 8-byte stores (X % 8 == 0 and the distance map on an 8-byte boundary; always
 *             0 for the log-step kernel)
 *   acc_vec   erode_z_shift_kernel<4> reads the sums with 16-byte loads (Xp % 4 == 0 and the sums on a 16-byte boundary; 0 for
 *             every other z kernel)
 * The three *_vec fields are the host-side values of the conditions the kernels evaluate. */
typedef struct dlv_finalize_ran {
    int xy_form, nc, y_v, z_form, z_v, nblk, zphase, raw_vec, dist_vec, acc_vec;
} dlv_finalize_ran;
int dlv_diag_finalize_ran(dlv_ctx* ctx, dlv_finalize_ran* out);

/* selects the 16-bit format dlv_debug_layer16 runs in (DLV_PREC_BF16 default, DLV_PREC_F16) */
int dlv_debug_set_format(dlv_ctx* ctx, int precision);

/* The layer test hook: one layer of the 16-bit path in the format of
 * dlv_debug_set_format, through the same dispatch as a forward, on fp32 NCDHW device tensors.
 *   op 0 (DLV_DBG_CONV)   kind 0/2/3: conv block `index` (1..17) on [in1 (c1), in2 (c2)]; ss1 (device float2 [B][c1], may be
 *                         NULL): in1 is RAW and awaits InstanceNorm scale/shift ss1 + Mish - the dispatcher (fuse_layers /
 *                         fuse_levels) decides whether the conv activates it while staging or a normalisation pass runs first.
 *                         kind 1: transposed conv `index` (0..3) of in1 -> raw output (B, Cout, sD, sH, sW).  With ss1 in1 is RAW:
 *                         plan_deconv decides between activation on load and a normalisation pass first (ran_norm_passes).
 *                         sD / sH / sW (all 0: 2D, 2H, 2W): the skip tensor's dimensions, each 2 x the input's or one more -
 *                         then the output is replicate-padded at the far end as UpCat does (ran_pad).
 *   op 1 (DLV_DBG_FOLDED) the folded first conv of upcat_1 (block 16): in1 = fine skip tensor (B, 32, D, H, W), raw if ss1 is
 *                         given, in2 = ACTIVATED coarse tensor (B, 32, D/2, H/2, W/2); DLV_EUNSUP where a forward would not fold.
 *   op 2 (DLV_DBG_STEM)   block 0 from vol (device uint16 (B, D, H, W): B windows) flipped along flip_dim (2/3/4, -1 none)
 *                         through the MFMA stem (kind 0: statistics pass + activating pass, kind 2/3: raw pass).
 *   op 3 (DLV_DBG_NORM)   an InstanceNorm + Mish pass over the raw in1 (B, c1, D, H, W) with scale/shift ss1: out = the tensor
 *                         as the pass leaves it (activated; with out2 and writeback 0: still raw), out2 (may be NULL) = the
 *                         MaxPool3d(2) of the activated tensor (B, c1, D/2, H/2, W/2).  fmt_out 1: the format seam of the mixed
 *                         mode - format fp16: the pooled tensor is written in bf16 (out2 required); format bf16: the activated
 *                         tensor is written in fp16 (no out2).  kind is ignored.
 *   op 4 (DLV_DBG_FINAL)  the final 1x1x1 conv on the raw in1 (B, 32, D, H, W) with scale/shift ss1 -> fp32 logits (B, D, H, W)
 *                         (no blending).  kind is ignored.  With acc (device fp32, planes of Yp x Xp): the BLEND instantiation
 *                         through the launcher a pass uses - window n of the forward of a window flipped along flip_dim is
 *                         un-flipped and added at starts[3n .. 3n+2] = (z, y, x) (host ints, copied by the hook):
 *                         acc += scale * logit (scale 0: 1), or with bw (device, D + H + W factors)
 *                         acc += g * logit, wsum (may be NULL) += g, g = max(bw[z] bw[D + y] bw[D + H + x], bmin) * scale at the
 *                         window coordinate (z, y, x) in volume orientation.  out is not written.  DLV_EINVAL for another
 *                         flip_dim, a non-finite scale or bmin, wsum without bw, or a window that leaves the Yp x Xp planes (the
 *                         caller answers for the planes: acc and wsum hold at least max(z) + D of them).
 * kind 0: final output (B, Cout, D, H, W); 2: raw output in the stored scale (see below); 3: scale/shift pairs (float2 [B][Cout]).
 * Reported: ran_zreg (DLV_DBG_ZR_* bits of the z-reg instantiation that ran, 0: another kernel), ran_upconv (1 one tile per
 * workgroup, 2 persistent, 0 none), ran_stem (1: stem_mfma_kernel), and how the raw output relates to conv3d + bias:
 *   raw = raw_scale * (conv3d(x, W) + (drops_bias ? 0 : bias) - (drops_fold_const ? sum_taps W_up * bias_up : 0))
 * raw_scale = 2^-shift of the block (dlv_unet_set_conv_shift), times STEM_SCALE (2^-8 in fp16) for the stem.
 * What the launchers of the other families ran (recorded at the launch sites, not read from the plan):
 *   ran_conv    DLV_PLAN_ZREG / DEEP / ZMARCH / GENERIC of the conv launch, -1: none; with it ran_tx / ran_ncb (DEEP, GENERIC: the
 *               template parameters; ZMARCH: cout blocks), ran_wlds (GENERIC), ran_grid (workgroups; DEEP, ZMARCH) and ran_items
 *               (DEEP: work items the persistent workgroups walk)
 *   ran_deconv  DLV_PLAN_DC_* of the transposed-conv launch, -1: none; ran_gpw: 64-channel groups per workgroup (DC_DEEP);
 *               ran_pad: replicate_pad_cp_kernel ran
 *   ran_norm    of the LAST normalisation pass: DLV_DBG_NM_* bits (0: none ran); ran_norm_passes: how many ran */
#define DLV_DBG_CONV 0
#define DLV_DBG_FOLDED 1
#define DLV_DBG_STEM 2
#define DLV_DBG_NORM 3
#define DLV_DBG_FINAL 4
#define DLV_DBG_ZR_RAN 1
#define DLV_DBG_ZR_F16 2
#define DLV_DBG_ZR_C64 4
#define DLV_DBG_ZR_T16 8
#define DLV_DBG_ZR_ACT 16
#define DLV_DBG_ZR_ADD 32
#define DLV_DBG_NM_RAN 1
#define DLV_DBG_NM_ROWS 2      /* norm_mish_pool_rows_kernel (else norm_mish_kernel) */
#define DLV_DBG_NM_POOLED 4
#define DLV_DBG_NM_WRITEBACK 8
#define DLV_DBG_NM_NT 16       /* non-temporal instantiation */
#define DLV_DBG_NM_SEAM 32     /* written-back or pooled tensor in the other 16-bit format */
typedef struct dlv_debug_layer_args {
    int kind, op, index;
    const float* in1;
    int c1;
    const float* ss1;
    const float* in2;
    int c2;
    const unsigned short* vol;
    int flip_dim;
    float* out;
    int B, D, H, W;
    /* reported */
    int ran_zreg, ran_upconv, ran_stem, drops_bias, drops_fold_const;
    float raw_scale;
    /* further inputs (0 / NULL: as before) */
    int sD, sH, sW;
    float* out2;
    int writeback, fmt_out;
    /* reported */
    int ran_conv, ran_tx, ran_ncb, ran_wlds, ran_grid, ran_items;
    int ran_deconv, ran_gpw, ran_pad;
    int ran_norm, ran_norm_passes;
    /* DLV_DBG_FINAL blending into an accumulator (acc NULL: plain logits, as before) */
    const int* starts;
    float* acc;
    int Yp, Xp;
    float scale;
    const float* bw;
    float bmin;
    float* wsum;
} dlv_debug_layer_args;
int dlv_debug_layer16(dlv_ctx* ctx, dlv_debug_layer_args* args);

/* Which kernel runs each layer of ONE 16-bit forward of a sliding-window pass (stem from the uint16 volume, final conv
 * blending) of B windows of d x h x w, without running it: host arithmetic only (delivr_cfos_amd/csrc/layer_plan.h, what the
 * forward itself consults) - no context, no HIP call, no GPU.  names / values: n switches as given to the switch setter above;
 * fmt16: 0 = bf16 everywhere, 1 = fp16, 2 = fp16 at level 0 + bf16 below (DLV_PREC_BF16).
 * DLV_EINVAL for an unknown switch or a value the setter refuses, DLV_EUNSUP for features or a window the 16-bit forward refuses. */
#define DLV_PLAN_NONE (-1)       /* not launched (deconv 3 when upcat_1 is folded) */
#define DLV_PLAN_ZREG 0          /* conv_zreg_kernel.h: register-resident weights */
#define DLV_PLAN_DEEP 1          /* conv_deep.hip */
#define DLV_PLAN_ZMARCH 2        /* conv_zmarch.hip: LDS-resident weights */
#define DLV_PLAN_GENERIC 3       /* conv3_mfma_kernel */
#define DLV_PLAN_STEM_MFMA 4     /* conv[0] only */
#define DLV_PLAN_STEM_VALU 5
#define DLV_PLAN_DC_DEEP 0       /* transposed convs: conv_deep.hip, */
#define DLV_PLAN_DC_REGW 1       /* register-resident weights, */
#define DLV_PLAN_DC_WST 2        /* weight-stationary, */
#define DLV_PLAN_DC_ROWS 3       /* row segments, */
#define DLV_PLAN_DC_PARITY 4     /* one output parity per launch item */
#define DLV_PLAN_MAX_LABELS 96
typedef struct dlv_plan_conv {
    int kernel, level, cin, cout; /* cin / cout of the launch: the folded block 16 runs its 32-channel skip half */
    int folded;                   /* upconv + z-reg conv with addend */
    int tile_rows;                /* ZREG: 8 / 16 */
    int act_on_load;              /* the conv activates its raw first input while staging (no normalisation pass) */
    int tx, ncb, wlds;            /* GENERIC: tile width, cout blocks per workgroup (the one field that follows B), weights through LDS */
    long long max_parts;          /* bound on the InstanceNorm partial-sum rows per sample */
} dlv_plan_conv;
typedef struct dlv_plan_deconv {
    int kernel;     /* DLV_PLAN_DC_*, DLV_PLAN_NONE */
    int norm_first; /* a normalisation pass makes its input final first (else: activated on load) */
    int padded;     /* followed by UpCat's replicate padding (odd skip tensor) */
} dlv_plan_deconv;
typedef struct dlv_plan_pool { /* the pass that pools level l into level l + 1 */
    int rows;       /* the kernel that walks full lines (else one pooled voxel per thread) */
    int writeback;  /* it also writes the activated level-l tensor back */
    int norm_after; /* odd level: pool only, then a full normalisation pass */
    int nt;         /* non-temporal policy (a tensor far beyond the caches: follows B, changes no value) */
} dlv_plan_pool;
typedef struct dlv_layer_plan {
    dlv_plan_conv conv[DLV_N_CONV];
    dlv_plan_deconv deconv[DLV_N_DECONV];
    dlv_plan_pool pool[4];
    int n_labels;                          /* kernel-timer labels in launch order, with their algorithmic FLOPs and bytes */
    char labels[DLV_PLAN_MAX_LABELS][48];
    double flops[DLV_PLAN_MAX_LABELS], bytes[DLV_PLAN_MAX_LABELS];
} dlv_layer_plan;
int dlv_diag_plan(const int features[6], const char* const* names, const int* values, int n, int fmt16, int B, int d, int h, int w,
                  dlv_layer_plan* out);

#ifdef __cplusplus
}
#endif
#endif /* DELIVR_HIP_DIAG_H */
