/* delivr_hip.h - C ABI of libdelivr_hip.so: the MI355X (gfx950) implementation of DELiVR's tiled
 * 3D-U-Net cFos inference path.
 *
 * The reference (erturklab/delivr_cfos) has no FFI layer: its boundary for this path is Python
 * calls + .npy files.  Each entry point below names the reference interface it replaces
 * (file:line relative to the reference root).  The Python host package (delivr_cfos_amd/) binds
 * these with ctypes and mirrors the reference's step API on top; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - every function returns int: 0 = DLV_OK, negative = DLV_E*; dlv_last_error(ctx) returns a
 *     message owned by the ctx (valid until the next call on that ctx).
 *   - no C++ exception and no HIP error code crosses the ABI.
 *   - pointers are caller-owned.  "_dev" parameters are device (HBM) pointers on the ctx's
 *     device; all others are host pointers.  Sizes are explicit; nothing allocated by the
 *     library is handed to the caller (scratch lives in the ctx and is freed by dlv_ctx_destroy).
 *   - volumes are C-order (Z,Y,X), X contiguous ("z-major slabs"), exactly the payload of the
 *     reference's .npy files (inference/inference.py:234, count_blobs.py:46).
 *   - a ctx is bound to one device and one HIP stream and is NOT thread-safe; distinct ctxs are
 *     independent.  Calls are asynchronous on the ctx stream unless documented "synchronous";
 *     dlv_sync() waits for the stream.
 */
#ifndef DELIVR_HIP_H
#define DELIVR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLV_OK 0
#define DLV_EINVAL (-1)   /* bad argument */
#define DLV_EHIP (-2)     /* a HIP runtime call failed (message has the HIP error string) */
#define DLV_ENOMEM (-3)   /* device allocation failed */
#define DLV_ESTATE (-4)   /* call order violated (e.g. forward before dlv_unet_load) */
#define DLV_EUNSUP (-5)   /* shape not supported by the kernels */
#define DLV_ERANGE (-6)   /* a 16-bit forward produced a non-finite value: the format's range was exceeded (fp16: use bf16) */

/* 2 (round 6): DLV_PREC_BF16 is the mixed format, DLV_PREC_BF16_ALL added; dlv_set_cu_split / dlv_set_conv_algo gone, the range
 * guard entry points (dlv_unet_set_conv_shift ... dlv_comm_range_recover) added and the weight blob re-laid out in round 5; the
 * dlv_debug_* hooks moved to delivr_hip_diag.h.  A host built against version 1 must be rebuilt: dlv_abi_version() tells. */
#define DLV_ABI_VERSION 2

/* compute precision of the U-Net forward */
#define DLV_PREC_F32 0  /* fp32 VALU kernels, NCDHW: parity mode (matches torch fp32 to ~1e-5) */
#define DLV_PREC_BF16 1 /* MFMA implicit-GEMM kernels, fp32 accumulate + fp32 norm statistics: bf16 operands and storage at levels
                           1-4 of the U-Net, IEEE half at level 0 (full resolution), where bf16's 8 significant bits cost the mask
                           its tolerance - the format changes in two normalisation passes */
#define DLV_PREC_F16 2  /* the same kernels on IEEE-half operands everywhere (11 significant bits, same MFMA rate): the default */
#define DLV_PREC_BF16_ALL 3 /* bf16 at every level (8 significant bits, fp32's exponent range): the last resort of the range guard */

#define DLV_N_CONV 18
#define DLV_N_DECONV 4

typedef struct dlv_ctx dlv_ctx;

/* ---- context ------------------------------------------------------------------------------ */
int dlv_abi_version(void);
/* stream == NULL: the ctx creates (and owns) a non-blocking HIP stream; otherwise it adopts the
 * caller's hipStream_t.  Replaces the device set-up at inference/inference.py:153-160. */
int dlv_ctx_create(int device_id, void* stream, dlv_ctx** out);
int dlv_ctx_destroy(dlv_ctx* ctx);
const char* dlv_last_error(dlv_ctx* ctx);
int dlv_sync(dlv_ctx* ctx);
void* dlv_stream(dlv_ctx* ctx); /* the hipStream_t kernels are launched on */

/* plain device-memory helpers so that a host without torch can drive the library */
int dlv_malloc(dlv_ctx* ctx, size_t bytes, void** out_dev);
int dlv_free(dlv_ctx* ctx, void* p_dev);
int dlv_memset_dev(dlv_ctx* ctx, void* p_dev, int value, size_t bytes);
int dlv_copy_h2d(dlv_ctx* ctx, void* dst_dev, const void* src, size_t bytes); /* synchronous */
int dlv_copy_d2h(dlv_ctx* ctx, void* dst, const void* src_dev, size_t bytes); /* synchronous */

/* ---- U-Net weights ------------------------------------------------------------------------ */
/* MONAI BasicUNet(3,1,1,features,act=mish,norm=instance-affine) parameters as fp32 host arrays
 * taken from the checkpoint's state_dict (inference/inference.py:190-200,222).  Conv layers are
 * listed in forward order:
 *   0 conv_0.conv_0   1 conv_0.conv_1   2,3 down_1.convs.conv_{0,1}   4,5 down_2   6,7 down_3
 *   8,9 down_4   10,11 upcat_4.convs   12,13 upcat_3.convs   14,15 upcat_2.convs   16,17 upcat_1.convs
 * conv_w[i]: (Cout,Cin,3,3,3); norm_g/norm_b: InstanceNorm3d affine weight/bias (Cout).
 * deconv_w[j] (j=0..3 = upcat_4..upcat_1): ConvTranspose3d weight (Cin,Cout,2,2,2).
 * final_w: (1,features[5],1,1,1). */
typedef struct dlv_unet_weights {
    int features[6];
    const float* conv_w[DLV_N_CONV];
    const float* conv_b[DLV_N_CONV];
    const float* norm_g[DLV_N_CONV];
    const float* norm_b[DLV_N_CONV];
    const float* deconv_w[DLV_N_DECONV];
    const float* deconv_b[DLV_N_DECONV];
    const float* final_w;
    const float* final_b;
} dlv_unet_weights;

/* copies (and re-packs for the MFMA kernels) the weights into HBM.  Synchronous. */
int dlv_unet_load(dlv_ctx* ctx, const dlv_unet_weights* w);
/* multi-GPU: after dlv_unet_load on the root rank the packed weight blob can be broadcast
 * (RCCL, by the host) instead of re-reading the checkpoint on every rank
 * (replaces DataParallel's per-forward broadcast_coalesced, inference/inference.py:217-219). */
int dlv_unet_blob_size(dlv_ctx* ctx, size_t* bytes);
int dlv_unet_blob_dev(dlv_ctx* ctx, void** blob_dev); /* device pointer owned by ctx */
int dlv_unet_alloc_blob(dlv_ctx* ctx, const int features[6]); /* non-root ranks: allocate only */

/* ---- U-Net forward (one batch of patches) -------------------------------------------------- */
/* logits = BasicUNet(x): x_dev (B,1,d,h,w) fp32 -> logits_dev (B,1,d,h,w) fp32; d,h,w >= 16 and
 * (d/16)*(h/16)*(w/16) > 1 (DLV_EUNSUP otherwise: torch raises there too); multiples of 16 keep every level
 * even, elsewhere MaxPool3d's dropped plane and UpCat's replicate padding as in MONAI.  Replaces predictor(window_data) at inference/sliding_window_inferer.py:222. */
int dlv_unet_forward_dev(dlv_ctx* ctx, const float* x_dev, float* logits_dev, int B, int d, int h, int w,
                         int precision);

/* ---- sliding-window pass ------------------------------------------------------------------- */
typedef struct dlv_sw_params {
    int Zp, Yp, Xp;      /* padded volume shape (inference/inference.py:229-231) */
    int roi[3];          /* window size (Z,Y,X) = config window_dim_0/1/2 (inference.py:162-168) */
    float overlap;       /* 0.5 in the reference (inference.py:127,211) */
    int flip_dim;        /* -1 none, 2 = Z, 3 = Y, 4 = X (sliding_window_inferer.py:218-226) */
    int skip_threshold;  /* window_data_threshold (sliding_window_inferer.py:52,198): a window whose
                            max <= threshold is not inferred and contributes -1000; decided PER
                            WINDOW (= the reference at sw_batch_size 1) */
    int precision;       /* DLV_PREC_* */
    int sw_batch;        /* windows per forward launch (0 = library default) */
    int64_t win_begin;   /* shard: windows [win_begin, win_end) of the reference's enumeration */
    int64_t win_end;     /* (Z slowest, X fastest); win_end <= 0 means "to the end" */
    int z0, nz;          /* the buffers below hold planes [z0, z0+nz) of the padded volume; every
                            window of the shard must lie inside (nz <= 0: whole volume) */
    int repeat;          /* this call stands for `repeat` identical passes (>= 1): acc += repeat*logit,
                            cnt += repeat.  The reference's 13-pass TTA schedule (inference.py:265-279)
                            has only 3 distinct passes once its <=1e-3 noise is dropped (5:4:4) */
    int blend_mode;      /* DLV_BLEND_CONSTANT (0): weights 1 - what the reference does, its mode="gaussian" argument
                            never reaches compute_importance_map (sliding_window_inferer.py:148).
                            DLV_BLEND_GAUSSIAN (1): MONAI 1.2.0's Gaussian importance map (sigma = sigma_scale*roi,
                            truncated at 4 sigma, erf form, normalised to max 1, floored at its smallest non-zero
                            value): acc += w*logit, wsum += w.  Option; no reference output exists for it. */
    float sigma_scale;   /* Gaussian mode: 0.125 in the reference's constructor call (inference.py:206); <= 0 -> 0.125 */
    float* wsum_dev;     /* Gaussian mode: optional fp32 (nz,Yp,Xp) sum of weights (the float count map); cnt_dev must
                            be NULL in that mode */
} dlv_sw_params;
#define DLV_BLEND_CONSTANT 0
#define DLV_BLEND_GAUSSIAN 1

typedef struct dlv_sw_stats {
    int64_t n_windows;   /* windows in the shard */
    int64_t n_skipped;   /* of which background-skipped */
    int64_t n_forward_launches;
} dlv_sw_stats;

/* number of windows the reference enumerates for this geometry (sliding_window_inferer.py:140-145) */
int dlv_sw_num_windows(const dlv_sw_params* p, int64_t* n_windows);
/* writes the (z0,y0,x0) start of every window in the reference's order: starts[3*n] */
int dlv_sw_window_starts(const dlv_sw_params* p, int64_t* starts, int64_t capacity);

/* Per-window maximum of the uint16 volume, in the reference's window order (the quantity the skip test of
 * sliding_window_inferer.py:198 looks at): wmax[n_windows] on the host.  Lets a multi-rank host balance its
 * shards by NON-background windows before calling dlv_sw_infer_dev.  p->win_begin/win_end and p->z0/nz are honoured
 * (wmax[i] = window win_begin + i, from a slab of the volume): the ranks of a sharded run each compute a part.  Synchronous. */
int dlv_sw_window_max_dev(dlv_ctx* ctx, const dlv_sw_params* p, const uint16_t* vol_dev, int32_t* wmax, int64_t capacity);

/* One pass of sliding_window_inference (inference/sliding_window_inferer.py:161-251) with the
 * volume resident in HBM: gather + cast, per-window background skip, optional flip, U-Net forward,
 * un-flip, acc += logit (fp32; the reference accumulates fp16), cnt += 1.
 * vol_dev: uint16 (nz,Yp,Xp); acc_dev: fp32 (nz,Yp,Xp) in/out; cnt_dev: uint8 (nz,Yp,Xp) in/out or
 * NULL.  Synchronous with respect to the host only for the small skip-list read-back. */
int dlv_sw_infer_dev(dlv_ctx* ctx, const dlv_sw_params* p, const uint16_t* vol_dev, float* acc_dev,
                     uint8_t* cnt_dev, dlv_sw_stats* stats);

/* ---- one process, N devices (replaces torch.nn.DataParallel, inference/inference.py:217-219) ------------------------
 * The reference scatters every sw-batch over the visible GPUs, re-broadcasts all parameters per forward and gathers the
 * logits through GPU 0.  Here: a static partition of the reference's window list (Z slowest) into contiguous ranges - a
 * rank's windows form a Z-slab of tile rows -, ONE broadcast of the packed weights, and ONE point-to-point exchange per
 * seam and pass (the planes a rank computed but another rank owns).  Every rank holds only ITS slab of the volume and of
 * the accumulator.  RCCL (ncclBroadcast, grouped ncclSend/ncclRecv over xGMI) is loaded at dlv_comm_init_all; there is
 * no all-reduce on this path.  The multi-process form of the same plan (one process per GPU, torch.distributed) lives in
 * delivr_cfos_amd/parallel.py. */
#define DLV_MAX_RANKS 16
typedef struct dlv_comm dlv_comm;
typedef struct dlv_shard_plan {
    int world;
    int64_t n_windows;
    int64_t win_begin[DLV_MAX_RANKS], win_end[DLV_MAX_RANKS]; /* [begin, end) of the reference's window enumeration */
    int z_comp_lo[DLV_MAX_RANKS], z_comp_hi[DLV_MAX_RANKS];   /* planes [lo, hi) the rank's windows touch ((0,0): none) */
    int z_own_lo[DLV_MAX_RANKS], z_own_hi[DLV_MAX_RANKS];     /* planes [lo, hi) the rank finalizes: a partition of [0, Zp) */
} dlv_shard_plan;
/* Host-only integer logic.  weights == NULL: equal windows, cuts snap to Z tile-row boundaries; otherwise weights[n_windows]
 * (e.g. 1 for a window that runs the network, 0.02 for a background-skipped one, from dlv_sw_window_max_dev) balance the
 * cumulative work.  Ownership: [0, Zp) split at the midpoints of the seams between consecutive non-empty ranks. */
int dlv_shard_plan_make(const dlv_sw_params* p, int world, const float* weights, dlv_shard_plan* out);
/* planes [*z0, *z0 + *nz) a rank must hold: its windows' planes and the planes it owns extended by erode_iters planes
 * inside their z-blocks (zblock <= 0: one block; Z = unpadded stack depth) - what dlv_finalize_slab_dev needs */
int dlv_shard_slab(const dlv_shard_plan* plan, int rank, int Z, int erode_iters, int zblock, int* z0, int* nz);
/* one context per entry of devs (rank r <-> devs[r]) and one RCCL communicator per device (ncclCommInitAll); ranks that
 * share a device (a test on a one-GPU box) exchange with device copies instead.  DLV_EUNSUP: several devices, no librccl. */
int dlv_comm_init_all(int n, const int* devs, dlv_comm** out);
int dlv_comm_destroy(dlv_comm* c);
int dlv_comm_size(dlv_comm* c);
/* 1 when the communicator moves data with RCCL (several distinct devices, or one device with DLV_FORCE_RCCL=1 in the
 * environment of dlv_comm_init_all: a 1-rank ncclCommInitAll), 0 for the device-copy transport of ranks sharing a device */
int dlv_comm_uses_rccl(dlv_comm* c);
/* Transport check before a long job: every rank sends `bytes` (a multiple of 4) to the next rank of the ring - itself when
 * there is one rank - with the grouped ncclSend/ncclRecv the seam exchange uses, then rank 0's buffer is broadcast
 * (ncclBroadcast, like the weight blob); everything received is compared word for word on the host.  DLV_ESTATE + message
 * on a mismatch.  Synchronous.  No reference counterpart (DataParallel has no such check). */
int dlv_comm_selftest(dlv_comm* c, size_t bytes);
dlv_ctx* dlv_comm_ctx(dlv_comm* c, int rank); /* owned by the communicator */
/* c == NULL: why the calling thread's last dlv_comm_init_all failed - for DLV_EUNSUP the librccl paths that were tried
 * ($DLV_RCCL_PATH, a librccl.so already mapped into the process, $ROCM_PATH/lib/librccl.so, then the soname). */
const char* dlv_comm_last_error(dlv_comm* c);
/* dlv_unet_load was called on rank `root`: every other rank allocates the blob and receives it with ONE ncclBroadcast */
int dlv_bcast_weights(dlv_comm* c, int root);
/* dlv_range_recover for every rank of the communicator (see the range guard below): one decision, the same shifts everywhere. */
int dlv_comm_range_recover(dlv_comm* c, int* n_changed /* or NULL */);
/* One sliding-window pass sharded over the communicator.  Rank r's buffers hold planes [slab_z0[r], slab_z0[r]+slab_nz[r])
 * of the padded volume (vol: uint16, acc: fp32 in/out, cnt: uint8 in/out or cnt_slab_dev == NULL), on device devs[r]; they
 * must cover the rank's z_comp and z_own ranges.  p->win_begin/win_end/z0/nz are ignored (taken from the plan).  After the
 * call the planes a rank OWNS hold the complete sums: a neighbour's partial sum is added as one term, in increasing
 * source-rank order - the result is fixed by the plan and does not depend on arrival order; against the single-device
 * pass it is the same terms in another association (fp32 rounding; the count map is exact).  stats: [world] or NULL.
 * Synchronous.  The planes a rank computed but does not own still hold its partial sums afterwards: a host that runs several
 * passes into the same slabs zeroes them between the calls (the owner has added them).  Gaussian blend over several ranks
 * with p->wsum_dev set: DLV_EINVAL (one buffer cannot be every rank's weight sums) - use dlv_sw_infer_sharded_wsum. */
int dlv_sw_infer_sharded(dlv_comm* c, const dlv_sw_params* p, const dlv_shard_plan* plan, const int* slab_z0, const int* slab_nz,
                         const uint16_t* const* vol_slab_dev, float* const* acc_slab_dev, uint8_t* const* cnt_slab_dev,
                         dlv_sw_stats* stats);
/* dlv_sw_infer_sharded plus one fp32 (slab_nz[r],Yp,Xp) weight-sum slab per rank for the Gaussian blend (wsum_slab_dev[r] on
 * devs[r], in/out; NULL: no weight sums); p->wsum_dev is ignored.  The seam exchange moves the weight sums beside the sums
 * and the owner adds them in the same increasing source-rank order, so the planes a rank owns hold the complete weight sums
 * too.  Constant mode ignores wsum_slab_dev.  Synchronous. */
int dlv_sw_infer_sharded_wsum(dlv_comm* c, const dlv_sw_params* p, const dlv_shard_plan* plan, const int* slab_z0,
                              const int* slab_nz, const uint16_t* const* vol_slab_dev, float* const* acc_slab_dev,
                              uint8_t* const* cnt_slab_dev, float* const* wsum_slab_dev, dlv_sw_stats* stats);

/* ---- finalize: divide, threshold, eroded re-mask ------------------------------------------- */
/* inference/inference.py:285-299 + create_nifti_seg (:31-95).  mean = acc/cnt; cnt_dev == NULL: acc_dev already holds
 * the MEAN logits - or, for threshold == 0.5 ONLY, any positive multiple of them such as the plain sum (the sign decides);
 * a caller with another threshold must pass the count map (the Python mirror enforces it).  fg = sigmoid(mean) >= threshold, keep = raw>0 eroded
 * by an L1 ball of radius erode_iters evaluated inside z-blocks of zblock planes (0 = whole
 * volume; the reference's Arrayterator rule gives floor(floor(1e9/X)/Y)), out = fg & keep.
 * erode_iters in [0, 253]; 0 means NO erosion (keep = raw > 0), unlike scipy's binary_erosion(iterations=0), which repeats
 * until nothing changes.
 * acc/cnt/raw are (.,Yp,Xp)-strided padded buffers, out_dev is the unpadded (Z,Y,X) uint8
 * binaries.npy payload; prob_dev (nullable) receives sigmoid(mean) as fp32 (Z,Y,X)
 * (network_output.npy, inference.py:312-318). */
int dlv_finalize_dev(dlv_ctx* ctx, const float* acc_dev, const uint8_t* cnt_dev, const uint16_t* raw_dev,
                     int Yp, int Xp, int Z, int Y, int X, float threshold, int erode_iters, int zblock,
                     uint8_t* out_dev, float* prob_dev);
/* the same on a Z-slab: the buffers hold planes [z_abs0, z_abs0 + nz) of the stack and the erosion's z-blocks sit at
 * absolute multiples of zblock (the reference's Arrayterator grid), so that a rank of a sharded run reproduces the
 * single-volume result on the planes it owns.  Planes beyond the slab count as foreground: the caller includes
 * erode_iters planes of margin unless the slab ends on a block boundary (dlv_shard_slab).  out/prob: (nz, Y, X). */
int dlv_finalize_slab_dev(dlv_ctx* ctx, const float* acc_dev, const uint8_t* cnt_dev, const uint16_t* raw_dev, int Yp, int Xp,
                          int z_abs0, int nz, int Y, int X, float threshold, int erode_iters, int zblock, uint8_t* out_dev,
                          float* prob_dev);

/* ---- connected components + statistics ------------------------------------------------------ */
/* cc3d.connected_components(bin_img, return_N=True), connectivity 26 (count_blobs.py:61): labels
 * 1..N in C-raster order of each component's first voxel, 0 = background.  labels_dev: uint32
 * (Z,Y,X).  Synchronous (returns N). */
int dlv_ccl26_dev(dlv_ctx* ctx, const uint8_t* mask_dev, int Z, int Y, int X, uint32_t* labels_dev,
                  uint64_t* n_out);
/* cc3d.statistics(labels, no_slice_conversion=True) (count_blobs.py:85): host outputs sized n+1:
 * voxel_counts uint32; bounding_boxes uint16 (n+1,6) = z0,z1,y0,y1,x0,x1 inclusive; centroids
 * float64 (n+1,3) = coordinate sums / count (row 0 = background).  Synchronous. */
int dlv_cc_stats_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n,
                     uint32_t* voxel_counts, uint16_t* bounding_boxes, double* centroids);

/* The cell table as the reference writes it (count_blobs.py:98-114: a pandas frame of Blob / Coords / Size rows for labels 1..N-1 -
 * `range(1, N)` drops the last label - through DataFrame.to_csv): header ",Blob,Coords,Size", then per label
 * `0,<label>,"[z, y, x]",<voxel count>` with the centroid as Python writes a list of floats (repr: the shortest digits that
 * round-trip, ".0" on integral values, exponent form below 1e-4 and from 1e16).  Host-only (no context, no GPU): 540 k rows take
 * ~0.1 s instead of 0.8 s of Python string formatting.  voxel_counts / centroids: the outputs of dlv_cc_stats_dev.  out / cap:
 * caller-owned text buffer (128 bytes per label are enough); *len_out = bytes written (no terminator); DLV_EINVAL when the buffer
 * is too small. */
int dlv_cells_csv(const uint32_t* voxel_counts, const double* centroids, uint64_t n, char* out, size_t cap, size_t* len_out);

/* Multi-GPU CCL (one process per GPU, every rank labels its own Z-slab with dlv_ccl26_dev): the pieces of the seam
 * merge that run on the device.  The reference has no counterpart - cc3d labels the whole volume on one core
 * (count_blobs.py:61); the contract is that the merged result is identical to that single-volume labelling.
 *  dlv_seam_pairs_dev: plane_a = labels of the LAST plane of a slab, plane_b = labels of the FIRST plane of the slab
 *    below it (both (Y,X) uint32).  Writes every (label_a, label_b) pair that is 26-adjacent across the seam (with
 *    repeats) to pairs_dev (cap pairs of 2 x uint32) and the number of pairs found to *count_out; pairs_dev == NULL
 *    counts only.  Synchronous.
 *  dlv_relabel_u32_dev: labels[i] = lut[labels[i]] for labels[i] != 0 (lut_len = n_local + 1, lut[0] unused).
 *  dlv_cc_stats_raw_dev: the accumulators behind dlv_cc_stats_dev, host arrays of n+1 rows: counts uint32, bbmin /
 *    bbmax uint32 (n+1,3) in z,y,x (0xffffffff / 0 for an absent label), coordinate sums uint64 (n+1,3); row 0
 *    (background) carries its bounding box only.  Synchronous. */
int dlv_seam_pairs_dev(dlv_ctx* ctx, const uint32_t* plane_a_dev, const uint32_t* plane_b_dev, int Y, int X,
                       uint32_t* pairs_dev, uint64_t cap, uint64_t* count_out);
int dlv_relabel_u32_dev(dlv_ctx* ctx, uint32_t* labels_dev, uint64_t nvox, const uint32_t* lut_dev, uint64_t lut_len);
int dlv_cc_stats_raw_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, uint32_t* counts,
                         uint32_t* bbmin, uint32_t* bbmax, uint64_t* sums);
/* Size filter on a label volume (what cc3d users know as cc3d.dust; count_blobs' min_size / max_size).  The reference has no
 * counterpart: it accepts the two bounds and ignores them.  Two calls, so that a sharded run can add up the counts of its
 * slabs in between.  labels_dev: nvox uint32 labels 0..n, 4-byte aligned (16-byte aligned volumes take the 16-byte path).
 *  dlv_cc_counts_dev: counts_dev[l] = number of voxels with label l, for l = 0..n (device array of n+1 uint32; labels above
 *    n are not counted).  Asynchronous on the context's stream.
 *  dlv_cc_size_filter_dev: label l >= 1 is kept when min_size <= counts_dev[l] <= max_size (both inclusive; a negative
 *    bound is no bound).  The kept labels are renumbered 1..K in the order they had, the others become 0, in place: the
 *    volume is the labelling of the mask without the removed components.  *n_kept_out = K.  Both bounds negative: K = n and
 *    nothing is touched; min_size > max_size with both >= 0: DLV_EINVAL.  Synchronous. */
int dlv_cc_counts_dev(dlv_ctx* ctx, const uint32_t* labels_dev, uint64_t nvox, uint64_t n, uint32_t* counts_dev);
int dlv_cc_size_filter_dev(dlv_ctx* ctx, uint32_t* labels_dev, uint64_t nvox, uint64_t n, const uint32_t* counts_dev,
                           int64_t min_size, int64_t max_size, uint64_t* n_kept_out);
/* Per-label statistics of a raw uint16 volume under a label volume (no counterpart in the reference).
 * labels_dev: uint32 (Z,Y,X) contiguous, labels 0..n; raw_dev: uint16, voxel (z,y,x) at raw_dev[z*raw_pitch_z + y*raw_pitch_y + x]
 * (pitches in elements: the raw file is padded to window multiples, the labels are not). Host outputs of n+1 rows:
 * sum, sumsq uint64 (exact), vmin, vmax uint16. A label with no voxel in this volume: sum 0, sumsq 0, vmin 0xFFFF, vmax 0 -
 * so two slabs merge with +, +, min, max. Row 0 (background) is not measured and always reads like an absent label. Labels above n
 * are not accumulated. raw_pitch_y < X, raw_pitch_z < Y*raw_pitch_y, a NULL pointer or Z/Y/X < 1: DLV_EINVAL. Synchronous. */
int dlv_cc_intensity_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint16_t* raw_dev, int Z, int Y, int X,
                         int64_t raw_pitch_y, int64_t raw_pitch_z, uint64_t n,
                         uint64_t* sum, uint64_t* sumsq, uint16_t* vmin, uint16_t* vmax);
/* Per-label confidence: statistics of the network's blended probabilities under a label volume (no counterpart in the reference,
 * whose users take them on the host). prob_dev: float32 (Z,Y,X) contiguous and unpadded, like labels_dev (uint32, labels 0..n) - the
 * volume dlv_finalize_dev leaves in prob_dev and run_inference writes as binary_segmentations/network_output.npy with
 * FLAGS.SAVE_ACTIVATED_OUTPUT (the reference: inference/inference.py:312-318). Every probability p is taken in fixed point,
 * q(p) = (uint32) rint(clamp(p, 0, 1) * 2^24): NaN counts as 0, +inf as 1, -inf as 0, the product is exact in float32 and rint rounds
 * half to even; for p >= 0.5 q loses nothing. Host outputs of n+1 rows, over the voxels that hold the label: sum_q uint64, min_q and
 * max_q uint32, peak_index uint64 = the linear index (z*Y + y)*X + x, inside the volume handed in, of the voxel of largest q, the first
 * in C-raster order on a tie. A label with no voxel in this volume, and row 0 (the background is not measured): 0, 0xFFFFFFFF, 0 and
 * 2^64 - 1 - so two slabs merge with +, min, max and "larger q, then smaller global index". Labels above n are not accumulated. Integer
 * work only after q: exact and independent of scheduling. A NULL pointer, Z/Y/X < 1, Z*Y*X >= 2^39 (the peak's index has 39 bits),
 * n >= 2^32 - 1 or a pointer not 4-byte aligned: DLV_EINVAL before any launch. Synchronous. */
int dlv_cc_confidence_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const float* prob_dev, int Z, int Y, int X, uint64_t n,
                          uint64_t* sum_q, uint32_t* min_q, uint32_t* max_q, uint64_t* peak_index);
/* Per-label order statistics of a raw uint16 volume under a label volume (no counterpart in the reference). For a label l with
 * m >= 1 voxels whose raw values sorted ascending are v[0] <= ... <= v[m-1], and a level p in per cent: Q_p(l) = v[(p * (m - 1)) / 100]
 * (integer division) - the "lower" quantile, always a value the label holds; p = 50 is the lower median, p = 0 / 100 the minimum /
 * maximum. labels_dev, raw_dev, the pitches and the alignment rules as for dlv_cc_intensity_dev. levels: host, n_levels = 1..8
 * integers 0..100, strictly increasing. Host outputs: out uint16 (n+1) x n_levels row-major, counts uint32 n+1 = the voxels
 * measured per label; row 0 (background) and a label without a voxel read 0 with a count of 0 - the count tells an absent label from
 * a true 0. Labels above n are not measured. Exact, and independent of scheduling. Device scratch: 2 bytes per foreground voxel, 12
 * bytes per label and the result table; DLV_ENOMEM names the sizes. A NULL pointer, Z/Y/X < 1, bad pitches, n >= 2^32 - 1, a
 * misaligned pointer or a bad level list: DLV_EINVAL, nothing written. Synchronous. */
int dlv_cc_quantiles_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint16_t* raw_dev, int Z, int Y, int X,
                         int64_t raw_pitch_y, int64_t raw_pitch_z, uint64_t n, int n_levels, const int* levels,
                         uint16_t* out, uint32_t* counts);
/* The background shell of every component (no counterpart in the reference): E_0 = labels; E_{k+1}(v) = E_k(v) where that is not
 * 0, else the smallest non-zero E_k over the 26 neighbours of v inside the volume (0 without one), every step from E_k alone;
 * shell(v) = E_radius(v) where labels(v) == 0 and raw(v) != 0, else 0 - the smallest label among the cells nearest to v in
 * Chebyshev distance, when that distance is at most radius. dlv_cc_intensity_dev / dlv_cc_counts_dev on shell_dev measure it.
 * labels_dev (not modified), raw_dev and the pitches as for dlv_cc_intensity_dev; raw_dev may be NULL: the raw != 0 condition is
 * dropped (labels_dev + shell_dev are then the expanded labels). shell_dev: Z*Y*X uint32, fully written. scratch_dev: a second
 * volume of that size, may be NULL with radius 1. radius outside 1..16, a NULL pointer, Z/Y/X < 1, bad pitches, a misaligned
 * pointer (4 / 2 bytes) or labels_dev / shell_dev / scratch_dev overlapping: DLV_EINVAL. Asynchronous on the context's stream. */
int dlv_cc_shell_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint16_t* raw_dev, int Z, int Y, int X,
                     int64_t raw_pitch_y, int64_t raw_pitch_z, int radius, uint32_t* shell_dev, uint32_t* scratch_dev);
/* Per-label shape accumulators of a label volume (no counterpart in the reference): second-order moments of the voxel coordinates
 * and the exposed faces. labels_dev: uint32 (Zb,Y,X) contiguous, labels 0..n. The voxels of the buffer's planes
 * [z_first, z_first + nz) are measured, the other planes only serve as neighbours (the halo planes of a slab of a sharded run). The
 * absolute z of buffer plane k is z_abs0 + k; y and x are the buffer's own. Host outputs of n+1 rows: counts uint32 (measured
 * voxels), sums uint64 (n+1,3) = sum z, y, x, moments uint64 (n+1,6) = sum zz, yy, xx, zy, zx, yx (absolute coordinates), faces
 * uint64 (n+1,3) = per axis z, y, x the pairs (measured voxel of label l, direction +-axis) whose face neighbour has a label != l or
 * lies outside the buffer (z outside [0, Zb), or outside the Y / X range), surface_voxels uint32 = measured voxels with at least one
 * such face. All exact. Row 0 (background) and a label without a measured voxel are all zero, so slabs merge by addition. Labels
 * above n are not accumulated, and differ from every label as a neighbour. A NULL pointer, Zb/Y/X < 1, nz < 1, z_first < 0,
 * z_first + nz > Zb, z_abs0 < 0, n >= 2^32 - 1 or labels not 4-byte aligned: DLV_EINVAL; z_abs0 + Zb, Y or X above 65536:
 * DLV_EUNSUP (as dlv_cc_stats_dev). Synchronous. */
int dlv_cc_shape_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Zb, int Y, int X, int z_first, int nz, int z_abs0, uint64_t n,
                     uint32_t* counts, uint64_t* sums, uint64_t* moments, uint64_t* faces, uint32_t* surface_voxels);
/* Per-label depth from the exact label-wise Euclidean distance map (no counterpart in the reference, whose users call
 * scipy.ndimage.distance_transform_edt per cell on the host; csrc/cc_depth.hip). labels_dev: uint32 (Z,Y,X) contiguous, labels 0..n,
 * not modified; wz, wy, wx: the voxel spacings, integers 1..64. For a voxel v with 1 <= labels(v) <= n
 *   D2(v) = min over u with labels(u) != labels(v) of (wz (vz - uz))^2 + (wy (vy - uy))^2 + (wx (vx - ux))^2,
 * where every position outside the volume counts as background: a cell cut by a face of the volume is shallow there and D2 is always
 * finite. D2(v) = 0 where labels(v) is 0 or above n; a label above n still differs from every label as a neighbour (as in
 * dlv_cc_shape_dev), and a touching cell of another label bounds a cell exactly as the background does. Integer work only: exact
 * and independent of scheduling. work_a_dev, work_b_dev: two scratch volumes of Z*Y*X uint32; on return work_a_dev holds D2 of every
 * voxel of the volume, fully written, and work_b_dev is undefined. Host outputs of n+1 rows: max_d2 uint32 = the largest D2 of the
 * label, sum_d2 uint64 = the exact sum of D2 over its voxels, peak_index uint64 = the linear index (z*Y + y)*X + x of the voxel with
 * the largest D2, the first in C-raster order on a tie. Row 0 (the background is not measured) and a label without a voxel read 0,
 * 0 and 2^64 - 1. DLV_EINVAL before any launch for a NULL pointer, Z/Y/X < 1, a spacing outside 1..64, n >= 2^32 - 1, a pointer
 * that is not 4-byte aligned or any two of the three volumes overlapping. DLV_EUNSUP before any launch, with a message that names
 * the axis, where w_a * ceil((dim_a + 1) / 2) >= 65536 on an axis a (below that every intermediate fits uint32), and for a volume
 * above 2^32 voxels (the peak's index has 32 bits; the kernels take whole rows, so the launch grid sets no bound of its own).
 * Synchronous. */
int dlv_cc_depth_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                     uint32_t* work_a_dev, uint32_t* work_b_dev, uint32_t* max_d2, uint64_t* sum_d2, uint64_t* peak_index);
/* Fused cells split by their erosion cores (no counterpart in the reference). labels_dev: uint32 (Z,Y,X) contiguous, labels 0..n,
 * rewritten in place. (1) Cores: C_0 = labels != 0; C_{k+1}(v) = C_k(v) and C_k(u) for the 6 face neighbours u of v, a neighbour
 * outside the volume counting as background; C = C_depth. (2) The cores are labelled 1..M as dlv_ccl26_dev labels a mask; with
 * min_core > 1 the cores of fewer than min_core voxels are dropped as dlv_cc_size_filter_dev(min_size = min_core) drops them. A core
 * lies in one label; cores(l) = the number of cores in label l. (3) Growth: G_0 = the core labels; G_{k+1}(v) = G_k(v) where that is
 * not 0, else where labels(v) != 0 the smallest non-zero G_k(u) over the 26 neighbours u inside the volume with labels(u) ==
 * labels(v) (0 without one), every step from G_k alone, up to the fixed point G: a voxel goes to the core nearest to it in 26-steps
 * through its own label, to the smallest core label on a tie. (4) Pieces: key(v) = 0 where labels(v) == 0, G(v) where
 * cores(labels(v)) >= 2 and G(v) != 0, M + labels(v) otherwise (a label with fewer than two cores stays whole). The distinct keys
 * are numbered 1..K in C-raster order of their first voxel - dlv_ccl26_dev's numbering - and written to labels_dev: the foreground
 * is unchanged, K >= the number of labels present, and a volume numbered by first voxel with nothing to split comes back as it was.
 * Integer work only: exact and independent of scheduling.
 * work_a_dev, work_b_dev: two scratch volumes of Z*Y*X uint32. *n_out = K; *n_split_out = the labels with two or more cores;
 * parent_dev: parent_cap uint32 on the device, parent[j] = the old label of piece j for j = 1..K, parent[0] = 0.
 * DLV_EINVAL with labels_dev unchanged for: parent_cap < K + 1 (*n_out is set to K: call again with a larger table), a NULL
 * pointer, Z/Y/X < 1, depth outside 1..16, min_core < 1, a pointer that is not 4-byte aligned, volumes that overlap, a label above
 * n in the volume, M + n beyond the uint32 keys, or a volume beyond the launch grid (as dlv_cc_shell_dev); above 2^32 voxels
 * DLV_EUNSUP (as dlv_ccl26_dev). Synchronous. */
int dlv_cc_split_dev(dlv_ctx* ctx, uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int depth, int64_t min_core,
                     uint32_t* work_a_dev, uint32_t* work_b_dev, uint64_t* n_out, uint64_t* n_split_out,
                     uint32_t* parent_dev, uint64_t parent_cap);
/* Fused cells split by their Euclidean depth cores (no counterpart in the reference; csrc/cc_split.hip): dlv_cc_split_dev with the
 * cores taken from the exact label-wise distance map instead of voxel-counted erosions, for stacks whose voxels are not cubes - a
 * Euclidean erosion in physical units. labels_dev: uint32 (Z,Y,X) contiguous, labels 0..n, rewritten in place. PRECONDITION: no two
 * different labels are 26-adjacent - what dlv_ccl26_dev, dlv_fill_holes_dev and dlv_cc_size_filter_dev produce; only then does a core
 * lie in one label. Where it is broken the result is unspecified, but every access stays in bounds.
 * (1) The distance map: D2(v) is what dlv_cc_depth_dev defines on labels_dev with the spacings wz, wy, wx (integers 1..64);
 * m(l) = the largest D2 of label l. (2) Cores: T(l) = max(core_d2, ceil(core_pct^2 * m(l) / 10000), 1) in 64-bit integers;
 * C(v) = 1 where 1 <= labels(v) <= n and D2(v) >= T(labels(v)), else 0: every voxel at least sqrt(core_d2) spacing units, and at
 * least core_pct per cent of its cell's inscribed radius, from the outside of its cell. With core_pct > 0 every label present holds
 * at least one core, the one around its peak; with core_d2 > m(l) a label has no core and stays whole. (3), (4): the cores are
 * labelled, filtered by min_core, grown back through their own label and the pieces numbered exactly as steps (2) - (4) of
 * dlv_cc_split_dev say, by the same code: *n_out = K, *n_split_out, parent_dev and parent_cap are that entry's, labels_dev unchanged
 * and *n_out = K when the table is too small. Integer work only: exact and independent of scheduling.
 * work_a_dev, work_b_dev: two scratch volumes of Z*Y*X uint32 (D2, then the byte mask of the cores beside it: no more than
 * dlv_cc_split_dev needs). DLV_EINVAL before any launch, labels_dev unchanged, for a NULL pointer, Z/Y/X < 1, a spacing outside
 * 1..64, core_pct outside 0..99, core_d2 == 0 together with core_pct == 0, min_core < 1, a pointer that is not 4-byte aligned,
 * volumes that overlap, n >= 2^32 - 1 or a volume beyond the launch grid; DLV_EUNSUP before any launch for the reach rule of
 * dlv_cc_depth_dev (w_a * ceil((dim_a + 1) / 2) >= 65536) and above 2^32 voxels. DLV_EINVAL with labels_dev unchanged for a label
 * above n in the volume (found after the seed pass, as in dlv_cc_split_dev) and for M + n beyond the uint32 keys. Synchronous. */
int dlv_cc_split_depth_dev(dlv_ctx* ctx, uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                           uint32_t core_d2, int core_pct, int64_t min_core, uint32_t* work_a_dev, uint32_t* work_b_dev,
                           uint64_t* n_out, uint64_t* n_split_out, uint32_t* parent_dev, uint64_t parent_cap);
/* The run-length coding of a label volume and its decoder (no counterpart in the reference, which writes the dense volume; the
 * format: delivr_cfos_amd/label_runs.py). labels_dev: uint32 (Z,Y,X) contiguous, 4-byte aligned, labels below 2^32 - 1. A run is a
 * maximal stretch of one non-zero label inside a row (z, y): it never crosses a row's end, and two touching runs of different labels
 * are two runs. Runs are in raster order, so a volume has one coding.
 *  dlv_cc_runs_count_dev: row_start_dev[r] = the runs of the rows before row r = z*Y + y (uint64, Z*Y + 1 entries on the device, the
 *    last one the number of runs R), *n_runs = R on the host. Synchronous.
 *  dlv_cc_runs_emit_dev: with row_start_dev and n_runs of the count on the same labels, run k's first x, last x (inclusive, so
 *    X = 65536 fits) and label go to x0_dev[k], x1_dev[k], label_dev[k] (n_runs entries each; may be NULL with n_runs == 0).
 *    Nothing is written at or beyond n_runs. Asynchronous on the context's stream.
 *  dlv_cc_runs_decode_dev: rows [0, n_rows) of a uint32 volume of row length X from row_start_dev (n_rows + 1 entries, rebased by
 *    its first one: a range of planes is a slice of the table) and the n_runs runs those rows hold. EVERY voxel of the rows is
 *    written, zeros included; a run is clamped to its row and a run index to n_runs, whatever the arrays hold. Asynchronous on the
 *    context's stream.
 * Integer work only: exact and independent of scheduling. A NULL pointer, Z/Y/X (n_rows) < 1 or a pointer not aligned to its
 * element: DLV_EINVAL; X above 65536: DLV_EUNSUP (as dlv_cc_shape_dev); nothing is written then. */
int dlv_cc_runs_count_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t* row_start_dev, uint64_t* n_runs);
int dlv_cc_runs_emit_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, const uint64_t* row_start_dev, uint64_t n_runs,
                         uint16_t* x0_dev, uint16_t* x1_dev, uint32_t* label_dev);
int dlv_cc_runs_decode_dev(dlv_ctx* ctx, const uint64_t* row_start_dev, uint64_t n_rows, int X, const uint16_t* x0_dev,
                           const uint16_t* x1_dev, const uint32_t* label_dev, uint64_t n_runs, uint32_t* labels_out_dev);
/* Exact hole filling of a byte mask, in place (no counterpart in the reference, whose users call scipy.ndimage.binary_fill_holes
 * on the host; csrc/fill_holes.hip). mask_dev: uint8 (Z,Y,X) contiguous; the foreground is every voxel that is not 0. Two background
 * voxels are connected when they share a face (6-connectivity); the voxels outside the volume count as background and are all
 * connected to each other. A hole is a background component with no voxel on any of the six faces of the volume: every voxel of
 * every hole is written as fill_value, and no other byte of the mask is written. This is binary_fill_holes(mask != 0) with its default
 * structure. Background that reaches the rest only over an edge or a corner is sealed; a cavity open to a face of the volume is not
 * a hole; a component inside the cavity of another is swallowed by it; a hole never holds the first voxel of the component around
 * it, so dlv_ccl26_dev on the filled mask numbers the surviving components in the order they had.
 * *voxels_filled = the hole voxels, *holes = the holes (the background components filled). Integer work only: exact and independent
 * of scheduling. DLV_EINVAL with the mask untouched for a NULL pointer, Z/Y/X < 1, fill_value == 0, or a mask that already holds
 * fill_value somewhere (the caller tells filled voxels from original ones by it); DLV_EUNSUP with the mask untouched for X > 65536
 * and for more than 2^32 voxels (as the run coder and dlv_ccl26_dev). Device scratch: 8 bytes per row and 10 bytes per gap (a
 * background stretch of a row with foreground on both sides), in the context's slots. Synchronous.
 *  dlv_cc_count_marked_dev: counts_dev[l] = the voxels with label l whose mask byte equals value, for l = 0..n (device array of n+1
 *    uint32; labels_dev: nvox uint32, 4-byte aligned; mask_dev: nvox bytes; labels above n are not counted, as in
 *    dlv_cc_counts_dev). On the labels of a filled mask with value = fill_value: the voxels the fill gave each component.
 *    n >= 2^32 - 1, a NULL or a misaligned pointer: DLV_EINVAL. Asynchronous on the context's stream. */
int dlv_fill_holes_u8_dev(dlv_ctx* ctx, uint8_t* mask_dev, int Z, int Y, int X, uint8_t fill_value, uint64_t* voxels_filled,
                          uint64_t* holes);
int dlv_cc_count_marked_dev(dlv_ctx* ctx, const uint32_t* labels_dev, const uint8_t* mask_dev, uint64_t nvox, uint64_t n, uint8_t value,
                            uint32_t* counts_dev);
/* The overlap table of two label volumes (no counterpart in the reference; csrc/cc_overlap.hip, delivr_cfos_amd/compare_cells.py): every
 * pair of labels (a, b) that share voxels, with the number of voxels they share. a_dev, b_dev: uint32 (Z,Y,X) contiguous, 4-byte
 * aligned, labels below 2^32 - 1. A voxel takes part when 1 <= a <= n_a and 1 <= b <= n_b: the background and labels above n in either
 * volume contribute nothing. The key of a pair is (a << 32) | b. A pair segment is a maximal stretch of one key inside a row (z, y).
 *  dlv_cc_overlap_count_dev: *n_segments = the pair segments S of the volumes, on the host. The distinct pairs P are at most
 *    min(S, n_a * n_b). Synchronous.
 *  dlv_cc_overlap_dev: with the S of the count on the same volumes, the P distinct keys go to keys_out_dev[0..P) and their voxels to
 *    voxels_out_dev[0..P) (uint64 each, out_cap >= min(S, n_a * n_b) entries, 8-byte aligned), *n_pairs = P on the host. table_dev: the
 *    caller's scratch of cap slots of 16 bytes (2 * cap uint64, 16-byte aligned), cap a power of two >= 2 * min(S, n_a * n_b); the call
 *    clears it. The order of the pairs on the device is unspecified (HipEngine.cc_overlap sorts by key on the host); the pairs and their
 *    voxels are exact and independent of scheduling: integer work only. With S = 0 nothing is launched and P = 0. Synchronous.
 * DLV_EINVAL, checked on the host before anything is launched and with nothing written: a NULL pointer, a misaligned pointer,
 * Z/Y/X < 1, n_a or n_b above 2^32 - 2, cap not a power of two or below 2 * min(S, n_a * n_b), out_cap below min(S, n_a * n_b). X above
 * 2^30: DLV_EUNSUP. DLV_ESTATE with a message that names the table: a key found no slot, or more pairs than out_cap - the kernels bound
 * every probe by cap and every write by out_cap, and neither happens when S is the count of these volumes. */
int dlv_cc_overlap_count_dev(dlv_ctx* ctx, const uint32_t* a_dev, const uint32_t* b_dev, int Z, int Y, int X, uint64_t n_a, uint64_t n_b,
                             uint64_t* n_segments);
int dlv_cc_overlap_dev(dlv_ctx* ctx, const uint32_t* a_dev, const uint32_t* b_dev, int Z, int Y, int X, uint64_t n_a, uint64_t n_b,
                       uint64_t n_segments, uint64_t* table_dev, uint64_t cap, uint64_t* keys_out_dev, uint64_t* voxels_out_dev,
                       uint64_t out_cap, uint64_t* n_pairs);
/* The neighbour table of a label volume (no counterpart in the reference; csrc/cc_neighbours.hip, count_blobs' neighbour_stats): every
 * pair of labels a < b whose cells come within a radius of each other, with the exact smallest squared distance between them.
 * labels_dev: uint32 (Z,Y,X) contiguous, 4-byte aligned, not written. A voxel takes part when 1 <= L(v) <= n: the background and
 * labels above n contribute nothing and block nothing. wz, wy, wx: the voxel spacings, integers 1..64 (as dlv_cc_depth_dev);
 * r2 >= 1: the squared radius in spacing units. gap2(a, b) = the minimum over the voxels v of a and u of b of
 * (wz (vz - uz))^2 + (wy (vy - uy))^2 + (wx (vx - ux))^2, at least 1; the table is every a < b with gap2(a, b) <= r2, under the key
 * (a << 32) | b. The reach along axis a is floor(sqrt(r2) / w_a) voxels; this version supports a reach of at most 8 on every axis
 * (0 is legal: no offsets along that axis). A segment is one flush of a thread's carry (one pair, its smallest distance so far)
 * in the scan of the surface voxels; both entries make the same scan.
 *  dlv_cc_neighbours_count_dev: *n_segments = the segments S of the volume, on the host. The pairs P are at most
 *    min(S, n (n - 1) / 2). Synchronous.
 *  dlv_cc_neighbours_dev: with the S of the count on the same volume and arguments, the P keys go to keys_out_dev[0..P) (uint64,
 *    8-byte aligned) and their gap2 to gap2_out_dev[0..P) (uint32, 4-byte aligned), out_cap >= min(S, n (n - 1) / 2) entries each,
 *    *n_pairs = P on the host. table_dev: the caller's scratch of cap slots of 16 bytes (2 * cap uint64, 16-byte aligned), cap a
 *    power of two >= 2 * min(S, n (n - 1) / 2); the call clears it. The order of the pairs on the device is unspecified
 *    (HipEngine.cc_neighbours sorts by key on the host); the pairs and their gaps are exact and independent of scheduling: integer
 *    work only. With S = 0 nothing is launched and P = 0. Synchronous.
 * DLV_EINVAL, checked on the host before anything is launched and with nothing written: a NULL pointer, a misaligned pointer,
 * Z/Y/X < 1, a spacing outside 1..64, r2 < 1, n above 2^32 - 2, cap not a power of two or below 2 * min(S, n (n - 1) / 2), out_cap
 * below min(S, n (n - 1) / 2), a volume beyond the launch grid (more than 65535 tiles of 8 planes or of 8 rows). DLV_EUNSUP, checked
 * in the same place, with a message that names the axis, its reach and the limit: a reach above 8; and X above 2^30. DLV_ESTATE with a
 * message that names the table: a key found no slot, or more pairs than out_cap - the kernels bound every probe by cap and every
 * write by out_cap, and neither happens when S is the count of this volume. */
int dlv_cc_neighbours_count_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx,
                                uint64_t r2, uint64_t* n_segments);
int dlv_cc_neighbours_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n, int wz, int wy, int wx, uint64_t r2,
                          uint64_t n_segments, uint64_t* table_dev, uint64_t cap, uint64_t* keys_out_dev, uint32_t* gap2_out_dev,
                          uint64_t out_cap, uint64_t* n_pairs);

/* ---- TIFF z-plane ingest -------------------------------------------------------- */
/* Replaces the per-plane cv2.imread / skimage.io / tifffile reads of the raw stack
 * (downsample/downsample_and_mask.py:25-30, :36-41, :396-404).  Classic TIFF and BigTIFF, II/MM, strips or tiles, 8/16-bit
 * unsigned single channel, compression 1 (none), 5 (LZW) or 8 / 32946 (deflate), predictor 1 or 2; anything else (JPEG,
 * float or multi-sample planes, ...) is refused with DLV_EUNSUP.
 *  dlv_tiff_plane_size / dlv_tiff_read_plane_u16: host-only (no context, no GPU): header fields / one decoded plane
 *    (8-bit samples widened) into a caller-owned (height,width) uint16 host array; dlv_tiff_last_error() holds the
 *    message of the calling thread's last failure.
 *  dlv_tiff_stack_to_device: planes paths[0..n_planes) are decoded by n_threads host threads (0 = one per core, at
 *    most 32) into pinned staging buffers and copied to vol_dev[(i*plane_stride) + y*row_stride + x] (uint16 elements;
 *    strides let the caller fill the zero-padded (Zp,Yp,Xp) network input directly) while the next chunk is being
 *    decoded.  Synchronous. */
const char* dlv_tiff_last_error(void);
int dlv_tiff_plane_size(const char* path, int* height, int* width, int* bits);
int dlv_tiff_read_plane_u16(const char* path, uint16_t* out_host, int height, int width);
/* egress: one (height,width) plane of 8- or 16-bit samples (host, native little-endian) as a classic TIFF with
 * ~64 KB strips, compression 1 (none) or 5 (LZW) - the plane files of blob_highlighter.py:131-133, :160 and
 * cells_to_atlas.py:320 (tifffile.imwrite(..., compression='lzw')).  Host-only. */
int dlv_tiff_write_plane(const char* path, const void* data_host, int height, int width, int bits, int compression);
int dlv_tiff_stack_to_device(dlv_ctx* ctx, const char* const* paths, int n_planes, int height, int width, uint16_t* vol_dev,
                             long long plane_stride, long long row_stride, int n_threads);

/* ---- blob painting (visualisation step) ------------------------------------------ */
/* The colouring loops of blob_highlighter.py:108-125 (RGB) and :150-158 (region id): cells are visited in CSV order
 * and IMG[box] = bin_img[box] * value is assigned over each cell's padded bounding box, so the last listed box that
 * contains a voxel wins.  dlv_paint_owner_dev computes that winner for every voxel: owner (Z,Y,X) uint32 = 1 + index
 * of the last box containing the voxel, 0 = none / background.  boxes (n,6) int32 = z0,z1,y0,y1,x0,x1 HALF-OPEN, i.e.
 * exactly the slices the reference takes after pad_bb (blob_highlighter.py:18-23); the same list is passed on the host
 * (bounds check, launch plan) and in HBM.  dlv_paint_apply_dev: out[v] = bin[v] * values[owner[v]-1] (0 where owner is
 * 0) in uint8 (elem_bytes 1: the R/G/B images) or uint16 (elem_bytes 2: region ids), numpy's wrap-around included. */
int dlv_paint_owner_dev(dlv_ctx* ctx, const uint8_t* bin_dev, int Z, int Y, int X, const int32_t* boxes_dev,
                        const int32_t* boxes_host, uint64_t n_boxes, uint32_t* owner_dev);
int dlv_paint_apply_dev(dlv_ctx* ctx, const uint32_t* owner_dev, const uint8_t* bin_dev, uint64_t nvox,
                        const void* values_dev, int elem_bytes, void* out_dev);
/* Painting from the labels (csrc/cc_paint.hip; blob_highlighter with settings["mi355x"]["paint_from"] = "labels"). Replaces the same
 * two loops, with their stated intent in place of their boxes: every voxel gets the value of the cell whose label it carries,
 * out[v] = lut[label[v]], and 0 elsewhere - no box, no padding, no "might accidentally re-color other blobs close by". The look-up
 * tables are indexed by label, n_lut entries each, entry 0 the background: lut_rgb_dev uint32 = r | g << 8 | b << 16 with the three
 * uint8 planes out_r / out_g / out_b (all three or none), lut_u16_dev uint16 with the plane out_u16; either pair may be NULL, and
 * one pass over the labels or the runs writes every plane asked for. A label of 0 writes 0 and so does a label >= n_lut: the
 * kernels clamp, they do not judge.
 *  dlv_paint_labels_dev: the labels are the dense uint32 volume (Z,Y,X), contiguous.
 *  dlv_paint_runs_dev: the labels are the run-length coding of dlv_cc_runs_emit_dev, addressed as dlv_cc_runs_decode_dev addresses
 *    it: rows [0, n_rows) of row length X, row_start_dev (n_rows + 1 entries) rebased by its first one, run indices clamped to n_runs
 *    (x0 / x1 / label may be NULL with n_runs == 0), a run clamped to its row. The label volume is never built.
 * Every element of every output row is written exactly once, zeros included: the planes need not be cleared. Integer work only,
 * one writer per element, no atomics: exact. DLV_EINVAL, with nothing written, for: neither table; a table without its planes or
 * planes without their table (the three byte planes count as one); a pointer not aligned to its element; a NULL ctx / labels /
 * row_start, an empty volume or n_lut < 1. X above 65536 in dlv_paint_runs_dev: DLV_EUNSUP. Asynchronous on the context's stream. */
int dlv_paint_labels_dev(dlv_ctx* ctx, const uint32_t* labels_dev, int Z, int Y, int X, uint64_t n_lut, const uint32_t* lut_rgb_dev,
                         const uint16_t* lut_u16_dev, uint8_t* out_r, uint8_t* out_g, uint8_t* out_b, uint16_t* out_u16);
int dlv_paint_runs_dev(dlv_ctx* ctx, const uint64_t* row_start_dev, uint64_t n_rows, int X, const uint16_t* x0_dev,
                       const uint16_t* x1_dev, const uint32_t* label_dev, uint64_t n_runs, uint64_t n_lut, const uint32_t* lut_rgb_dev,
                       const uint16_t* lut_u16_dev, uint8_t* out_r, uint8_t* out_g, uint8_t* out_b, uint16_t* out_u16);

/* Depth-coded blob map (blob_depthmap.py:160-170): scipy.ndimage.distance_transform_edt(np.pad(stack, 1), sampling)
 * [1:-1,1:-1,1:-1].astype(np.uint16) of the down-sampled masked stack - the distance (in the units of `sampling_zyx`, 3
 * doubles on the host) of every non-zero voxel to the nearest zero voxel, the stack being surrounded by zeros; exact
 * (separable lower-envelope algorithm in fp64), truncated to uint16 like numpy's astype.  The painting itself
 * (blob_depthmap.py:186-198: IMG[box] = bin_img[box] * depth_of_the_cell) is dlv_paint_owner_dev + dlv_paint_apply_dev. */
int dlv_edt_u16_dev(dlv_ctx* ctx, const uint16_t* in_dev, int Z, int Y, int X, const double* sampling_zyx, uint16_t* out_dev);


/* ---- cell-density heat map in atlas space (region assignment step) --------------- */
/* create_heatmap (cells_to_atlas.py:174-200): heat (Z,Y,X) float32 = number of cells per atlas voxel (cells (n,3) int32
 * = x,y,z as in the reference's columns; cells outside the grid are ignored - the reference drops them before, :139-144),
 * then scipy.ndimage.gaussian_filter(heat, sigma) = dlv_gauss_blur_f32_dev with the host-computed half kernel
 * weights[0..radius] (weights[0] = centre; scipy: radius = int(4*sigma + 0.5), phi / phi.sum()), boundary 'reflect',
 * float32 between the axis passes, in place (tmp_dev: scratch of the same size).  Bit-identical to scipy. */
int dlv_heatmap_counts_dev(dlv_ctx* ctx, const int32_t* xyz_dev, uint64_t n_cells, int Z, int Y, int X, float* heat_dev);
int dlv_gauss_blur_f32_dev(dlv_ctx* ctx, float* vol_dev, int Z, int Y, int X, const double* weights_host, int radius,
                           float* tmp_dev);

/* ---- resamplers (the steps either side of the path) ----------------------------------------- */
/* transform.downscale_local_mean(chunk,(fz,fy,fx)).astype(uint16) (downsample_and_mask.py:44):
 * out (ceil(Z/fz),ceil(Y/fy),ceil(X/fx)) = floor(sum over zero-padded block / (fz*fy*fx)). */
int dlv_block_mean_u16_dev(dlv_ctx* ctx, const uint16_t* in_dev, int Z, int Y, int X, int fz, int fy, int fx,
                           uint16_t* out_dev);
/* scipy.ndimage.zoom(mask, out/in, output=uint8, order=2, prefilter=False)
 * (downsample_and_mask.py:299). */
int dlv_zoom_spline2_u8_dev(dlv_ctx* ctx, const uint8_t* in_dev, int iz, int iy, int ix, uint8_t* out_dev,
                            int oz, int oy, int ox);
/* img *= mask_us[i]; masked_nii[0,0,i,:Y,:X] = img (downsample_and_mask.py:396-417): writes the
 * zero-padded (Zp,Yp,Xp) uint16 volume from raw (Z,Y,X) uint16 and mask (Z,Y,X) uint8 (nullable:
 * threshold mode, values < threshold -> 0). */
int dlv_mask_pad_u16_dev(dlv_ctx* ctx, const uint16_t* raw_dev, const uint8_t* mask_dev, int threshold, int Z,
                         int Y, int X, uint16_t* out_dev, int Zp, int Yp, int Xp);
/* north-star extension (no reference counterpart): trilinear resample, align_corners=False,
 * clamp-to-edge, uint16 -> uint16 (round half up). */
int dlv_trilinear_u16_dev(dlv_ctx* ctx, const uint16_t* in_dev, int iz, int iy, int ix, uint16_t* out_dev,
                          int oz, int oy, int ox);
/* north-star extension "affine atlas-space warp" (BASELINE config 5).  The reference has no volume warp: it registers with
 * the external mBrainAligner binaries and moves cell COORDINATES (automate_mBrainaligner.py:21-72, :292-435).
 * out[z,y,x] = trilinear sample of `in` at the index-space point matrix34 . (z,y,x,1) (row-major 3x4, host pointer: maps
 * OUTPUT voxel indices to INPUT voxel indices), zero outside the input, round half up.  fp64 arithmetic, bit-exact
 * against oracle.affine_warp_u16.  hostlogic.affine_apply maps cell coordinates found in the warped volume back. */
int dlv_affine_warp_u16_dev(dlv_ctx* ctx, const uint16_t* in_dev, int iz, int iy, int ix, const double* matrix34,
                            uint16_t* out_dev, int oz, int oy, int ox);

/* ---- in-library kernel timing (bench.py's roofline leg) ------------------------------------- */
#define DLV_PROF_MAX_KERNELS 64
typedef struct dlv_prof_entry {
    char name[48];
    int64_t launches;
    double total_ms;     /* sum of HIP-event durations on the ctx stream */
    double flops;        /* algorithmic FLOPs summed over those launches */
    double bytes;        /* algorithmic HBM bytes summed over those launches */
} dlv_prof_entry;
/* fp16 range guard, the remedy.  fp16 ends at 65504; a checkpoint whose RAW (pre-normalisation) output of conv block `layer`
 * exceeds it makes dlv_sw_infer_dev / dlv_unet_forward_dev return DLV_ERANGE.  Every 3x3x3 conv of the network is followed by
 * InstanceNorm, which is invariant to a scale of its input: dlv_unet_set_conv_shift(ctx, layer, k) packs that block's 16-bit
 * weights (and bias) multiplied by 2^-k (exact) and normalises with eps * 4^-k - the stored raw tensor is 2^k times smaller, the
 * normalised value the same, the format stays fp16 (11 significant bits; bf16, the other way out, has 8).  The fp32 path is
 * not affected.  Shifts are reset by dlv_unet_load / dlv_unet_alloc_blob; a rank that received its weights by broadcast sets
 * the same shifts itself.  dlv_range_report: the layer the last DLV_ERANGE named (-1: none; 18: the logits) - its INPUT
 * overflowed, i.e. the block(s) feeding it - and per conv block the largest |mean| + 8 sigma of its raw output (in stored
 * units; 0: the block did not run) seen since the last pass started: above 4096 it is the hint for k, and it tells which blocks
 * are too small to be moved at all.  inference/inference.py's
 * run_inference applies both before it falls back to bf16.  No reference counterpart (the reference network is fp32:
 * inference/sliding_window_inferer.py:205-229). */
int dlv_unet_set_conv_shift(dlv_ctx* ctx, int layer, int shift);
int dlv_unet_get_conv_shift(dlv_ctx* ctx, int layer, int* shift);
int dlv_range_report(dlv_ctx* ctx, int* layer, float* peaks /* [DLV_N_CONV] or NULL */);
/* The policy between the two, for hosts that do not go through run_inference (same rules as delivr_cfos_amd/range_guard.py; a CPU
 * test compares them).  dlv_range_next_shifts is pure host logic: given the layer and peaks of dlv_range_report and the current
 * shifts it writes the next shifts to out[DLV_N_CONV] and returns how many blocks changed (0: nothing left to try; -1: null
 * argument) - the blocks feeding `layer` (MONAI BasicUNet's wiring, inference/inference.py:190-197) move so that |mean| + 8 sigma
 * of their stored output falls to <= 1024, or by 6 bits where no block reported a peak above 4096 (never a block whose peak would
 * fall below 1).  dlv_range_recover applies it to one context after a DLV_ERANGE: DLV_OK = shifts changed (committed only after
 * the weights were re-packed; the report is cleared), repeat the passes (zero the accumulators first); DLV_ERANGE = nothing left,
 * or a 6-bit step on no evidence did not move the overflow - the shifts are back where the sequence started (the caller's last
 * resort is DLV_PREC_BF16_ALL); run_inference gives up after four steps.  dlv_comm_range_recover does the
 * same for every rank of a dlv_comm with the largest layer / peaks any rank saw, so all ranks keep the same shifts. */
int dlv_range_next_shifts(int layer, const float* peaks, const int* shifts, int* out /* [DLV_N_CONV] each */);
int dlv_range_recover(dlv_ctx* ctx, int* n_changed /* or NULL */);
/* The blob this context RECEIVED (dlv_unet_alloc_blob + a broadcast into dlv_unet_blob_dev) holds 16-bit packs made with these
 * shifts: record them - the InstanceNorm eps of a shifted block scales with 4^-shift - without packing again.  dlv_bcast_weights
 * does it for the ranks of a dlv_comm; parallel.broadcast_weights for the ranks of a torch.distributed job. */
int dlv_unet_note_conv_shifts(dlv_ctx* ctx, const int* shifts /* [DLV_N_CONV] */);
/* 1 = run batches back to back on the ctx stream; 2 .. 6 (default 3) = rotate consecutive batches over that many HIP
 * streams so that HBM-bound and MFMA-bound kernels of neighbouring batches overlap (results are identical). */
int dlv_set_lanes(dlv_ctx* ctx, int lanes);
int dlv_prof_enable(dlv_ctx* ctx, int on); /* on: bracket each kernel launch with hipEvents */
int dlv_prof_reset(dlv_ctx* ctx);
int dlv_prof_report(dlv_ctx* ctx, dlv_prof_entry* entries, int capacity, int* n_out); /* synchronous */

/* Allocates now what a pass with these parameters (window shape, precision, batch; dlv_set_lanes) and the finalize of a Z x Y x X
 * stack (0s: none) will ask for later - ~10 GB of activations per pipeline lane, the erosion's distance map.  Fresh device memory
 * is free to allocate, memory that went back to the driver is not (up to seconds for tens of GB in a long-lived process:
 * profiles/r06r_alloc_probe2.json): a host calls this from a second thread while it reads the volume (inference/inference.py
 * does), and keeps one context per device for all its volumes so that nothing is released in between.  Optional: the pass
 * allocates on demand otherwise.  The ctx must not be used by another thread meanwhile.  No reference counterpart (PyTorch's
 * caching allocator plays this role there, inference/inference.py:240-247). */
int dlv_reserve_dev(dlv_ctx* ctx, const dlv_sw_params* p, int Z, int Y, int X);

/* Test hooks and A/B switches (dlv_debug_*, dlv_diag_set) are declared in delivr_hip_diag.h: they are not part of the drop-in
 * boundary.  The library reads these environment variables and no others: DLV_LANES (default of dlv_set_lanes), DLV_LAUNCH_LOG
 * (file that receives one line per kernel launch: profiles/make_traffic.py), and for the transport of dlv_comm_init_all
 * DLV_RCCL_PATH / ROCM_PATH (where librccl.so is looked for) and DLV_FORCE_RCCL (RCCL also for a one-rank communicator). */

#ifdef __cplusplus
}
#endif
#endif /* DELIVR_HIP_H */
