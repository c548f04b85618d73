/*
 * adapted_hip.h -- C ABI of libadapted_hip.so: the MI355X (gfx950) implementation of the
 * `adapted detect` signal-segmentation hot path.
 *
 * Drop-in boundary.  The reference (KleistLab/ADAPTed v0.2.4) exposes this path as Python
 * operators over one dense minibatch; each entry point below replaces one of them
 * (file:line under the reference tree):
 *
 *   adp_detect_llr          <- combined_detect_llr2(batch f32[N,m], full_lens i32[N], spc)
 *                              adapted/detect/combined.py:122-227   (called from
 *                              adapted/file_proc.py:230-235), which itself wraps the only
 *                              native code of the reference, adapted/detect/_c_llr.pyx:
 *                              c_llr_trace :202-236, c_llr_trace_gains :176-199, _gains :67-88
 *   adp_detect_start_peak   <- combined_detect_start_peak(...)   adapted/detect/combined.py:312-355
 *                              (detect_rna_start_peak, adapted/detect/start_peak.py:7-119)
 *   adp_detect_cnn          <- combined_detect_cnn(...)          adapted/detect/combined.py:230-309 (with ADP_CNN_FALLBACK; without
 *                              the flag up to its short-read fallback :251-301, which callers then apply themselves with
 *                              adp_llr_refine_polya + adp_validate_candidates)
 *   adp_cnn_prepare         <- prepare_data(...)                 adapted/detect/cnn.py:70-82
 *   adp_cnn_forward         <- BoundariesCNN.forward / cnn_score adapted/detect/cnn.py:16-52, 85-98 (hand-written conv
 *                              stack; default: float16 matrix cores on split float32 operands at float32 accuracy,
 *                              adapted_amd/csrc/cnn_conv_split.h, with the exact float32 MFMA kernels of cnn_conv.h behind
 *                              it for activations outside the float16 range -- or for every call when the handle was
 *                              created with ADP_CNN_CONV=f32 in the environment; PyTorch is not involved)
 *   adp_cnn_predict         <- cnn_predict + cnn_detect scaling  adapted/detect/cnn.py:101-182
 *   adp_validate_candidates <- the validate_boundaries loop of combined_detect_cnn
 *                              adapted/detect/combined.py:243-305
 *   adp_cfg                 <- SigProcConfig                     adapted/config/sig_proc.py:161-221
 *   adp_row                 <- DetectResults                     adapted/container_types.py:23-92
 *
 * Conventions: plain C, caller-allocated outputs, no exceptions.  Every function returns 0
 * or a negative ADP_ERR_* code.  A handle owns one device, its HIP streams and its workspace
 * (allocated by the first call that needs it, for the reads of that call, and kept: a call may
 * therefore return ADP_ERR_HIP for an allocation that adp_create did not attempt); it is not
 * thread-safe, distinct handles are independent.  Every call returns with its work finished.  `signals` is the reference's
 * minibatch layout (adapted/file_proc.py:143-190): row-major float32 [n_reads, m], NaN from
 * each read's end to m; full_len[i] is the read's true length (may exceed m).  A call may
 * carry several minibatches: reads [k*minibatch, (k+1)*minibatch) form minibatch k, and the
 * LLR path normalises with ONE median/MAD per minibatch exactly as the reference does
 * (adapted/detect/normalize.py:15-22 on the 2-D array).
 */
#ifndef ADAPTED_HIP_H
#define ADAPTED_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADP_ABI_VERSION 3

/* error codes */
#define ADP_OK 0
#define ADP_ERR_INVALID (-1)       /* bad argument */
#define ADP_ERR_HIP (-2)           /* a HIP runtime call failed (see adp_last_error) */
#define ADP_ERR_CAPACITY (-3)      /* n_reads / m exceed what the handle was created for */
#define ADP_ERR_UNSUPPORTED (-4)   /* config outside the implemented surface */
/* per-minibatch status (mb_status[]): the reference raises and drops the minibatch */
#define ADP_MB_OK 0
#define ADP_MB_MAD_ZERO 1          /* "MAD normalization failed: scale is 0" normalize.py:56-59 */
#define ADP_MB_EMPTY_TRACE 2       /* a read has no valid pooled block: np.argmin of an empty
                                      trace, adapted/detect/llr.py:136 */

/* memory-kind flags */
#define ADP_IN_DEVICE 1            /* signals / full_len are device pointers */
#define ADP_OUT_DEVICE 2           /* rows_out is a device pointer */
#define ADP_WITH_START_PEAK 4      /* adp_detect_llr / adp_detect_cnn: also fill the start_peak_* columns (extension) */
#define ADP_TOPK_NONE 8            /* adp_validate_candidates: polya_end_topk is None (k must be 1) */
#define ADP_BOUNDS_HOST 16         /* adp_validate_candidates: `bounds` is host memory even though ADP_IN_DEVICE is set */
#define ADP_TAILS_NAN 32           /* adp_detect_llr: the caller guarantees that row r is NaN from min(full_len[r], m) on (the
                                      padding of adapted/file_proc.py:170-174): the streaming passes then stop at the read's
                                      end instead of reading the padding.  Without the flag the rows are taken as they are. */
#define ADP_CNN_FALLBACK (1 << 17)  /* adp_detect_cnn: apply the short-read LLR fallback (adapted/detect/combined.py:251-301) inside the
                                      call, where cfg.fallback_to_llr_short_reads is set: the rows are combined_detect_cnn's */
#define ADP_CNN_SECOND_LLR (1 << 18) /* adp_detect_cnn: a read whose row fails gets the row of combined_detect_llr2 on its minibatch, if
                                      that row passes (an extension; adp_row.reserved_ bit 0 marks such a row) */
#define ADP_FLAG_TRUNCATED (1 << 19) /* adp_detect_llr / adp_detect_cnn: flag poly(A) tails cut off by the preload window (an extension,
                                      see adp_detect_llr; adp_row.reserved_ bits 1 and 2) */
#define ADP_POLYA_TRUNCATED (1 << 20) /* adp_validate_candidates: Boundaries.polya_truncated is True for every read -- the RNA partition
                                      is all None (adapted/partition/signal_partitions.py:74-77) */
/* (1 << 21 is ADP_LLR_RESEGMENT, a flag of adp_detect_llr with a header of its own: adapted_hip_resegment.h, included below;
 * 1 << 22 is ADP_KNN_NO_PRUNE of adapted_hip_knn.h; 1 << 23 is ADP_CNN_SECOND_RESEGMENT, a flag of adp_detect_cnn(_i16):
 * adapted_hip_second_resegment.h; 1 << 24 is ADP_PACKED_I16 of adapted_hip_events_packed.h) */

/* SigProcConfig, flattened.  Ranges are [lo, hi] with -inf/+inf for "None". */
typedef struct adp_cfg {
    int32_t min_obs_adapter, max_obs_adapter, min_obs_polya, downscale_factor, max_obs_trace;
    int32_t primary_method;            /* 0 llr, 1 cnn, 2 start_peak: names the *_adapter_end columns */
    double sig_norm_outlier_thresh;
    double adapter_peak_prominence, adapter_peak_rel_height;
    int32_t adapter_peak_width;
    int32_t mvs_detect_check, mvs_detect_overwrite, search_window;
    int32_t pA_mean_window, pA_var_window, median_shift_window, polyA_window;
    double pA_mean_range[2], pA_var_range[2], median_shift_range[2];
    double polyA_med_range[2], polyA_local_range[2], pA_mean_adapter_med_scale_range[2];
    int32_t detect_open_pores, real_signal_check, mean_window, max_obs_local_range;
    double mean_start_range[2], mean_end_range[2], local_range[2], adapter_mad_range[2];
    int32_t detect_med_shift, med_shift_window;
    double med_shift_range[2];
    int32_t sp_downscale_factor, start_peak_max_idx, sp_offset1, sp_offset2;
    double open_pore_pa;
    int32_t polya_cand_k, fallback_to_llr_short_reads;
} adp_cfg;

/* numeric columns of a result row, in DetectResults field order */
enum adp_col {
    ADP_C_SIGNAL_LEN, ADP_C_PRELOADED,
    ADP_C_ADAPTER_START, ADP_C_ADAPTER_END, ADP_C_ADAPTER_LEN, ADP_C_ADAPTER_MEAN, ADP_C_ADAPTER_STD,
    ADP_C_ADAPTER_MED, ADP_C_ADAPTER_MAD,
    ADP_C_POLYA_START, ADP_C_POLYA_END, ADP_C_POLYA_LEN, ADP_C_POLYA_MEAN, ADP_C_POLYA_STD,
    ADP_C_POLYA_MED, ADP_C_POLYA_MAD,
    ADP_C_RNA_START, ADP_C_RNA_LEN, ADP_C_RNA_MEAN, ADP_C_RNA_STD, ADP_C_RNA_MED, ADP_C_RNA_MAD,
    ADP_C_SP_IDX, ADP_C_SP_PA, ADP_C_SP_NEXT_IDX, ADP_C_SP_NEXT_PA, ADP_C_SP_OPEN_PORE_IDX,
    ADP_C_MED_SHIFT, ADP_C_PRIMARY_ADAPTER_END, ADP_C_PRIMARY_POLYA_END,
    ADP_C_MVS_MEAN, ADP_C_MVS_VAR, ADP_C_MVS_POLYA_MED, ADP_C_MVS_LOCAL_RANGE, ADP_C_MVS_MED_SHIFT,
    ADP_C_REAL_MEAN_START, ADP_C_REAL_MEAN_END, ADP_C_REAL_LOCAL_RANGE,
    ADP_C_MVS_ADAPTER_END,             /* mvs_detect_overwrite: position found by the MVS scan, 0 if none (combined.py:523) */
    ADP_NCOL
};

/* fail codes <-> the reference's fail_reason strings (adapted/detect/combined.py:396-580) */
enum adp_fail {
    ADP_F_NONE = 0,
    ADP_F_NO_ADAPTER = 1,       /* "No adapter detected (primary)" */
    ADP_F_ADAPTER_MAD = 2,      /* "adapter MAD check failed" */
    ADP_F_OPEN_PORE = 3,        /* "Open pore too close to boundary" */
    ADP_F_REAL_RANGE = 4,       /* "Real signal check failed" */
    ADP_F_NO_POLYA = 5,         /* "No polya detected (primary)" */
    ADP_F_MVS_NOT_ENOUGH = 6,   /* "MVS polya check failed: not enough signal" */
    ADP_F_MVS_CHECKS = 7,       /* "MVS polya check failed: " + names from mvs_fail_mask */
    ADP_F_MED_SHIFT = 8,        /* "Median shift check failed" */
    /* 9..14: the reference raised inside the per-read try block; the row is all-None */
    ADP_F_EXC_TOPK_NONE = 9,    /* "'NoneType' object is not iterable" (combined.py:464) */
    ADP_F_EXC_SLICE = 10,       /* "slice indices must be integers or None or have an __index__ method" */
    ADP_F_EXC_MOVE_WINDOW = 11, /* bottleneck: moving window larger than the slice */
    ADP_F_EXC_PA_RANGE = 12,    /* "pA_mean_range is not specified" (combined.py:462) */
    ADP_F_EXC_EMPTY_TRACE = 13, /* "attempt to get argmin of an empty sequence" (CNN fallback, llr.py:136) */
    ADP_F_EXC_MAD_ZERO = 14,    /* "MAD normalization failed: scale is 0" (CNN fallback, normalize.py:56-59) */
    ADP_F_NO_ADAPTER_MVS = 15   /* "No adapter detected in range (mvs_detect)" (mvs_detect_overwrite, combined.py:540) */
};
#define ADP_F_IS_EXCEPTION(code) ((code) >= 9 && (code) <= 14)
/* adp_row.mvs_fail_mask bit 8: mvs_llr_polya_end_to_early_stop (mvs_detect_overwrite moved the adapter end past the
 * poly(A) end; the reference then takes Boundaries.trace_early_stop_pos, None on every v0.2.4 path: polya_end is None) */
#define ADP_MVS_TO_EARLY_STOP 256

#define ADP_MAX_CAND 16
#define ADP_MAX_OPEN_PORES 16

/* one read's result: fixed width so that rows can be gathered across GPUs as bytes */
typedef struct adp_row {
    double col[ADP_NCOL];      /* ints exactly, float32 statistics widened exactly */
    uint64_t present;          /* bit c set <=> col[c] is not None */
    int32_t success;
    int32_t fail_code;         /* enum adp_fail */
    int32_t mvs_fail_mask;     /* bit0 mean, bit1 var, bit2 med, bit3 range, bit4 shift failed; bit8 ADP_MVS_TO_EARLY_STOP */
    int32_t start_peak_type;   /* 0 None, 1 "open pore in adapter", 2 "potential concatemer adapter-only read" */
    int32_t n_cand;            /* polya_candidates length; -1 <=> None */
    int32_t n_open_pores;      /* open_pores length (may exceed ADP_MAX_OPEN_PORES: see open_pores_more); -1 <=> None */
    int64_t cand[ADP_MAX_CAND];
    int32_t open_pores[ADP_MAX_OPEN_PORES]; /* the first ADP_MAX_OPEN_PORES positions */
    int32_t open_pores_more;   /* n_open_pores > ADP_MAX_OPEN_PORES: the WHOLE list lies at this offset of the call's
                                  open-pore arena (adp_open_pores_arena); -1 otherwise */
    int32_t reserved_;         /* ADP_ROW_* bits.  bit 0: the row was made by the LLR second opinion of adp_detect_cnn
                                  (ADP_CNN_SECOND_LLR): its primary columns are the LLR's.  bit 1: the poly(A) runs into the end of the
                                  preloaded window (ADP_FLAG_TRUNCATED): polya_end is the window's end, the RNA partition all None.
                                  bit 2: the call looked for that (set in EVERY row of a call made with ADP_FLAG_TRUNCATED, so that a
                                  row says by itself whether "not truncated" was decided or never asked).  bit 3: adp_adapter_front moved
                                  the row's adapter_start (adapted_hip_adapter_front.h): adapter_start, adapter_len and the four adapter
                                  statistics are the trimmed adapter's, everything else the first validation's.  bit 4 (beside bit 3):
                                  adp_adapter_front_revalidate replaced the row by the validation from the trimmed start
                                  (adapted_hip_revalidate.h).  bit 5: the row is the validation of the second segmentation of
                                  ADP_LLR_RESEGMENT, bits 6-9 the fail_code of the row it replaced (adapted_hip_resegment.h).  0 in
                                  every other row */
} adp_row;
#define ADP_ROW_FROM_SECOND_LLR 1
#define ADP_ROW_POLYA_TRUNCATED 2
#define ADP_ROW_TRUNC_LOOKED 4
#define ADP_ROW_ADAPTER_FRONT 8

typedef struct adp_handle adp_handle;

int adp_abi_version(void);
int adp_sizeof_cfg(void);
int adp_sizeof_row(void);
const char *adp_last_error(void);

/* Number of visible HIP devices, or a negative error. */
int adp_device_count(void);

/* Create a handle on `device` able to process up to max_reads reads of m samples per call. */
int adp_create(int device, const adp_cfg *cfg, int max_reads, int m, adp_handle **out);
int adp_destroy(adp_handle *h);
int adp_set_config(adp_handle *h, const adp_cfg *cfg);
/* Layout of the LLR path.  ADP_LAYOUT_MINIBATCH (default): combined_detect_llr2, adapted/detect/combined.py:122-227.
 * ADP_LAYOUT_SINGLE_READ: combined_detect_llr, adapted/detect/combined.py:39-119 (API only in v0.2.4) -- every read
 * normalised on its own (adp_detect_llr with minibatch = 1), pooled from sample 0 with offset_head = 5 +
 * min_obs_adapter // ds, min_obs_adapter still added to the positions, no poly(A) search behind a candidate at index 0,
 * the ragged last pooled block filled up with zeros at the READ's end. */
#define ADP_LAYOUT_MINIBATCH 0
#define ADP_LAYOUT_SINGLE_READ 1
int adp_set_layout(adp_handle *h, int layout);
/* The handle's main HIP stream (hipStream_t as void*): staging copies, single-group calls and the non-LLR entry points are
 * ordered on it; asynchronous helpers (adp_calibrate_i16, adp_expand_ragged*) enqueue on it and a following detect call is
 * ordered behind them. */
void *adp_stream(adp_handle *h);
int adp_synchronize(adp_handle *h);

/* LLR primary + validation (+ optional start-peak columns) over n_reads reads.
 * rows_out: adp_row[n_reads]; mb_status: int32[ceil(n_reads/minibatch)] (host, may be NULL).
 * Rows of a dropped minibatch are zeroed with fail_code = 0 and success = 0.
 * Optional grouped execution (environment, read per call): ADP_GROUPS=k (k > 1; 0 = automatic) cuts a call that carries two or
 * more minibatches into about k groups of whole minibatches that run software-pipelined over ADP_LANES (default 2, <= 4)
 * internal streams, each with a workspace for ONE group -- while one group streams the signal for its normalisation, pooling
 * or partition statistics, its neighbour runs the float64 gains and the peak picking on its pooled trace; ADP_STAGGER=bits
 * orders phase p (bit 0 streaming-in, 1 gains, 2 validation) of consecutive groups.  Minibatches are independent of each
 * other, so the rows are the same bytes whatever the grouping (tests/test_gpu_grouped.py).  The default is one group: on
 * MI355X the overlap buys no time (profiles/r03_overlap_*), a smaller workspace is what grouping is for.
 * N1 (the minibatch's median / MAD): minibatches of at least ADP_N1_FUSED_MIN samples (default 2^22 = minibatch x max_obs_trace;
 * the reference's defaults are 1000 x 16 000) take ONE verified pass over the signal, smaller ones three or four; the values are
 * the exact np.nanmedian / MAD either way.
 * With ADP_FLAG_TRUNCATED in `flags` (rows_out given; an extension, off by default -- the reference ships the column
 * polya_truncated and never sets it, combined.py:606) the call ends with a look at every read's final row: does the poly(A) run
 * into the end of the preloaded window?  With obs_end = min(full_len, m), W = cfg.median_shift_window and ae = the row's primary
 * adapter end, a read is ELIGIBLE when full_len > m (a read that simply ends inside its poly(A) was not cut by the preload), its
 * row is neither an exception row nor one of a dropped minibatch, ae is present and > 0, adapter_med is present and
 * ae + W <= obs_end.  T1, on the eligible reads: the last W observed samples look like poly(A) -- the first four entries (mean,
 * var, med, range) of the check vector of mean_var_shift_polyA_check(signal[:obs_end], obs_end - W, obs_end, less_signal_ok =
 * True) hold, with cfg.pA_mean_range, or pA_mean_adapter_med_scale_range x the row's adapter_med where that range is empty (a NaN
 * in the window fails it).  T2, on the reads that passed T1: the call's own validation with the boundaries (ae, obs_end), k = 1
 * and Boundaries.polya_truncated = True, i.e. the reference's gates decide whether everything observed behind the adapter is
 * poly(A).  Where T2's row passes it REPLACES the read's row with bit 1 of adp_row.reserved_ set; the primary's poly(A) end, cand[],
 * the start-peak columns and start_peak_type and bit 0 of reserved_ stay those of the first row.  Every other row keeps its
 * bytes, apart from bit 2 of reserved_, which the flag sets in every row of the call.  T2's open-pore lists share the call's
 * arena; adp_debug_fetch(12) has the counts.  ADP_ERR_UNSUPPORTED, before anything is launched: mvs_detect_check == 0,
 * mvs_detect_overwrite != 0, ADP_LAYOUT_SINGLE_READ, adp_detect_llr_i16, adp_detect_start_peak, W > 4096, or a
 * pA_mean_window / pA_var_window outside [1, W - 3] (T1 is the windowed form of the check).  Without the flag every row of every
 * call keeps the bytes it had before the flag existed. */
int adp_detect_llr(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m,
                   int minibatch, int flags, adp_row *rows_out, int32_t *mb_status);

/* The same over RAW samples (an EXTENSION of the boundary: the reference's operators take calibrated
 * float32): raw = DEVICE int16 [n_reads, m] as the sequencer stores them, scale / offset = DEVICE float32 [n_reads] (pod5's
 * per-read calibration), full_len = DEVICE int32 [n_reads]; flags must hold ADP_IN_DEVICE.  Every kernel that touches the
 * signal forms pA = scale * (float32(adc) + offset) in registers (both operations rounded to float32, never fused --
 * bit-identical to adp_calibrate_i16's output) and treats samples at or beyond min(full_len, m) as the NaN padding of
 * adapted/file_proc.py:170-174, so rows are identical to adp_calibrate_i16 + adp_detect_llr while every streaming pass
 * moves 2 bytes per sample instead of 4.  m must be a multiple of 4.  The CNN primary has the same twin, adp_detect_cnn_i16,
 * declared in adapted_hip_i16.h. */
int adp_detect_llr_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset,
                       int n_reads, int m, int minibatch, int flags, adp_row *rows_out, int32_t *mb_status);

/* Start-peak primary + validation. */
int adp_detect_start_peak(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads,
                          int m, int minibatch, int flags, adp_row *rows_out);

/* CNN head, C1: the network's input.
 * prepared_out: float32 [n_reads, Lc] with Lc = ceil((m - min_obs_adapter)/downscale_factor). */
int adp_cnn_prepare(adp_handle *h, const float *signals, int n_reads, int m, int flags, float *prepared_out);
/* C2, the conv net itself (BoundariesCNN adapted/detect/cnn.py:16-52; cnn_score :85-98), hand-written for gfx950
 * (adapted_amd/csrc/cnn_conv.h: the two 64 -> 64 layers on the float32 matrix cores, fixed accumulation order).
 * adp_cnn_set_weights: HOST pointers in the layout of the reference's state dict ("0.weight" [64,1,7], "0.bias" [64],
 * "2.weight" [64,64,7], "2.bias", "4.weight" [64,64,7], "4.bias", "6.weight" [64,2,7], "6.bias" [2]).
 * adp_cnn_forward: prepared = DEVICE float32 [n_reads, Lc] (adp_cnn_prepare's output), scores_out = DEVICE float32
 * [n_reads, 2, Lo], Lo = 3 * ((Lc - 1) / 3 + 1) - 2 -- what model(x) returns in the reference. */
int adp_cnn_set_weights(adp_handle *h, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                        const float *b2, const float *w3, const float *b3);
int adp_cnn_forward(adp_handle *h, const float *prepared, int n_reads, int Lc, float *scores_out);
/* C3, cnn_predict (adapted/detect/cnn.py:101-160) and the scaling of cnn_detect (:165-182) on the device
 * (adapted_amd/csrc/cnn_topk.h).  scores: DEVICE float32 [n, 2, Lo] (the conv net's output).  Reads [q * minibatch,
 * (q + 1) * minibatch) are one call of the reference: its find_peaks runs over that minibatch's FLATTENED scores and the
 * candidates of the i-th read with peaks go to row i of the minibatch (:150-158), both reproduced.
 * bounds_out: HOST int64 [n, 1 + max(k, 1)], k = cfg.polya_cand_k: adapter end and the k poly(A) candidates in samples
 * (index * downscale_factor + min_obs_adapter, a value equal to min_obs_adapter -> 0), i.e. what cnn_detect returns.
 * Exact ties between peaks closer than 5 samples: the later index counts as higher (scipy leaves it to an unstable sort). */
int adp_cnn_predict(adp_handle *h, const float *scores_dev, int n_reads, int minibatch, int Lo, int64_t *bounds_out);
/* The k > 1 part alone, behind given arg-maxes (tests): adapter_pos / polya_pos DEVICE int64 [n]; host outputs cand int32
 * [n, k] (positions inside the read, zero padded) and n_peaks int32 [n] (peaks of the read after the distance rule).
 * All n reads are one minibatch. */
int adp_cnn_topk(adp_handle *h, const float *scores_dev, const int64_t *adapter_pos_dev, const int64_t *polya_pos_dev,
                 int n_reads, int Lo, int k, int32_t *cand_out, int32_t *n_peaks_out);
/* combined_detect_cnn (adapted/detect/combined.py:230-309) in one call: prepare_data -> conv net -> cnn_predict -> the
 * validate_boundaries loop, and with ADP_CNN_FALLBACK in `flags` (and cfg.fallback_to_llr_short_reads != 0; rows_out given) its
 * short-read fallback (:251-301) on the device.  A read takes the fallback when its first row failed without an exception code
 * (ADP_F_IS_EXCEPTION), both of its predictions are > 0 and more than 1000 samples apart, and full_len < 2 * max_obs_adapter.
 * For such a read the chain of adp_llr_refine_polya runs over [adapter_end, polya_end) of the resident row; an exception status
 * (ADP_F_EXC_EMPTY_TRACE / ADP_F_EXC_MAD_ZERO) makes the row the all-None row with that fail_code; a new poly(A) end > 0 has
 * the read validated again with (adapter_end, new polya_end), k = 1, and that row REPLACES the first one (also when it fails
 * again); otherwise the first row stays.  Rows of both passes share the call's one open-pore arena.  Without the flag the call
 * stops in front of the fallback (callers that apply it themselves with adp_llr_refine_polya + adp_validate_candidates).
 * Needs adp_cnn_set_weights.  bounds_out (HOST, may be NULL) as adp_cnn_predict: what cnn_detect returned -- the fallback does
 * not rewrite it.
 * With ADP_CNN_SECOND_LLR in `flags` (rows_out given; an extension, the reference keeps its two detectors apart) every read whose
 * row has success == 0 behind all of the above -- exception rows included -- gets an LLR second opinion in the same call: the
 * LLR primary exactly as adp_detect_llr computes it for the read's minibatch in ADP_LAYOUT_MINIBATCH (N1 over all reads of the
 * minibatch), then the validation with those boundaries (k = 1).  Where that row passes it REPLACES the read's row, with bit 0 of
 * adp_row.reserved_ set; otherwise the CNN path's row stays, byte for byte.  A minibatch whose LLR status is not ADP_MB_OK (where
 * combined_detect_llr2 raises) gives none of its reads a second opinion.  Rows of reads that pass the CNN path are never touched;
 * bounds_out stays what cnn_detect returned; the second rows' open-pore lists share the call's arena.
 * ADP_FLAG_TRUNCATED: as for adp_detect_llr, on the rows behind all of the above (a second-opinion row that is flagged keeps
 * bit 0 of reserved_).
 * ADP_WITH_START_PEAK (rows_out given; an extension, the reference keeps one primary per run): every read's row is exactly the row
 * of the call without the flag, with the result of detect_rna_start_peak (adapted/detect/start_peak.py:7-119, the rna_start_peak
 * numbers of cfg) overlaid as on the LLR path: a row made for an exception the reference raises (ADP_F_IS_EXCEPTION) stays bare; a
 * read whose start-peak result is not valid gets nothing; every other read gets start_peak_idx / _pa / _next_max_idx / _next_max_pa
 * with their `present` bits, start_peak_open_pore_idx only when the read is flagged, and start_peak_type.  No other byte of a row
 * changes -- success and fail_code included: failing on a flag is the start-peak primary's -- and neither does bounds_out.  This
 * holds for the row the call finally delivers, whichever phase made it (first pass, fallback, second opinion, truncation look).
 * The scan rides the pooling pass of prepare_data when cfg.sp_downscale_factor == cfg.downscale_factor and min_obs_adapter is a
 * multiple of it (ADP_SP_FUSED=0 in the environment: never), else it streams the signal once more beside the conv stack. */
int adp_detect_cnn(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m, int minibatch, int flags,
                   adp_row *rows_out, int64_t *bounds_out);
/* Validate with explicit primary boundaries: bounds int64 [n_reads, 1 + k] = adapter_end, k poly(A)
 * candidates (0 terminates), exactly what cnn_detect_boundaries hands to validate_boundaries.
 * ADP_POLYA_TRUNCATED in `flags`: Boundaries.polya_truncated is True for every read, so its RNA partition is all None
 * (ADP_ERR_UNSUPPORTED with mvs_detect_overwrite, where the reference's poly(A) end then takes another branch, combined.py:548-562). */
int adp_validate_candidates(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m,
                            const int64_t *bounds, int k, int flags, adp_row *rows_out);

/* CNN fallback for short reads (adapted/detect/combined.py:251-301): per-read normalisation, LLR trace
 * (offsets 5/5) over [ranges[2i], ranges[2i+1]) and P4 on it.  polya_out[i] = new poly(A) end in samples or 0;
 * status_out[i] = 0 or the ADP_F_EXC_* code of the exception the reference would have raised. */
int adp_llr_refine_polya(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m,
                         const int64_t *ranges, int flags, int64_t *polya_out, int32_t *status_out);

/* The open-pore arena of the LAST detect / validate call on this handle: find_open_pores (adapted/detect/anomalies.py:15-35)
 * returns a list without a length limit, and the CSV prints all of it; rows with more than ADP_MAX_OPEN_PORES entries keep
 * their whole list here (row.open_pores_more = offset, row.n_open_pores = length).  ONE arena per API call, whatever the
 * number of minibatches (or internal groups) the call carries: the offsets of all its rows index the same array.  Copies
 * min(used, cap) int32 entries to the HOST buffer `out` and the number in use to *used (a call that finds the arena too
 * small grows it and runs again before it returns: a call never loses entries). */
int adp_open_pores_arena(adp_handle *h, int32_t *out, uint64_t cap, uint64_t *used);

/* Synthetic squiggles generated on the device (bit-identical to adapted_amd/synth.py).
 * dev_signals: device float32 [n, m]; dev_full_len: device int32 [n] or NULL (=> all m). */
int adp_synth_fill(adp_handle *h, float *dev_signals, const int32_t *dev_full_len, int n, int m,
                   uint32_t seed, uint32_t first_read, int decorate);

/* Device memory helpers so callers need no HIP binding of their own. */
int adp_dev_alloc(adp_handle *h, uint64_t bytes, void **out);
int adp_dev_free(adp_handle *h, void *p);
int adp_memcpy_h2d(adp_handle *h, void *dst, const void *src, uint64_t bytes);
int adp_memcpy_d2h(adp_handle *h, void *dst, const void *src, uint64_t bytes);
/* int16 ingestion (an EXTENSION of the boundary: the reference's operators take calibrated float32):
 * raw ADC samples int16 [n, m] + per-read calibration -> the float32 [n, m] NaN-padded minibatch the detect entry points
 * take, on the device, so that only 2 bytes per sample cross PCIe.  pA = scale * (float32(adc) + offset), both
 * operations rounded to float32 -- pod5's calibrate_signal_array; pod5 is not in this build's container, so the formula
 * is unpinned against it and stated here.  Samples at or beyond min(full_len, m) become NaN (minibatch layout B0,
 * adapted/file_proc.py:170-174).  All pointers are DEVICE pointers. */
int adp_calibrate_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset,
                      int n_reads, int m, float *signals_out);

/* Ragged ingestion (extension, next to adp_calibrate_i16): the reads of a minibatch packed back to back -- read r's first
 * min(full_len[r], m) samples at packed[offsets[r] ...], float32 pA or (is_int16) raw ADC samples with per-read
 * calibration -- are laid out as the float32 [n, m] NaN-padded minibatch on the device.  Only the samples that exist
 * cross PCIe: with heavy-tailed read lengths most of the padded matrix is NaN (84 % for BASELINE configs[4]).
 * All pointers are DEVICE pointers; scale / offset may be NULL for float32 input. */
int adp_expand_ragged(adp_handle *h, const void *packed, int is_int16, const int64_t *offsets, const int32_t *full_len,
                      const float *scale, const float *offset, int n_reads, int m, float *signals_out);

/* Packed raw samples -> the raw int16 [n, m] matrix adp_detect_llr_i16 reads (zeros behind each read; DEVICE pointers). */
int adp_expand_ragged_i16(adp_handle *h, const int16_t *packed, const int64_t *offsets, const int32_t *full_len, int n_reads, int m,
                          int16_t *raw_out);

/* Streaming input (adapted_amd/pipeline.py): page-locked host staging memory, and a host-to-device copy on the handle's
 * COPY stream (neither the compute stream nor its side stream), so that the copy of the next minibatch overlaps the
 * detect call of the current one.  adp_copy_mark(slot) marks the copies issued so far (slot in [0, 16));
 * adp_copy_wait(slot) blocks the host until the copies marked by that slot have landed (slot < 0: all copies). */
int adp_host_alloc(adp_handle *h, uint64_t bytes, void **out);
int adp_host_free(adp_handle *h, void *p);
int adp_memcpy_h2d_async(adp_handle *h, void *dst, const void *src_pinned, uint64_t bytes);
int adp_copy_mark(adp_handle *h, int slot);
int adp_copy_wait(adp_handle *h, int slot);

/* The reference's native module (adapted/detect/_c_llr.pyx, imported at adapted/detect/llr.py:18) as a batched call:
 * `c_llr_trace(raw_signal, start, end, min_obs, border_trim, stride, adapter_early_stopping, adapter_early_stop_window,
 * adapter_early_stop_stride, polya_early_stopping, polya_early_stop_window, polya_early_stop_stride, return_c_c2)` (:202-236)
 * for n_reads float64 signals -- raw [n_reads, L], read r valid in [0, len[r]) -- with `_gains` (:67-88) and both early-stopping
 * forms (`_gains_w_early_stop` :91-122, `_gains_w_polya_early_stop` :125-173) behind the same dispatch (:190-197).
 *   gain_out [n_reads, L]   zeros outside the computed points, as np.zeros_like(c)
 *   c_io, c2_io [n_reads, L] np.cumsum(raw), np.cumsum(raw * raw): outputs (may be NULL), or -- with ADP_TRACE_FROM_SUMS, the
 *                           form of `c_llr_trace_gains` (:176-199) and `_gains` -- the INPUTS (raw is ignored, may be NULL)
 *   len, start, end         HOST int32 [n_reads] (checked here: 0 <= start <= end <= len <= L)
 *   flags                   ADP_IN_DEVICE: raw (or the sums) are device pointers; ADP_OUT_DEVICE: gain_out (and the sums when
 *                           they are outputs) are device pointers
 * Returns ADP_ERR_INVALID where the reference asserts (an early-stop stride that is not a multiple of `stride`) or would
 * index outside its arrays.  The product path does not go through here (adp_detect_llr has its own fused passes). */
typedef struct adp_trace_args {
    int32_t min_obs, border_trim, stride;
    int32_t adapter_early_stopping, adapter_early_stop_window, adapter_early_stop_stride;
    int32_t polya_early_stopping, polya_early_stop_window, polya_early_stop_stride;
} adp_trace_args;
#define ADP_TRACE_FROM_SUMS 64
int adp_c_llr_trace(adp_handle *h, const double *raw, const int32_t *len, const int32_t *start, const int32_t *end, int n_reads,
                    int L, const adp_trace_args *args, int flags, double *gain_out, double *c_io, double *c2_io);

/* The rest of the reference's native module: `_best_split` (_c_llr.pyx:40-64) and the unnormalised 3-split segmenters
 * `c_llr_detect_adapter` (:239-287) / `c_llr_detect_adapter_polya` (:290-365), batched (adapted_amd/csrc/llr_detect_api.h).
 *
 * adp_c_llr_best_split: per row r of the cumulative sums c, c2 [n_reads, L] (row r valid in [0, len[r])), the best split of
 *   [start[r], end[r]) over the points [start + offset_head, end - offset_tail) -> x_out (int64, -1 when no gain is > 0) and
 *   gain_out (0.0 then).  len, start, end, offset_head, offset_tail: HOST int32 [n_reads], checked here (0 <= start <= end <= len
 *   <= L, offsets >= 0).  flags: ADP_IN_DEVICE -- c, c2 are device pointers.  x_out / gain_out: host.
 * adp_c_llr_detect: raw [n_reads, L] float64 (float32 with ADP_CLLR_F32: widened on the device, the rows of x.astype(float64)),
 *   read r valid in [0, len[r]), len HOST int32 [n_reads] with 1 <= len <= L; offsets >= 0.  flags: ADP_IN_DEVICE -- raw is a
 *   device pointer; ADP_CLLR_POLYA -- c_llr_detect_adapter_polya (else c_llr_detect_adapter).  Host outputs:
 *     rows_out   int64 [n_reads, 4]  adapter_start, adapter_end, polya_end, and the LENGTH of the tuple the reference returns:
 *                2 for c_llr_detect_adapter, and for c_llr_detect_adapter_polya when the first split finds nothing (its
 *                `return 0,0`, :310-312); 3 otherwise (polya_end 0 in a 2-tuple row)
 *     splits_out int64 [n_reads, 4] or NULL: x_first, x_head, x_tail, x_polya as the searches returned them (-1: none / not searched)
 *     stats_out  double [n_reads, 8] or NULL: the gains of those four searches, then the four medians (0.0 where not computed) */
#define ADP_CLLR_POLYA 128
#define ADP_CLLR_F32 256
int adp_c_llr_best_split(adp_handle *h, const double *c, const double *c2, const int32_t *len, const int32_t *start, const int32_t *end,
                         const int32_t *offset_head, const int32_t *offset_tail, int n_reads, int L, int flags, int64_t *x_out, double *gain_out);
int adp_c_llr_detect(adp_handle *h, const void *raw, const int32_t *len, int n_reads, int L, int32_t min_obs_adapter, int32_t border_trim,
                     int32_t min_obs_polya, int flags, int64_t *rows_out, int64_t *splits_out, double *stats_out);

/* The reference's Python LLR module (adapted/detect/llr.py) above its native one, batched on traces [n_reads, L] float64 (read r
 * valid in [0, len[r])), one wave per read (adapted_amd/csrc/trace_peaks_api.h).  len and every other per-read array: HOST int32
 * [n_reads], checked here (0 <= len <= L).  flags: ADP_IN_DEVICE -- `trace` is a device pointer (resident traces never cross
 * PCIe).  Outputs: host memory.
 *
 * adp_llr_trace_bounds: the derived state of `LLRTrace` (llr.py:53-132) -- `_trace_start_end` (:135-142: the first and last index
 *   whose value is not <= 0, NaN counting as positive; 0 and len - 1 when there is none), `early_stop` (:86: end <
 *   `max_len_no_early_stop` :72-84, np.arange(min_obs, len - 1 - tail_trim, stride)[-1], len - 1 - tail_trim for an empty
 *   range) and, with ADP_LLR_INTERP and stride > 1, `interp_stride` (:116-132) IN PLACE (a host trace is copied back): np.interp
 *   of the knots -- the indices in [start, end) whose value is != 0, NaN included -- bit for bit, left = right = 0.
 *   min_obs, tail_trim: per read (calc_polya_trace derives both from adapter_end, :375-381).  early_stop_out: bit 0 the flag,
 *   bit 1 set when interpolation was asked for and the knot set is empty (numpy raises ValueError; the trace is unchanged).
 * adp_llr_trace_peaks: `find_peaks_in_trace` (:204-224) on trace[clip_lo:clip_hi] -- scipy's find_peaks with prominence
 *   args->prominence * np.nanstd(clip) (numpy's summation order), width and rel_height -- then for EVERY peak, in index order,
 *   `correct_for_plateau` (:145-177) and `correct_for_split_peak` (:180-201) as `adapter_end_from_trace` (:227-263) applies them
 *   (each when its `*_on` is set, with its own s / t / window; the split test's find_peaks uses width = split_s, the absolute
 *   split_prominence and rel_height 0.5).  peaks_out int64 [n_reads, cap]: full-trace indices, -1 padding; count_out int64
 *   [n_reads]: the true number of peaks, also when it exceeds cap.  0 <= clip_lo <= clip_hi <= len; plateau_s >= 1.
 *   With ADP_LLR_GIVEN_PEAK, clip_lo[r] is a peak (0 <= clip_lo < len) that only the corrections are applied to (the reference's
 *   correct_for_plateau / correct_for_split_peak on their own; clip_hi is not read, count_out is 1).
 * adp_llr_spike_peak: `detect_full_polya_trace_peak_with_spike` (:406-479) with all five parameters -> out int64 [n_reads] (0: no
 *   peak).  scipy's find_peaks(np.nan_to_num(trace, nan=0), distance, prominence, width, rel_height=0.5): the distance selection
 *   over ALL local maxima first (ties: the later index wins), then prominence and width; the heights, np.argmin and
 *   linregress's r on the trace as given.  min_peak_distance >= 1 (scipy's ValueError otherwise). */
typedef struct adp_peak_args {
    double prominence, width, rel_height;             /* find_peaks_in_trace; prominence relative to np.nanstd(clip) */
    double plateau_t, split_t, split_prominence;
    int32_t plateau_on, plateau_s, plateau_window;    /* correct_for_plateau(trace, peak, s, t, window) */
    int32_t split_on, split_s, split_window;          /* correct_for_split_peak(trace, peak, s, t, window, prominence) */
} adp_peak_args;
typedef struct adp_spike_args {
    double min_peak_distance, prominence_threshold, min_width, threshold_prominence_ratio, threshold_r_squared;
} adp_spike_args;
#define ADP_LLR_INTERP 512
#define ADP_LLR_GIVEN_PEAK 1024
int adp_sizeof_peak_args(void);
int adp_sizeof_spike_args(void);
int adp_llr_trace_bounds(adp_handle *h, double *trace, const int32_t *len, const int32_t *min_obs, const int32_t *tail_trim, int stride,
                         int n_reads, int L, int flags, int32_t *start_out, int32_t *end_out, int32_t *early_stop_out);
int adp_llr_trace_peaks(adp_handle *h, const double *trace, const int32_t *len, const int32_t *clip_lo, const int32_t *clip_hi, int n_reads,
                        int L, const adp_peak_args *args, int flags, int cap, int64_t *peaks_out, int64_t *count_out);
int adp_llr_spike_peak(adp_handle *h, const double *trace, const int32_t *len, int n_reads, int L, const adp_spike_args *args, int flags,
                       int64_t *out);

/* The reference's MVS poly(A) module (adapted/detect/mvs.py), batched on signals [n_reads, L] float32, or float64 with
 * ADP_MVS_F64 (read r valid in [0, len[r])), one wave per read (adapted_amd/csrc/mvs_api.h).  len and the per-read positions:
 * HOST int32 / int64 [n_reads], checked here (0 <= len <= L, positions >= 0).  flags: ADP_IN_DEVICE -- `sig` is a device
 * pointer.  Windows must be >= 1 and search_increment_step >= 1 (the reference never returns otherwise).  Outputs: host memory.
 *
 * adp_mvs_check: mean_var_shift_polyA_check (mvs.py:45-158) with the mvs_polya fields and both flags.
 * adp_mvs_detect_at_loc: mean_var_shift_polyA_detect_at_loc (mvs.py:181-338) with the mvs_polya fields and less_signal_ok.
 *   info_out int32 [n_reads, 8]: 0 the result (check_vector.all() / the accept), 1 the check vector (bit j: entry j True; check
 *   only), 2 status (0; 1 the reference raises IndexError; 2 bottleneck's ValueError), 3 and 4 the exception's numbers (ValueError:
 *   the window and the slice size; IndexError: the index and the size, -1 and 0 for np.percentile of an empty slice), 5 (check
 *   only) set when the read got past the early outs.  vals_out float64 [n_reads, 5]: mean, var, poly(A) median, local range, median shift as the reference returns them
 *   (0.0 on the early outs).  idx_out int64 [n_reads]: detect_at_loc's index (0: none).
 * adp_mvs_detect: mean_var_shift_polyA_detect (mvs.py:341-426) with the streaming fields (s_*) -> out int64 [n_reads] (0: none). */
typedef struct adp_mvs_args {
    /* [mvs_polya] */
    double pA_mean_range[2], pA_var_range[2], median_shift_range[2], polyA_med_range[2], polyA_local_range[2];
    int32_t search_window, pA_mean_window, pA_var_window, median_shift_window, polyA_window;
    int32_t less_signal_ok, windowed_stats;
    /* [streaming] */
    int32_t min_obs_adapter, min_obs_post_loc, search_increment_step;
    int32_t s_pA_mean_window, s_pA_var_window, s_median_shift_window, s_polyA_window;
    int32_t pad;
    double s_pA_mean_range[2], s_pA_var_range[2], s_median_shift_range[2], s_polyA_med_range[2], s_polyA_local_range[2];
} adp_mvs_args;
#define ADP_MVS_F64 2048
int adp_sizeof_mvs_args(void);
int adp_mvs_check(adp_handle *h, const void *sig, const int32_t *len, const int64_t *adapter_end, const int64_t *polya_end, int n_reads,
                  int L, const adp_mvs_args *args, int flags, int32_t *info_out, double *vals_out);
int adp_mvs_detect_at_loc(adp_handle *h, const void *sig, const int32_t *len, const int64_t *loc, int n_reads, int L,
                          const adp_mvs_args *args, int flags, int32_t *info_out, int64_t *idx_out, double *vals_out);
int adp_mvs_detect(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_mvs_args *args, int flags,
                   int64_t *out);

/* The reference's partition statistics (adapted/partition/signal_partitions.py: calc_partition_stats), batched: n_seg segments
 * signal[row, start:end] of signals [n_reads, L] float32, or float64 with ADP_MVS_F64 (read r valid in [0, len[r])), one wave per
 * segment (adapted_amd/csrc/sigstats_api.h).  A segment is clipped to its read as a Python slice is (end or start beyond len[row]);
 * start < 0 or end <= start gives an empty one.  len and segs: HOST arrays, checked here (0 <= len <= L, 0 <= row < n_reads,
 * positions <= 2^40).  flags: ADP_IN_DEVICE -- `sig` is a device pointer.  Outputs, host memory: stats_out float64 [n_seg, 4] --
 * np.mean, np.std, np.median and np.median(np.abs(x - median)) of the clipped slice, computed in the signals' type in numpy's
 * order of operations and widened exactly (NaN x 4 for an empty slice; a NaN sample makes all four NaN); count_out int64 [n_seg]
 * -- the clipped slice's size. */
typedef struct adp_seg {
    int64_t start, end;
    int32_t row, pad;
} adp_seg;
int adp_sizeof_seg(void);
int adp_seg_stats(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg, int flags,
                  double *stats_out, int64_t *count_out);

/* The reference's signal statistics modules next to it, on the same batches (float32, or float64 with ADP_MVS_F64;
 * ADP_IN_DEVICE: `sig` / `data` is a device pointer; every call completes before it returns; outputs: host memory unless said
 * otherwise).  Kernels: adapted_amd/csrc/sigstats_api.h.
 *
 * adp_med_mad: med_mad (adapted/detect/normalize.py) of every row's [0, len[r]) -> out float64 [n_reads, 2]; with ADP_SS_WHOLE
 *   of the whole [n_reads, L] array as one population (len is not read and may be NULL) -> out [1, 2].  ADP_SS_NANSKIP:
 *   np.nanmedian's (with_nan=True).  Nothing counted: NaN.  A population of more than ADP_SS_GRID_MIN samples is selected by
 *   many workgroups, a smaller one by one workgroup; ADP_SS_FORCE_GRID / ADP_SS_FORCE_WAVE choose (tests).
 * adp_normalize: normalize_signal -- (clip(x, med - mad * thresh, med + mad * thresh) - med) / mad with each row's own median
 *   and MAD, or the whole array's with ADP_SS_WHOLE -> out [n_reads, L] of the input's type (host, or device with
 *   ADP_OUT_DEVICE; cells behind len[r] are not written), medmad_io float64 [n_reads, 2] / [1, 2], status_out int32 [n_reads] /
 *   [1]: 1 where the MAD is 0 (the reference raises ValueError; the row is not written).  ADP_SS_CLIP: clip_signal -- medmad_io
 *   is an INPUT and only the clip is applied.
 * adp_pool_mean: efficient_average_pooling (adapted/detect/downscale.py) of data [n_rows, n_cols] -> out [n_rows,
 *   ceil(n_cols / pool_size)] of the input's type (host, or device with ADP_OUT_DEVICE); a ragged last block is filled with zeros.
 * adp_real_range: real_range_check (adapted/detect/real_range.py) of the segments -> info_out int32 [n_seg, 2]: the result; the
 *   stage reached (0 fewer than 2 * mean_window samples, 1 a mean out of range, 2 the local range taken); vals_out float64
 *   [n_seg, 3]: mean_start, mean_end (the input type's values), local range (float64).
 * adp_open_pores: find_open_pores (adapted/detect/anomalies.py) of the segments: positions from the segment's start, in
 *   [lo, hi], whose distance to the preceding position in range is >= min_obs_diff -> pos_out int64 [n_seg, cap] (the first cap
 *   of them, then -1), count_out int64 [n_seg, 3]: their number (also past cap: call again with a larger cap), the number of
 *   positions in range, the last of those (-1: none). */
#define ADP_SS_NANSKIP 4096
#define ADP_SS_WHOLE 8192
#define ADP_SS_CLIP 16384
#define ADP_SS_FORCE_GRID 32768
#define ADP_SS_FORCE_WAVE 65536
#define ADP_SS_GRID_MIN 16384
typedef struct adp_real_range_args {
    double mean_start_range[2], mean_end_range[2], local_range[2];
    int32_t mean_window, max_obs_local_range;
} adp_real_range_args;
int adp_sizeof_real_range_args(void);
int adp_med_mad(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, int flags, double *out);
int adp_normalize(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, double outlier_thresh, int flags,
                  double *medmad_io, void *out, int32_t *status_out);
int adp_pool_mean(adp_handle *h, const void *data, int n_rows, int n_cols, int pool_size, int flags, void *out);
int adp_real_range(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                   const adp_real_range_args *args, int flags, int32_t *info_out, double *vals_out);
int adp_open_pores(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg, double lo,
                   double hi, double min_obs_diff, int flags, int cap, int64_t *pos_out, int64_t *count_out);

/* The reference's start-peak and adapter-start modules (adp_start_peak, adp_adapter_start): the part of this ABI that is declared
 * in a header of its own, with its own prototype table in adapted_amd/lib.py (MODULE_PROTOTYPES). */
#include "adapted_hip_startmods.h"

/* The CNN primary over raw int16 rows, adp_detect_cnn_i16: declared in a header of its own as well, with its prototype table in
 * adapted_amd/lib.py, I16_PROTOTYPES. */
#include "adapted_hip_i16.h"

/* Event segmentation of signal segments and the statistics of the event lengths -- adp_segment_events, an extension --: declared in
 * a header of its own, with its prototype table in adapted_amd/lib.py, EVENT_PROTOTYPES. */
#include "adapted_hip_events.h"

/* Adapter event fingerprints and their comparison by dynamic time warping -- adp_event_levels and adp_dtw_assign, an extension --:
 * a header of its own again, with its prototype table in adapted_amd/lib.py, FINGERPRINT_PROTOTYPES. */
#include "adapted_hip_fingerprint.h"

/* The packed forms of those two event calls -- segments back to back in one array, float32 pA or raw int16 samples with a
 * calibration per segment (ADP_PACKED_I16, 1 << 24), an extension --: a header of its own, with its prototype table in
 * adapted_amd/lib.py, EVENT_PACKED_PROTOTYPES. */
#include "adapted_hip_events_packed.h"

/* The adapter's front boundary as a post-pass over the rows of a detect call -- adp_adapter_front and adp_adapter_front_i16, an
 * extension --: a header of its own, with its prototype table in adapted_amd/lib.py, ADAPTER_FRONT_PROTOTYPES. */
#include "adapted_hip_adapter_front.h"

/* Validation from a given adapter start -- adp_validate_candidates_from -- and the front pass that validates its trimmed rows again
 * -- adp_adapter_front_revalidate and adp_adapter_front_revalidate_i16, an extension --: a header of its own, with its prototype
 * table in adapted_amd/lib.py, REVALIDATE_PROTOTYPES. */
#include "adapted_hip_revalidate.h"

/* Building barcode templates: the warping path of a DTW alignment and one iteration of DTW barycentre averaging -- adp_dtw_align
 * and adp_dba_step, an extension --: a header of its own, with its prototype table in adapted_amd/lib.py, TEMPLATE_PROTOTYPES. */
#include "adapted_hip_templates.h"

/* Clustering fingerprints without labels -- the all-pairs DTW matrix, PAM's BUILD, alternating k-medoids and the silhouette, on a
 * matrix that stays on the device; an extension --: a header of its own, with its prototype table in adapted_amd/lib.py,
 * CLUSTER_PROTOTYPES. */
#include "adapted_hip_clusters.h"

/* The k nearest labelled fingerprints of every query under DTW, pairs abandoned behind a lower bound -- adp_dtw_knn, an extension --:
 * a header of its own, with its prototype table in adapted_amd/lib.py, KNN_PROTOTYPES. */
#include "adapted_hip_knn.h"

/* Re-segmentation of reads the LLR primary fails -- ADP_LLR_RESEGMENT, a flag of adp_detect_llr, an extension --: its rule, its row
 * bits and its counters in a header of its own; it declares no entry point (adapted_amd/lib.py, RESEGMENT_PROTOTYPES, is empty). */
#include "adapted_hip_resegment.h"

/* The same re-segmentation behind the CNN primary's LLR second opinion -- ADP_CNN_SECOND_RESEGMENT, a flag of adp_detect_cnn(_i16), an
 * extension --: its rule and its counters in a header of its own; no entry point (adapted_amd/lib.py, SECOND_RESEGMENT_PROTOTYPES,
 * is empty). */
#include "adapted_hip_second_resegment.h"

/* The rows of one output file to that file's CSV text on the GPU -- adp_format_rows, an extension --: a header of its own, with its
 * prototype table in adapted_amd/lib.py, CSV_PROTOTYPES. */
#include "adapted_hip_csv.h"

/* Per-kernel timing of the LAST detect call, measured with HIP events on the handle's stream.
 * Enable with adp_set_profiling(h, 1).  names_out: up to cap pointers to static strings. */
int adp_set_profiling(adp_handle *h, int on);
int adp_kernel_times(adp_handle *h, const char **names_out, float *ms_out, int cap);

/* Debug/inspection of intermediate stages of the last LLR call (tests only).
 * what: 0 norm params double[4*n_minibatch]; 1 n_valid int32[n]; 2 pooled float32[n*Lp];
 *       3 trace float64[n*Lp] (pass-2 trace after a full call); 4 adapter idx int32[n];
 *       5 polya idx int32[n]; 6 Lp (int32[1]); 7 the T1 pairs int32[2*n];
 *       8 process-wide tallies uint64[8..48] (cumulative): 0 large S1 segments, 1 MAD brackets that held, 2 generic median
 *         selections, 3 MADs not predicted, 4 MAD bracket overflows (0-4 are kept on 256 cache lines by workgroup and summed
 *         here: per-workgroup device atomics on one address serialise chip-wide), 5 single-pass N1 attempts, 6 / 7 their
 *         median / MAD misses, 22 / 23 N1 heavy keys / samples; the rest: phase cycles of -DADP_PHASE_TIMING builds
 *       10 int32[3], the fallback of the last adp_detect_cnn call: reads selected, exception rows made, rows re-validated
 *       11 int32[4], the LLR second opinion of the last adp_detect_cnn call: reads selected, rows replaced, rows re-validated and
 *          still failing, minibatches (with a selected read) that gave none
 *       12 int32[3], the truncation look of the last adp_detect_llr / adp_detect_cnn call made with ADP_FLAG_TRUNCATED: eligible
 *          reads, reads whose tail window looks like poly(A) (T1), rows replaced
 *       25 int32[3], the re-segmentation of the last adp_detect_llr call (ADP_LLR_RESEGMENT, adapted_hip_resegment.h): eligible
 *          reads, reads whose second segmentation found a poly(A) end, rows replaced
 *       9 int8[n], 1: the read's moving-window series were prepared by a series kernel
 *       What phase C's kernels hand to each other (nck = Lp / 16, nsum = Lp / 64; a copy beyond the buffer is ADP_ERR_INVALID):
 *       13 ck float64[n*nck*2]: (c, c2) in front of pooled sample 16 q, written for q < ceil(n_valid / 16);
 *       14 tail float64[n*2]: (c, c2)[n_valid - 2]; 15 / 16 bmax / bmin float64[n*nsum]: the trace's maximum / minimum per 64
 *       points, written for blocks below ceil(n_valid / 64) -- pass 1: NaN counts as +inf in bmax and is left out of bmin,
 *       pass 2: of the np.nan_to_num trace; 17 gstat float64[n*3]: sum, sum of squares, NaN count of pass 1's trace;
 *       18 npk int32[n]: strict local maxima of pass 2's sanitised trace, -1: a plateau was met (k_polya_peak recounts);
 *       19 pk int32[n*(Lp/2+1)]: their positions; 20 pkv float64[n*(Lp/2+1)]: their heights (ADP_ERR_INVALID on a handle made
 *       with ADP_PK_VALUES=0); 21 int32[n_minibatch]: the minibatches' status words.  Reads of a dropped minibatch and reads
 *       whose pass did not run (no adapter candidate: pass 2) keep what an earlier call left.
 *       22 wend int32[n]: pass 2 computed the read's trace, summaries and maxima on [0, wend) (ADP_G2_WINDOW; n_valid: all of it;
 *       a read of the redo list ends with n_valid); 23 int32[n+1]: the windowed pass 2's redo list of the last call, count then reads
 *       (in no order).  Tallies 78 / 79 of selector 8: windowed reads decided inside the window / sent to the redo list.
 *       24 uint32[n_minibatch * 78]: what the single-pass N1 (n1_fused.h) of the last plain call left behind, per
 *       minibatch: words 0-9 the brackets as float bits and flags (med_s, A0, A1, D0, D1, eps, ok, wide_ok, D0w, D1w; D0 / D1 are
 *       the band the pass used), 10 whether the pass settled the minibatch, 11 its status word, 12 the number of heavy keys,
 *       13 the sample points inside the brackets, 14-45 the heavy keys (ascending, order-preserving uint32 keys of the float32
 *       values), 46-77 the samples the pass counted on each.  bytes must be exactly that; ADP_ERR_INVALID when the last call did
 *       not take the single-pass route (or was grouped).  Tallies 17 / 18 / 19 of selector 8 count the minibatches whose band
 *       list / median list / LDS staging overflowed (shared with k_partition_stats' own tallies in those slots). */
int adp_debug_fetch(adp_handle *h, int what, void *host_out, uint64_t bytes);
/* Run the LLR pipeline only up to a stage (1 N1, 2 pool, 3 cumsum, 4 gains1, 5 adapter, 6 gains2, 7 polya) */
int adp_debug_llr_upto(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m,
                       int minibatch, int flags, int stage);

/* fdiv_shared (adapted_amd/csrc/common.h: float32 division by a divisor shared by many numerators) against the IEEE
 * division, for `count` consecutive float bit patterns from first_bits on and their negatives (tests only) */
int adp_debug_divcheck(adp_handle *h, float d, uint32_t first_bits, uint32_t count, uint64_t *mismatches_out);
/* log_cr (adapted_amd/csrc/log_cr.h), the logarithm of the gains kernels, applied to n host doubles (tests only) */
int adp_debug_log(adp_handle *h, const double *host_in, double *host_out, int n);

#ifdef __cplusplus
}
#endif
#endif /* ADAPTED_HIP_H */
