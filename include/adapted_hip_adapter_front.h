/* adapted_hip_adapter_front.h -- the adapter's front boundary as a post-pass over the rows of a detect call (an EXTENSION: the
 * reference ships the detector, adapted/detect/adapter_start.py:20-54, and nothing in it calls it).  Part of the C ABI of
 * include/adapted_hip.h, which includes this file (inside its extern "C" block, behind its types and flags): include that one.
 * adapted_amd/lib.py restates these prototypes in ADAPTER_FRONT_PROTOTYPES; tests/test_adapter_front_cpu.py holds that table
 * against this header, as tests/test_host_cpu.py holds PROTOTYPES against adapted_hip.h. */
#ifndef ADAPTED_HIP_ADAPTER_FRONT_H
#define ADAPTED_HIP_ADAPTER_FRONT_H

/* adp_adapter_front: `rows` are the n_reads rows of a finished detect call over `sig`, the float32 [n_reads, m] minibatch that
 * call took (calibrated pA, not the normalised signal: the threshold is min_pA_current).  For every row r with success == 1 and
 * adapter_end present, with a0 = adapter_start (0 if absent) and ae = adapter_end:
 *   x = sig[r, a0:ae];  s = moving_mean_adapter_start_detect(x, args) in the float32 arithmetic of adp_adapter_start (bottleneck's
 *   chain, both cumulative sums in float32, `difference` in float64)
 *   the reference would raise bottleneck's ValueError (len(x) - min_obs_adapter < window): status 2, the row keeps every byte
 *   s > 0 and ae - (a0 + s) >= min_adapter_len: the row is PATCHED -- adapter_start = a0 + s, adapter_len = ae - adapter_start,
 *     adapter_mean / std / med / mad = calc_partition_stats(sig[r, adapter_start:ae]) (numpy's float32 results, as every other
 *     partition statistic of a row), bit 3 of adp_row.reserved_ (ADP_ROW_ADAPTER_FRONT) set.  Every other byte of the row stays:
 *     real_adapter_*, adapter_rna_median_shift, the MVS columns, open_pores, success and fail_code are those of the validation
 *     with the first adapter_start -- validation is NOT repeated
 *   otherwise (a failing row, s == 0, a NaN in the slice, too little adapter left) the row keeps every byte.
 * A row whose a0 / ae do not satisfy 0 <= a0 <= ae <= m is not looked at.  The defaults of MMAdapterStartConfig (window 100,
 * min_obs_adapter 2500, min_shift 20, min_pA_current 90) are the reference's and UNTUNED for RNA004.
 * flags: ADP_IN_DEVICE -- `sig` is a device pointer (else host memory, staged in); ADP_OUT_DEVICE -- `rows` is device memory and is
 * patched in place (else host memory, staged in and out).  full_len is not read by this form (the matrix is read as it lies: NaN
 * behind a read's end) and may be NULL.  Side outputs, host memory, one entry per read:
 *   info_out  int32 [n_reads, 4]  status (-1 the row was not looked at, 0 fine, 2 the ValueError), the exception's window and slice
 *                                 size, 1 where the row was patched
 *   shift_out int64 [n_reads]     s (0: the detector accepted nothing)
 *   cand_out  int64 [n_reads]     np.argmin(difference) (-1: difference is empty, the exception, or not looked at)
 *   diff_out  double [n_reads]    difference[cand]
 * adp_adapter_front_i16: the same over RAW rows -- raw = DEVICE int16 [n_reads, m], scale / offset = DEVICE float32 [n_reads],
 * full_len = DEVICE int32 [n_reads], as adp_detect_llr_i16 / adp_detect_cnn_i16 take them; pA = scale * (float32(adc) + offset) is
 * formed in registers, samples at or beyond min(full_len, m) read as NaN: rows and side outputs are those of adp_calibrate_i16 +
 * adp_adapter_front.  flags must hold ADP_IN_DEVICE.
 * Refused before anything is launched (the handle stays usable): null pointers, n_reads or m < 1, window < 1, min_obs_adapter or
 * min_adapter_len < 0, the int16 form without ADP_IN_DEVICE -- ADP_ERR_INVALID; m % 4 != 0 on the int16 form (8-byte aligned rows)
 * and ADP_LAYOUT_SINGLE_READ -- ADP_ERR_UNSUPPORTED.  The call completes before it returns. */
typedef struct adp_adapter_front_args {
    double min_shift, min_pA_current;
    int32_t window, min_obs_adapter; /* up to here: adp_adapter_start_args */
    int32_t min_adapter_len, pad;
} adp_adapter_front_args;
int adp_sizeof_adapter_front_args(void);
int adp_adapter_front(adp_handle *h, const float *sig, const int32_t *full_len, int n_reads, int m, adp_row *rows,
                      const adp_adapter_front_args *args, int flags, int32_t *info_out, int64_t *shift_out, int64_t *cand_out,
                      double *diff_out);
int adp_adapter_front_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset,
                          int n_reads, int m, adp_row *rows, const adp_adapter_front_args *args, int flags, int32_t *info_out,
                          int64_t *shift_out, int64_t *cand_out, double *diff_out);

#endif /* ADAPTED_HIP_ADAPTER_FRONT_H */
