/* adapted_hip_i16.h -- the CNN primary over raw int16 ADC rows.  Part of the C ABI of include/adapted_hip.h, which includes this
 * file (inside its extern "C" block, behind its types and flags): include that one.  adapted_amd/lib.py restates these prototypes
 * in I16_PROTOTYPES; tests/test_cnn_i16_cpu.py holds that table against this header, as tests/test_host_cpu.py holds PROTOTYPES
 * against adapted_hip.h.  (adp_detect_llr_i16, the LLR primary's twin, is declared in adapted_hip.h itself.) */
#ifndef ADAPTED_HIP_I16_H
#define ADAPTED_HIP_I16_H

/* adp_detect_cnn over RAW samples (an EXTENSION of the boundary, like adp_detect_llr_i16: the reference's operators take
 * calibrated float32): raw = DEVICE int16 [n_reads, m] as the sequencer stores them, scale / offset = DEVICE float32 [n_reads]
 * (pod5's per-read calibration), full_len = DEVICE int32 [n_reads]; flags must hold ADP_IN_DEVICE (else ADP_ERR_INVALID).
 * rows_out: host, or device with ADP_OUT_DEVICE; bounds_out: host or NULL, int64 [n_reads, 1 + max(k, 1)].
 *
 * Every kernel that touches the signal -- the pooling pass in front of the conv stack, the moving-window series, the shared
 * order-statistics sweeps, the validation and the partition statistics, the start-peak scan, and behind the first pass the
 * fallback's chain, the LLR second opinion and both re-validations, which read the selected rows where they lie -- forms
 * pA = scale * (float32(adc) + offset) in registers (both operations rounded to float32, never fused: bit-identical to
 * adp_calibrate_i16's output) and treats samples at or beyond min(full_len, m) as the NaN padding of adapted/file_proc.py:170-174.
 * So rows, bounds_out, the open-pore arena and the counts of adp_debug_fetch(10) / (11) are identical to adp_calibrate_i16
 * followed by adp_detect_cnn with the same flags, while no float32 matrix exists and every pass over the signal moves 2 bytes per
 * sample instead of 4.  ADP_CNN_FALLBACK, ADP_CNN_SECOND_LLR, ADP_WITH_START_PEAK and ADP_OUT_DEVICE mean what they mean for
 * adp_detect_cnn, in both execution forms (one chunk; ADP_CNN_GROUPS).
 *
 * Refused before anything is launched: m % 4 != 0 (8-byte aligned rows), ADP_LAYOUT_SINGLE_READ and ADP_FLAG_TRUNCATED (the
 * truncation look is a float32-row phase: adp_calibrate_i16 + adp_detect_cnn) with ADP_ERR_UNSUPPORTED; missing weights,
 * m <= min_obs_adapter, null arguments and capacity as adp_detect_cnn refuses them.  A refused call leaves the handle usable. */
int adp_detect_cnn_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset,
                       int n_reads, int m, int minibatch, int flags, adp_row *rows_out, int64_t *bounds_out);

#endif /* ADAPTED_HIP_I16_H */
