/* adapted_hip_startmods.h -- the start-peak and adapter-start modules of libadapted_hip.so.  Part of the C ABI of
 * include/adapted_hip.h, which includes this file (inside its extern "C" block, behind its types and flags): include that one.
 * adapted_amd/lib.py restates these prototypes in MODULE_PROTOTYPES; tests/test_startmods_module_cpu.py holds that table against
 * this header, as tests/test_host_cpu.py holds PROTOTYPES against adapted_hip.h. */
#ifndef ADAPTED_HIP_STARTMODS_H
#define ADAPTED_HIP_STARTMODS_H

/* The reference's start-peak and adapter-start modules (adapted/detect/start_peak.py, adapter_start.py), batched on signals
 * [n_reads, m] / [n_reads, L] float32, or float64 with ADP_MVS_F64, one wave per read (adapted_amd/csrc/startmods_api.h).
 * full_len / len: HOST int32 [n_reads], checked here (full_len >= 0 -- it may exceed m --; 0 <= len <= L).  flags:
 * ADP_IN_DEVICE -- `sig` is a device pointer.  Outputs: host memory.
 *
 * adp_start_peak: detect_rna_start_peak (start_peak.py:19-84) with every [rna_start_peak] field an argument (downscale_factor
 *   >= 1, the offsets and start_peak_max_idx >= 0).  info_out int32 [n_reads, 5]: 0 valid (0: the reference's per-read try
 *   block raised: an all-None row), 1 start_peak_idx, 2 next_greater_idx, 3 open_pore_idx (-1: None), 4 the flagged type
 *   (0 None, 1 "open pore in adapter", 2 "potential concatemer adapter-only read"); POOLED indices (the reference multiplies
 *   them by downscale_factor).  vals_out float64 [n_reads, 2]: start_peak_pa, next_greater_pa (the input type's values).
 * adp_adapter_start: moving_mean_adapter_start_detect (adapter_start.py:20-54) of x[r, 0:len[r]) (window >= 1, min_obs_adapter
 *   >= 0).  info_out int32 [n_reads, 4]: 0 status (0; 2 bottleneck's ValueError "Moving window (=w) must between 1 and n,
 *   inclusive"), 1 and 2 its window and slice size, 3 accepted.  out int64 [n_reads]: adapter_start (0: not accepted).
 *   cand_out int64 [n_reads]: np.argmin(difference) (-1: difference is empty, or the exception).  diff_out float64 [n_reads]:
 *   difference[cand]. */
typedef struct adp_start_peak_args {
    double open_pore_pa;
    int32_t downscale_factor, start_peak_max_idx, offset1, offset2;
} adp_start_peak_args;
typedef struct adp_adapter_start_args {
    double min_shift, min_pA_current;
    int32_t window, min_obs_adapter;
} adp_adapter_start_args;
int adp_sizeof_start_peak_args(void);
int adp_sizeof_adapter_start_args(void);
int adp_start_peak(adp_handle *h, const void *sig, const int32_t *full_len, int n_reads, int m, const adp_start_peak_args *args,
                   int flags, int32_t *info_out, double *vals_out);
int adp_adapter_start(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_adapter_start_args *args,
                      int flags, int32_t *info_out, int64_t *out, int64_t *cand_out, double *diff_out);

#endif /* ADAPTED_HIP_STARTMODS_H */
