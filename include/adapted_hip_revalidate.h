/* adapted_hip_revalidate.h -- validate_boundaries from a given Boundaries.adapter_start, and the adapter-front pass that validates
 * the rows it trims again (an EXTENSION, as adp_adapter_front is).  Part of the C ABI of include/adapted_hip.h, which includes this
 * file (inside its extern "C" block, behind its types, its flags and adapted_hip_adapter_front.h): include that one.
 * adapted_amd/lib.py restates these prototypes in REVALIDATE_PROTOTYPES; tests/test_revalidate_cpu.py holds that table against this
 * header. */
#ifndef ADAPTED_HIP_REVALIDATE_H
#define ADAPTED_HIP_REVALIDATE_H

/* adp_row.reserved_ bit 4: the row is the validation from the trimmed adapter start (set together with ADP_ROW_ADAPTER_FRONT) */
#define ADP_ROW_REVALIDATED 16

/* adp_validate_candidates_from: adp_validate_candidates with Boundaries.adapter_start = starts[r] (the reference's
 * validate_boundaries, adapted/detect/combined.py:363, 398-419): adapter_med / adapter_mad and the adapter-MAD gate work on
 * signal[start:adapter_end], find_open_pores scans that slice (positions stay absolute; samples in front of the start do not exist
 * for it), and real_range_check, the MVS mean range taken from adapter_med, and the adapter partition follow.  starts: int64
 * [n_reads], lying where `bounds` lies (ADP_BOUNDS_HOST applies to both); NULL: every start is 0 -- the bytes of
 * adp_validate_candidates.  Flags and refusals as adp_validate_candidates.
 * A read with adapter_end != 0 whose start does not lie in [0, min(adapter_end, full_len, m)) -- the reference takes the median of
 * an empty slice there -- is not validated and nothing outside its row is read: it gets the row of a read without an adapter
 * (success 0, ADP_F_NO_ADAPTER, partitions from start 0).  A read with adapter_end == 0 is the read without an adapter whatever its
 * start; a negative start counts as 0 there (adapter_start of the row), so no start makes the call read outside a row. */
int adp_validate_candidates_from(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m,
                                 const int64_t *bounds, const int64_t *starts, int k, int flags, adp_row *rows_out);

/* adp_adapter_front_revalidate: adp_adapter_front whose accepted reads are validated again.  The detector, its acceptance rule and
 * the side outputs are exactly adp_adapter_front's.  Every accepted read is validated with Boundaries.adapter_start = a0 + s and
 * the bounds its first validation took, read back from its row: the primary adapter end and polya_candidates (n_cand == -1: the list
 * is None); a row with ADP_ROW_POLYA_TRUNCATED is validated as the truncation look validated it (primary adapter end, the row's
 * polya_end, k = 1, Boundaries.polya_truncated).  A validation with success == 1 REPLACES the read's row: carried over are the
 * primary's poly(A) end, polya_candidates, the start-peak columns with start_peak_type and reserved_ bits 0-2; bits 3
 * (ADP_ROW_ADAPTER_FRONT) and 4 (ADP_ROW_REVALIDATED) are set.  A validation that fails leaves every byte of the read's row: the
 * trim is rejected (an opt-in, untuned pass never costs a read its pass status).  info_out[r][3] is 1 only where the row was
 * replaced.  full_len IS read here (host memory, or device memory with ADP_IN_DEVICE).
 *   reval_out int32 [n_reads, 2] (host): (-1, 0) the detector did not accept the read; (1, 0) validated again and replaced;
 *                                        (0, fail_code) validated again and failed with that code
 * `rows` is host memory.  A replaced row with more than ADP_MAX_OPEN_PORES open pores holds an offset into THIS call's open-pore
 * arena (adp_open_pores_arena); the other rows' open_pores_more are not touched.
 * adp_adapter_front_revalidate_i16: the same over raw rows, as adp_adapter_front_i16.
 * Refused before anything is launched (the handle stays usable): what adp_adapter_front(_i16) refuse; full_len or reval_out NULL,
 * min_adapter_len < 1 (an empty adapter slice has no median) -- ADP_ERR_INVALID; n_reads or m beyond the handle's --
 * ADP_ERR_CAPACITY; cfg.mvs_detect_overwrite and ADP_OUT_DEVICE (the call opens its own arena: offsets in untouched device rows would
 * be left pointing into the previous call's) -- ADP_ERR_UNSUPPORTED. */
int adp_adapter_front_revalidate(adp_handle *h, const float *sig, const int32_t *full_len, int n_reads, int m, adp_row *rows,
                                 const adp_adapter_front_args *args, int flags, int32_t *info_out, int64_t *shift_out,
                                 int64_t *cand_out, double *diff_out, int32_t *reval_out);
int adp_adapter_front_revalidate_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale,
                                     const float *offset, int n_reads, int m, adp_row *rows, const adp_adapter_front_args *args,
                                     int flags, int32_t *info_out, int64_t *shift_out, int64_t *cand_out, double *diff_out,
                                     int32_t *reval_out);

#endif /* ADAPTED_HIP_REVALIDATE_H */
