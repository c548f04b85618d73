/* adapted_hip_resegment.h -- ADP_LLR_RESEGMENT, a flag of adp_detect_llr: reads the LLR primary fails are segmented once more behind
 * their first change point (an EXTENSION, off by default, UNTUNED: nothing of it has been validated on real data).  Part of the C ABI
 * of include/adapted_hip.h, which includes this file (inside its extern "C" block, behind its types and flags): include that one.
 * The extension adds a flag, bits of adp_row.reserved_ and a selector of adp_debug_fetch -- no entry point: adapted_amd/lib.py's
 * RESEGMENT_PROTOTYPES is empty, and tests/test_resegment_cpu.py holds that against this header.
 *
 * Why: the LLR primary takes the first qualifying peak of the pass-1 trace as the adapter end (single change-point detection,
 * adapted/detect/combined.py:184).  When something sits in front of the adapter -- a stall, a level step, a long start peak -- the
 * strongest change point of the read is the end of that front stretch, pass 2 reports the true adapter end as the "poly(A) end", the
 * validation rejects the pair and the read is lost.  One more segmentation step from that "poly(A) end" finds the boundaries; whether
 * they are accepted stays with the reference's validate_boundaries.
 *
 * THE RULE, to the bit.  It applies to adp_detect_llr in ADP_LAYOUT_MINIBATCH with ADP_LLR_RESEGMENT in `flags` and rows_out given,
 * after the first validation of every read of the call (and the start-peak overlay of ADP_WITH_START_PEAK) and before anything else.
 * With ds = cfg.downscale_factor, a1 = the row's ADP_C_PRIMARY_ADAPTER_END and p1 = its ADP_C_PRIMARY_POLYA_END:
 *   ELIGIBLE is a read whose minibatch has status ADP_MB_OK and whose row has success == 0, is no exception row
 *     (ADP_F_IS_EXCEPTION), holds a1 (present) with a1 > 0 and holds p1 (present) with p1 > a1.  Reads that fail with "No adapter
 *     detected (primary)" or "No polya detected (primary)" are therefore never eligible.
 *   SECOND SEGMENTATION.  c = (p1 - cfg.min_obs_adapter) / ds (exact: p1 was made as index * ds + min_obs_adapter).  The trace is the
 *     reference's calc_adapter_trace(s_, offset_head = 1, offset_tail = 1, trace_start = c, c = trace.c, c2 = trace.c2) on the read's
 *     own pooled signal s_ -- normalised with the median and MAD of the read's OWN minibatch, pooled as numpy pools it -- and on that
 *     signal's sequential float64 cumulative sums: the bits of the first pass.  p = detect_full_polya_trace_peak_with_spike(
 *     trace.signal); p2 = p * ds + cfg.min_obs_adapter if p > 0, else 0.
 *   VALIDATION.  p2 == 0: nothing more happens to the read (the reference would fail with "No polya detected (primary)").  Otherwise
 *     validate_boundaries(signal[:full_len], Boundaries(adapter_start = a1, adapter_end = p1, polya_end = p2, polya_end_topk =
 *     [p2]), spc, full_len), as adp_validate_candidates_from computes it.
 *   MERGE.  A validation with success == 1 REPLACES the read's row: the primary columns become (p1, p2), polya_candidates [p2];
 *     the five start-peak columns (with their present bits) and start_peak_type are carried over from the first row.  reserved_ of
 *     such a row: ADP_ROW_RESEGMENTED | (the first row's fail_code << ADP_ROW_FIRST_FAIL_SHIFT) -- bits 6-9 hold the code, which is
 *     at most 15.  A validation that fails leaves the first row byte for byte.  One level only: a second failure ends it.
 *   Without the flag every row of every call keeps the bytes it had before the flag existed.
 * The rows are the same bytes under grouped execution (ADP_GROUPS / ADP_LANES) and whatever ADP_G2_WINDOW says.  The second rows'
 * open-pore lists share the call's arena.
 * adp_debug_fetch(h, 25, int32[3], 12): of the last adp_detect_llr call -- eligible reads, reads whose second segmentation found
 * p2 > 0, rows replaced; (0, 0, 0) behind a call without the flag.
 * Refused before anything is launched, ADP_ERR_UNSUPPORTED with adp_last_error: cfg.mvs_detect_overwrite; ADP_LAYOUT_SINGLE_READ;
 * the flag in adp_detect_llr_i16, adp_detect_cnn(_i16) and adp_detect_start_peak; the flag together with ADP_FLAG_TRUNCATED (the
 * truncation look's T2 validates from start 0 and would undo the row). */
#ifndef ADAPTED_HIP_RESEGMENT_H
#define ADAPTED_HIP_RESEGMENT_H

#define ADP_LLR_RESEGMENT (1 << 21) /* adp_detect_llr: re-segment failed reads behind their first change point */

/* adp_row.reserved_ bit 5: the row is the validation of the second segmentation; bits 6-9: the fail_code of the row it replaced */
#define ADP_ROW_RESEGMENTED 32
#define ADP_ROW_FIRST_FAIL_SHIFT 6
#define ADP_ROW_FIRST_FAIL_MASK (15 << ADP_ROW_FIRST_FAIL_SHIFT)

#endif /* ADAPTED_HIP_RESEGMENT_H */
