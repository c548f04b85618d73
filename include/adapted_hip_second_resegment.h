/* adapted_hip_second_resegment.h -- ADP_CNN_SECOND_RESEGMENT, a flag of adp_detect_cnn and adp_detect_cnn_i16: a read the CNN primary
 * fails AND whose LLR second opinion (ADP_CNN_SECOND_LLR) fails behind a first change point is segmented once more from that second
 * opinion's "poly(A) end" (an EXTENSION, off by default, UNTUNED: nothing of it has been validated on real data).  Part of the C ABI
 * of include/adapted_hip.h, which includes this file (inside its extern "C" block, behind adapted_hip_resegment.h): include that one.
 * The extension adds a flag and a selector of adp_debug_fetch -- no entry point and no row bit: adapted_amd/lib.py's
 * SECOND_RESEGMENT_PROTOTYPES is empty, and tests/test_cnn_second_resegment_cpu.py holds that against this header.
 *
 * Why: ADP_LLR_RESEGMENT (adapted_hip_resegment.h) recovers reads with a stall or a level step in front of their adapter, but only
 * under the LLR primary.  Under the CNN primary such a read fails the conv stack's candidates, and its second opinion -- the LLR
 * path's row on the same minibatch -- fails as the LLR primary's first validation does: the read is lost although the LLR primary
 * with ADP_LLR_RESEGMENT keeps it.  This flag puts the re-segmentation behind the second opinion.
 *
 * THE RULE, to the bit.  It applies to adp_detect_cnn(_i16) in ADP_LAYOUT_MINIBATCH with ADP_CNN_SECOND_LLR and
 * ADP_CNN_SECOND_RESEGMENT in `flags` and rows_out given, behind the second opinion's validation and merge, before the start-peak
 * overlay of ADP_WITH_START_PEAK is applied again and before anything else.  For every read r the second opinion selected (its row
 * failed on the CNN path, the short-read fallback included) let s be the row the second opinion's own validation made for it -- the
 * row adp_detect_llr delivers for r on that minibatch, which a call without this flag discards when it fails.  With
 * ds = cfg.downscale_factor, a1 = s's ADP_C_PRIMARY_ADAPTER_END and p1 = s's ADP_C_PRIMARY_POLYA_END:
 *   s.success == 1: the second opinion replaced the row; nothing more happens to the read.
 *   ELIGIBLE is otherwise a read whose minibatch has status ADP_MB_OK and whose s is no exception row (ADP_F_IS_EXCEPTION), holds a1
 *     (present) with a1 > 0 and holds p1 (present) with p1 > a1 -- the test of adapted_hip_resegment.h, read on s.
 *   SECOND SEGMENTATION, VALIDATION: those of adapted_hip_resegment.h with "the first row" read as s.  c = (p1 - cfg.min_obs_adapter)
 *     / ds; the trace on the read's own pooled signal, normalised with the median and MAD of its OWN minibatch as the second opinion's
 *     LLR run over all reads of the call computed them; p = detect_full_polya_trace_peak_with_spike(trace.signal); p2 = p * ds +
 *     cfg.min_obs_adapter if p > 0, else 0; validate_boundaries(signal[:full_len], Boundaries(adapter_start = a1, adapter_end = p1,
 *     polya_end = p2, polya_end_topk = [p2]), spc, full_len).
 *   MERGE.  A validation with success == 1 REPLACES the call's row r with every byte adp_detect_llr with ADP_LLR_RESEGMENT delivers
 *     for that read on that minibatch, except reserved_ = ADP_ROW_FROM_SECOND_LLR | ADP_ROW_RESEGMENTED | (s.fail_code <<
 *     ADP_ROW_FIRST_FAIL_SHIFT).  Nothing of the CNN path's row is kept; with ADP_WITH_START_PEAK the overlay is applied once more
 *     behind the merge, as behind the second opinion.
 *   Everything else -- a read that is not eligible, p2 == 0, a validation that fails -- keeps the CNN path's failing row byte for
 *     byte.  One level only.
 *   Without the flag every row of every call keeps the bytes it had before the flag existed, and adp_debug_fetch(h, 11, ...) keeps
 *     its meaning with or without it: its counts are the second opinion's alone.
 * The rows are the same bytes under grouped execution (ADP_CNN_GROUPS / ADP_CNN_LANES, ADP_GROUPS / ADP_LANES) and whatever
 * ADP_G2_WINDOW says.  The second rows' open-pore lists share the call's arena.  adp_detect_cnn_i16 runs the phase on the raw rows
 * (the subset kernels' int16 instantiations): its rows are those of calibrating first.
 * adp_debug_fetch(h, 26, int32[3], 12): of the last adp_detect_cnn(_i16) call -- eligible reads, reads whose second segmentation
 * found p2 > 0, rows replaced; (0, 0, 0) behind a call without the flag.
 * ADP_ERR_INVALID before anything is launched: the flag without ADP_CNN_SECOND_LLR, or without rows_out.
 * Refused before anything is launched, ADP_ERR_UNSUPPORTED with adp_last_error, the handle stays usable: the flag together with
 * ADP_FLAG_TRUNCATED (the truncation look's T2 validates from start 0 and would undo the row); cfg.mvs_detect_overwrite;
 * ADP_LAYOUT_SINGLE_READ; the flag in adp_detect_llr(_i16) and adp_detect_start_peak. */
#ifndef ADAPTED_HIP_SECOND_RESEGMENT_H
#define ADAPTED_HIP_SECOND_RESEGMENT_H

#define ADP_CNN_SECOND_RESEGMENT (1 << 23) /* adp_detect_cnn(_i16), with ADP_CNN_SECOND_LLR: re-segment reads the second opinion fails too */

#endif /* ADAPTED_HIP_SECOND_RESEGMENT_H */
