/* adapted_hip_csv.h -- the rows of one output file of `adapted detect` to that file's text (an EXTENSION: the reference writes its
 * CSV files with pandas on the host).  Part of the C ABI of include/adapted_hip.h, which includes this file (inside its extern "C"
 * block, behind its types and flags): include that one.  adapted_amd/lib.py restates this prototype in CSV_PROTOTYPES;
 * tests/test_native_csv_cpu.py holds that table against this header.
 *
 * adp_format_rows: rows adp_row [n] (host) are the rows of ONE file, detected_boundaries_<k>.csv (fail == 0) or failed_reads_<k>.csv
 * (fail != 0), in file order; primary 0 llr, 1 cnn, 2 start_peak names the *_adapter_end / *_polya_end columns (a row with
 * ADP_ROW_FROM_SECOND_LLR is named llr whatever it says).  The text is, byte for byte, what adapted_amd/output.py's
 * save_detected_boundaries writes for adapted_amd.lib.rows_to_results of the same rows -- pandas' DataFrame.round(3).to_csv, which
 * chooses every column's type from the whole file: that writer is the specification, and the rules it comes to are written out in
 * adapted_amd/csrc/csv_api.h.  n == 0 gives what it gives for no rows: a line break.
 *   ids, id_off [n + 1]: the read ids as UTF-8 bytes back to back, id i is ids[id_off[i] .. id_off[i + 1]); id_off[0] == 0.
 *   more, more_off [n + 1]: the open_pores lists of the rows that hold more than ADP_MAX_OPEN_PORES entries (a row keeps only the
 *   first ones), int64 back to back: row i's whole list is more[more_off[i] .. more_off[i + 1]), n_open_pores entries; every other
 *   row takes none (more_off[i + 1] == more_off[i]); more_off[0] == 0; more may be NULL where more_off[n] == 0.
 *   strings, str_off [n_str + 1]: the texts the rows' codes stand for, packed the same way, n_str == 69 entries: 0-15 the
 *   fail_reason of fail_code 0-15 (code 7 without the names of the failed MVS tests), 16-18 start_peak_open_pore_type 0-2, 19-34
 *   the llr_detect_log of a re-segmented row by the first row's code, 35-66 the names of the failed MVS tests joined with spaces by
 *   bits 0-4 of mvs_fail_mask, 67 and 68 the header line of the pass file and of the fail file with its line break.  The caller
 *   owns these texts so that they are stated once (adapted_amd/lib.py: csv_string_table); they are copied as they are.
 * Checked before anything is launched (ADP_ERR_INVALID; the handle stays usable): n >= 0, the offsets ascend from 0, fail_code in
 * [0, 15], start_peak_type in [0, 2], n_cand in [-1, ADP_MAX_CAND], n_open_pores >= -1 and, beyond ADP_MAX_OPEN_PORES, equal to the
 * row's entries of more.
 * Outputs, host memory: *len_out the text's length in bytes; text_out [text_cap] the text where *len_out <= text_cap -- else
 * NOTHING is written there: call again with a buffer of *len_out bytes --; *n_fallback_out the rows that hold a value outside the
 * bounds within which the text is known to be pandas' (a finite float64 value of magnitude >= 2^43; a finite value >= 2^14 in
 * a float32 column of a file where that column has no None; an integer column's value that is not finite or >= 2^62): such a
 * value is printed as an empty field, so a text with *n_fallback_out != 0 is NOT the file -- the caller writes that file with the
 * pandas writer.  The call completes before it returns. */
#ifndef ADAPTED_HIP_CSV_H
#define ADAPTED_HIP_CSV_H

int adp_format_rows(adp_handle *h, const adp_row *rows, int n, int fail, int primary, const void *ids, const int64_t *id_off,
                    const int64_t *more, const int64_t *more_off, const void *strings, const int32_t *str_off, int n_str,
                    void *text_out, uint64_t text_cap, uint64_t *len_out, int32_t *n_fallback_out);

#endif /* ADAPTED_HIP_CSV_H */
