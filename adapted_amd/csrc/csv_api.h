// csv_api.h -- the rows of ONE output file (detected_boundaries_<k>.csv / failed_reads_<k>.csv) to that file's text, byte for byte
// what adapted_amd/output.py's save_detected_boundaries writes for lib.rows_to_results of the same rows (an extension; the writer
// behind `detect --native_csv`).  Compiled in modules.hip only.  The specification is that writer: pandas picks a column's dtype
// from the whole file and the text depends on it, so a pass over the file's rows settles every column's state first.
//
//   k_csv_state   a thread per row: which columns hold a None in this row, under the views of lib.rows_to_results (an exception
//                 row, codes 9-14, carries nothing but its fail_reason; a row the truncation look replaced has no rna_preloaded_*;
//                 a row is named by ITS primary: a second-opinion row fills llr_*), OR-ed into one 64-bit word of the file.
//   k_csv_rows<W> a thread per row, one formatter (csv_row) for two passes: W = false adds up the row's bytes and says whether the
//                 row leaves the verified bounds; W = true writes them at the row's offset.  A formatter that is the same code in
//                 both passes cannot disagree with itself about a length.
//   k_csv_scan    one workgroup: the exclusive sum of the row lengths -> the offsets, the total behind them.
//
// Numbers (DataFrame.round(3).to_csv): a column without a None is int64 (plain integers), float64, or -- the three columns the
// reference keeps as numpy float32 scalars, lib._F32_COLS -- float32; with a None in the file an int column prints as float64
// ("4040.0") and a float32 column is widened and rounded in float64.  A float x prints as n / 1000 with n = rint(x * 1000) in the
// column's precision (one multiply, ties to even, not contracted), trailing zeros trimmed to one decimal, the sign x's ("-0.0");
// "inf" / "-inf"; nothing for NaN.  That decimal IS the shortest text that reads back as round(x, 3) while half a unit in the last
// place stays below 0.0005 and x * 1000 keeps integer precision: |x| < 2^43 in float64 (CSV_F64_BOUND), |x| < 2^14 in float32
// (CSV_F32_BOUND: x * 1000 < 2^24).  tests/test_native_csv_cpu.py holds both against pandas on a dense sample and the ties (the
// float32 bound is derived and sampled, not exhausted).  A finite value at or beyond its bound is not approximated: its row is
// counted (n_fallback) and the caller writes that file with pandas.
// Lists (polya_candidates, open_pores) are numpy int64 arrays in the frame and print as numpy's str(): the entries right-aligned to
// the widest, one space between, a line break and one space of indent where the next entry would pass column 74, and beyond 1000
// entries the first and the last three around "...".  Fields are quoted as csv.QUOTE_MINIMAL does (a comma, a quote or a line
// break inside).
#pragma once
#include <cstdint>

#include "adapted_hip.h"

#define CSV_F64_BOUND 8796093022208.0 // 2^43
#define CSV_F32_BOUND 16384.0f        // 2^14
#define CSV_INT_BOUND 4611686018427387904.0 // 2^62: an int column's value goes through int64
#define CSV_LIST_EDGE 3               // numpy's edgeitems
#define CSV_LIST_THRESHOLD 1000       // numpy's threshold: longer arrays are summarised
#define CSV_LIST_WIDTH 74             // numpy's linewidth 75 less the closing bracket
#define CSV_MAX_INLINE 16             // open_pores entries a row holds (ADP_MAX_OPEN_PORES)

// the packed string table of a call (adapted_amd/lib.py: csv_string_table builds it from FAIL_REASONS, START_PEAK_TYPES,
// first_fail_text and output.CSV_COLUMNS): entry k is str[off[k] .. off[k + 1])
#define CSV_S_FAIL 0    // 16: FAIL_REASONS[code] ("" for None)
#define CSV_S_SPT 16    // 3: START_PEAK_TYPES
#define CSV_S_RESEG 19  // 16: llr_detect_log of a re-segmented row by the first row's code
#define CSV_S_MVS 35    // 32: the MVS check's names joined by the bits 0-4 of mvs_fail_mask
#define CSV_S_HEAD 67   // 2: the header line of the pass file and of the fail file, line break included
#define CSV_N_STR 69

#define CSV_STATE_ALL 0x1fffffffffffull // 39 columns, then (adapter_end, polya_end) of the llr, cnn and start_peak names
#define CSV_HD __host__ __device__ static inline

struct CsvIn {
    const adp_row *rows; int n, fail, primary;
    const unsigned char *ids; const int64_t *id_off;     // read ids, [n + 1]
    const int64_t *more; const int64_t *more_off;        // the open_pores lists longer than a row holds, [n + 1]
    const unsigned char *str; const int32_t *str_off;    // the string table, [CSV_N_STR + 1]
};

// where a row's bytes go: W writes, else only `at` moves.  bad: the row cannot be printed identically
template <bool W> struct CsvSink {
    unsigned char *p; uint64_t at; bool bad;
    __host__ __device__ void put(unsigned char c) { if (W) p[at] = c; at++; }
    __host__ __device__ void put(const char *s) { while (*s) put((unsigned char)*s++); }
};

CSV_HD int csv_row_primary(const adp_row &r, int primary) { return (r.reserved_ & ADP_ROW_FROM_SECOND_LLR) ? 0 : primary; }

// the columns that hold a None in this row: bit c for col[c] (c != 28, 29), bit 39 + 2 * p + (c - 28) for col[28 / 29] under the
// names of primary p
CSV_HD uint64_t csv_absent(const adp_row &r, int primary)
{
    if (ADP_F_IS_EXCEPTION(r.fail_code)) return CSV_STATE_ALL;
    const uint64_t two = 3ull << 28;
    uint64_t a = ~r.present & ((1ull << ADP_NCOL) - 1) & ~two;
    if (r.reserved_ & ADP_ROW_POLYA_TRUNCATED) a |= 0x3full << 16;
    const int p = csv_row_primary(r, primary);
    for (int q = 0; q < 3; q++)
        for (int c = 0; c < 2; c++)
            if (q != p || !(r.present >> (28 + c) & 1)) a |= 1ull << (39 + 2 * q + c);
    return a;
}

template <bool W> CSV_HD void csv_uint(CsvSink<W> &o, uint64_t v)
{
    char d[20];
    int k = 0;
    do { d[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) o.put((unsigned char)d[--k]);
}
CSV_HD int csv_int_len(int64_t v)
{
    uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    int k = v < 0 ? 2 : 1;
    while (a >= 10) { a /= 10; k++; }
    return k;
}
template <bool W> CSV_HD void csv_int(CsvSink<W> &o, int64_t v, int width = 0)
{
    for (int s = csv_int_len(v); s < width; s++) o.put(' ');
    if (v < 0) o.put('-');
    csv_uint(o, v < 0 ? 0 - (uint64_t)v : (uint64_t)v);
}
// n thousandths behind x's sign: "q.r" with r's trailing zeros trimmed to one decimal
template <bool W> CSV_HD void csv_milli(CsvSink<W> &o, bool neg, uint64_t n)
{
    const unsigned r = (unsigned)(n % 1000);
    if (neg) o.put('-');
    csv_uint(o, n / 1000);
    o.put('.');
    o.put((unsigned char)('0' + r / 100));
    if (r % 100) o.put((unsigned char)('0' + r / 10 % 10));
    if (r % 10) o.put((unsigned char)('0' + r % 10));
}
template <bool W> CSV_HD void csv_f64(CsvSink<W> &o, double x)
{
    if (x != x) return;
    const double a = __builtin_fabs(x);
    const bool neg = __builtin_signbit(x);
    if (a == __builtin_inf()) { o.put(neg ? "-inf" : "inf"); return; }
    if (!(a < CSV_F64_BOUND)) { o.bad = true; return; }
    csv_milli(o, neg, (uint64_t)__builtin_rint(a * 1000.0));
}
template <bool W> CSV_HD void csv_f32(CsvSink<W> &o, float x)
{
    if (x != x) return;
    const float a = __builtin_fabsf(x);
    const bool neg = __builtin_signbit(x);
    if (a == __builtin_inff()) { o.put(neg ? "-inf" : "inf"); return; }
    if (!(a < CSV_F32_BOUND)) { o.bad = true; return; }
    csv_milli(o, neg, (uint64_t)__builtin_rintf(a * 1000.0f));
}

// lib._INT_COLS: 0-4, 9-11, 16, 17, 22, 24, 26, 28, 29, 38
CSV_HD bool csv_is_int_col(int c) { return ((0x1full | 7ull << 9 | 3ull << 16 | 1ull << 22 | 1ull << 24 | 1ull << 26 | 3ull << 28 | 1ull << 38) >> c) & 1; }
CSV_HD bool csv_is_f32_col(int c) { return c == 23 || c == 25 || c == 27; }  // lib._F32_COLS

// col[c] under the file's state of its column (`mixed`: the column holds a None somewhere in the file)
template <bool W> CSV_HD void csv_num(CsvSink<W> &o, const adp_row &r, int c, bool absent, bool mixed)
{
    if (absent) return;
    const double v = r.col[c];
    if (csv_is_int_col(c)) {
        if (!(__builtin_fabs(v) < CSV_INT_BOUND)) { o.bad = true; return; }
        if (mixed) csv_f64(o, (double)(int64_t)v);
        else csv_int(o, (int64_t)v);
    } else if (csv_is_f32_col(c) && !mixed) csv_f32(o, (float)v);
    else if (csv_is_f32_col(c)) csv_f64(o, (double)(float)v);
    else csv_f64(o, v);
}

// a list as numpy prints an int64 array.  at(k): its entry k
template <bool W, class At> CSV_HD bool csv_list_body(CsvSink<W> &o, At at, int64_t cnt)
{
    const bool summary = cnt > CSV_LIST_THRESHOLD;
    const int64_t words = summary ? 2 * CSV_LIST_EDGE + 1 : cnt;
    int width = 1;
    for (int64_t k = 0; k < words; k++) {
        if (summary && k == CSV_LIST_EDGE) continue;
        const int l = csv_int_len(at(summary && k > CSV_LIST_EDGE ? cnt - words + k : k));
        if (l > width) width = l;
    }
    bool wrapped = false, first = true;
    int line = 1;
    o.put('[');
    for (int64_t k = 0; k < words; k++) {
        const bool dots = summary && k == CSV_LIST_EDGE;
        const int wl = dots ? 3 : width;
        if (line + wl > CSV_LIST_WIDTH && line > 1) { o.put('\n'); o.put(' '); line = 1; first = true; wrapped = true; }
        if (!first) o.put(' ');
        if (dots) o.put("...");
        else csv_int(o, at(summary && k > CSV_LIST_EDGE ? cnt - words + k : k), width);
        line += wl + 1;
        first = false;
    }
    o.put(']');
    return wrapped;
}
template <bool W, class At> CSV_HD void csv_list(CsvSink<W> &o, At at, int64_t cnt)
{
    if (cnt < 0) return;
    CsvSink<false> dry{nullptr, 0, false};
    const bool quote = csv_list_body(dry, at, cnt); // (a line break inside: the only thing in a list that asks for quotes)
    if (quote) o.put('"');
    csv_list_body(o, at, cnt);
    if (quote) o.put('"');
}

// up to four pieces of text as ONE field, quoted as csv.QUOTE_MINIMAL does
#define CSV_PIECES 4
struct CsvText { const unsigned char *p[CSV_PIECES]; int64_t n[CSV_PIECES]; };
template <bool W> CSV_HD void csv_text(CsvSink<W> &o, const CsvText &t)
{
    bool quote = false;
    for (int k = 0; k < CSV_PIECES; k++)
        for (int64_t i = 0; i < t.n[k]; i++) {
            const unsigned char c = t.p[k][i];
            quote |= c == ',' || c == '"' || c == '\n' || c == '\r';
        }
    if (quote) o.put('"');
    for (int k = 0; k < CSV_PIECES; k++)
        for (int64_t i = 0; i < t.n[k]; i++) {
            if (t.p[k][i] == '"') o.put('"');
            o.put(t.p[k][i]);
        }
    if (quote) o.put('"');
}
CSV_HD void csv_entry(const CsvIn &in, int k, CsvText &t, int slot)
{
    t.p[slot] = in.str + in.str_off[k];
    t.n[slot] = in.str_off[k + 1] - in.str_off[k];
}

// row i of the file, line break included.  state: the file's columns that hold a None (k_csv_state)
template <bool W> CSV_HD void csv_row(CsvSink<W> &o, const CsvIn &in, int i, uint64_t state)
{
    const adp_row &r = in.rows[i];
    const uint64_t gone = csv_absent(r, in.primary);
    const bool exc = ADP_F_IS_EXCEPTION(r.fail_code);
    const int p = csv_row_primary(r, in.primary);
    auto num = [&](int c) { csv_num(o, r, c, gone >> c & 1, state >> c & 1); o.put(','); };
    { CsvText t{}; t.p[0] = in.ids + in.id_off[i]; t.n[0] = in.id_off[i + 1] - in.id_off[i]; csv_text(o, t); }
    o.put(',');
    for (int c = 0; c < 16; c++) num(c);
    if (!exc) {
        if (r.reserved_ & ADP_ROW_POLYA_TRUNCATED) o.put("True");
        else if ((r.reserved_ & ADP_ROW_TRUNC_LOOKED) && r.success) o.put("False");
    }
    o.put(',');
    if (!exc) { const int64_t *cand = r.cand; csv_list(o, [cand](int64_t k) { return cand[k]; }, r.n_cand); }
    o.put(',');
    for (int c = 16; c < 27; c++) num(c);
    if (!exc) { CsvText t{}; csv_entry(in, CSV_S_SPT + r.start_peak_type, t, 0); csv_text(o, t); }
    o.put(',');
    num(27);
    for (int q = 0; q < 3; q++)
        for (int c = 0; c < 2; c++) {
            const int bit = 39 + 2 * q + c;
            csv_num(o, r, 28 + c, gone >> bit & 1, state >> bit & 1);
            o.put(',');
        }
    o.put(",,,"); // llr_adapter_end_adjust, llr_polya_end_adjust, llr_trace_early_stop_pos: None on every path
    if (!exc) o.put("False");
    o.put(',');
    if (!exc) o.put((r.mvs_fail_mask & ADP_MVS_TO_EARLY_STOP) ? "True" : "False");
    o.put(',');
    num(38);
    for (int c = 30; c < 38; c++) num(c);
    if (!exc) {
        if (r.n_open_pores <= CSV_MAX_INLINE) { const int32_t *op = r.open_pores; csv_list(o, [op](int64_t k) { return (int64_t)op[k]; }, r.n_open_pores); }
        else { const int64_t *op = in.more + in.more_off[i]; csv_list(o, [op](int64_t k) { return op[k]; }, r.n_open_pores); }
    }
    o.put(',');
    if (!exc && p != 2 && (r.reserved_ & ADP_ROW_RESEGMENTED)) { // llr_detect_log
        CsvText t{};
        csv_entry(in, CSV_S_RESEG + ((r.reserved_ >> 6) & 15), t, 0);
        csv_text(o, t);
    }
    if (in.fail) {
        o.put(',');
        CsvText t{};
        csv_entry(in, CSV_S_FAIL + r.fail_code, t, 0);
        if (r.fail_code == 7) csv_entry(in, CSV_S_MVS + (r.mvs_fail_mask & 31), t, 1);
        if (!exc && p == 2 && r.fail_code != 0 && r.start_peak_type != 0) { // "<reason>+<type>"
            t.p[2] = (const unsigned char *)"+"; t.n[2] = 1;
            csv_entry(in, CSV_S_SPT + r.start_peak_type, t, 3);
        }
        csv_text(o, t);
    }
    o.put('\n');
}

#ifdef __HIPCC__
// a thread per row; state: one word, zero before
__global__ void __launch_bounds__(256) k_csv_state(CsvIn in, unsigned long long *state)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= in.n) return;
    const uint64_t a = csv_absent(in.rows[i], in.primary);
    if (a) atomicOr(state, (unsigned long long)a);
}

// a thread per row.  W = false: len [n] and n_bad (zero before) from the rows; W = true: the rows' bytes at text + off[i], inside
// text [cap] (a row that would pass it is left out: the caller sized the buffer from the same lengths)
template <bool W>
__global__ void __launch_bounds__(256) k_csv_rows(CsvIn in, const unsigned long long *state, uint32_t *len, unsigned int *n_bad,
                                                const uint64_t *off, unsigned char *text, uint64_t cap)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= in.n) return;
    if (W) {
        if (off[i] > cap || len[i] > cap - off[i]) return;
        CsvSink<true> o{text + off[i], 0, false};
        csv_row(o, in, i, (uint64_t)*state);
    } else {
        CsvSink<false> o{nullptr, 0, false};
        csv_row(o, in, i, (uint64_t)*state);
        len[i] = (uint32_t)o.at;
        if (o.bad) atomicAdd(n_bad, 1u);
    }
}

// one workgroup of 256: off [n + 1], the exclusive sum of len [n]
__global__ void __launch_bounds__(256) k_csv_scan(const uint32_t *__restrict__ len, int n, uint64_t *__restrict__ off)
{
    __shared__ __attribute__((aligned(16))) uint64_t part[256];
    const int t = (int)threadIdx.x, chunk = (n + 255) / 256;
    const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    uint64_t s = 0;
    for (int i = lo; i < hi; i++) s += len[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        uint64_t run = 0;
        for (int k = 0; k < 256; k++) { const uint64_t v = part[k]; part[k] = run; run += v; }
        off[n] = run;
    }
    __syncthreads();
    uint64_t run = part[t];
    for (int i = lo; i < hi; i++) { off[i] = run; run += len[i]; }
}
#endif
