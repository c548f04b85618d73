// modules.hip -- the reference-module drop-ins (adp_c_llr_*, adp_llr_*, adp_mvs_*, the signal statistics, the start peak, the adapter start, the event segmentation, the event fingerprints, the template building, the clustering of fingerprints, the adapter-front post-pass and the CSV text of a file's rows): their kernels and entry points, a
// translation unit of their own, so that nothing here can move the code the compiler makes for the detect path's kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "handle.h"
#include "trace_api.h"
#include "llr_detect_api.h"
#include "trace_peaks_api.h"
#include "mvs_api.h"
#include "sigstats_api.h"
#include "startmods_api.h"
#include "events_api.h"
#include "fingerprint_api.h"
#include "dtw_align_api.h"
#include "dtw_cluster_api.h"
#include "dtw_knn_api.h"
#include "adapter_front.h"
#include "csv_api.h"

// ---- workspace, staging and per-read checks of the entry points

// copies on the handle's stream between a host array and a workspace piece (handle.h: ws_carve): the whole piece, or its first
// `count` elements
template <class T> static int h2d(adp_handle *h, Piece<T> dst, const void *src, size_t count)
{
    if (count > dst.n) { g_err = "internal error: a copy past its workspace piece"; return ADP_ERR_INVALID; }
    HIPCHK(hipMemcpyAsync(dst.p, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return ADP_OK;
}
template <class T> static int d2h(adp_handle *h, void *dst, Piece<T> src, size_t count)
{
    if (count > src.n) { g_err = "internal error: a copy past its workspace piece"; return ADP_ERR_INVALID; }
    HIPCHK(hipMemcpyAsync(dst, src.p, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    return ADP_OK;
}
template <class T> static int h2d(adp_handle *h, Piece<T> dst, const void *src) { return h2d(h, dst, src, dst.n); }
template <class T> static int d2h(adp_handle *h, void *dst, Piece<T> src) { return d2h(h, dst, src, src.n); }
template <class T> static int zero(adp_handle *h, Piece<T> piece) { HIPCHK(hipMemsetAsync(piece.p, 0, piece.bytes(), h->stream)); return ADP_OK; }

// the device pointer of an input that is device memory with ADP_IN_DEVICE, else host memory: then copied to `piece` (a
// workspace piece taken for it only in that case; of bytes where the input's element type is a flag's)
template <class S, class T> static int stage_in(adp_handle *h, int flags, const S *src, Piece<T> piece, const S **dev)
{
    if (flags & ADP_IN_DEVICE) { *dev = src; return ADP_OK; }
    *dev = piece.p;
    return h2d(h, piece, src);
}

// a signal whose element type is a flag's: fn(the typed pointer), for float64 with `f64`, else float32; elem_t names the type there
template <class F> static auto by_elem(bool f64, const void *sig, F &&fn) { return f64 ? fn((const double *)sig) : fn((const float *)sig); }
template <class P> using elem_t = std::remove_cv_t<std::remove_pointer_t<P>>;

// the samples of a segmentation call: the signals (host, or device with ADP_IN_DEVICE) and their bytes; the element type --
// float32, float64 with `f64`, raw int16 with `i16`: then a calibration per segment, float32 [n_seg] each, where `sig` is
struct EvIn { const void *sig; size_t bytes; bool f64, i16; const float *scale, *offset; };
// fn(the kernels' sample source, events_api.h) of the staged input
template <class F> static auto by_source(const EvIn &in, const void *ds, const float *dscale, const float *doffset, F &&fn)
{
    if (in.i16) return fn(EvI16{(const int16_t *)ds, dscale, doffset});
    return in.f64 ? fn(EvPlain<double>{(const double *)ds}) : fn(EvPlain<float>{(const float *)ds});
}

// a byte budget in MiB: `dflt`, or what the environment holds under `name` (`value`: its getenv, read per call)
static int scratch_mib(const char *name, const char *value, long long dflt, long long *mib)
{
    *mib = value ? atoll(value) : dflt;
    if (value && (*mib < 1 || *mib > (1 << 20))) { g_err = std::string(name) + " must lie in [1, 2^20]"; return ADP_ERR_INVALID; }
    return ADP_OK;
}

// the DTW kernels' register tile for rows of up to E <= FP_EMAX values: fn(C as an integral_constant), the least C of 1, 2, 4, 8
// with C * 64 >= E; dtw_width: that C as a number
template <class F> static auto by_width(int E, F &&fn)
{
    const int C = (E + 63) / 64;
    if (C <= 1) return fn(std::integral_constant<int, 1>());
    if (C <= 2) return fn(std::integral_constant<int, 2>());
    if (C <= 4) return fn(std::integral_constant<int, 4>());
    return fn(std::integral_constant<int, 8>());
}
static int dtw_width(int E) { return by_width(E, [](auto c) { return (int)decltype(c)::value; }); }

// a host table t [rows, E] with its counts, as the DTW calls take their templates / references: 1 <= count <= E and finite values
// inside the count, refused in the caller's nouns; -> the greatest count (cmax may be null)
static int table_check(const double *t, const int32_t *count, int rows, int E, const char *count_name, const char *E_name,
                       const char *noun, int *cmax)
{
    int most = 1;
    for (int k = 0; k < rows; k++) {
        if (count[k] < 1 || count[k] > E) {
            g_err = std::string("need 1 <= ") + count_name + " <= " + E_name + " for every " + noun;
            return ADP_ERR_INVALID;
        }
        for (int j = 0; j < count[k]; j++)
            if (!std::isfinite(t[(size_t)k * E + j])) { g_err = std::string(noun) + " values inside their count must be finite"; return ADP_ERR_INVALID; }
        if (count[k] > most) most = count[k];
    }
    if (cmax) *cmax = most;
    return ADP_OK;
}

// what adp_dtw_assign, adp_dtw_align and adp_dba_step check of their sizes and templates; -> the longest template
static int dtw_templates_check(int Eq, const double *t, const int32_t *t_count, int nt, int Et, int band, int *mmax)
{
    if (Eq < 1 || Eq > FP_EMAX || Et < 1 || Et > FP_EMAX) { g_err = "Eq and Et must lie in [1, 512]"; return ADP_ERR_INVALID; }
    if (nt < 1 || nt > DTW_NT_MAX) { g_err = "nt must lie in [1, 4096]"; return ADP_ERR_INVALID; }
    if (band < 0) { g_err = "band must be >= 0"; return ADP_ERR_INVALID; }
    return table_check(t, t_count, nt, Et, "t_count", "Et", "template", mmax);
}

// the rows of one batch of `n` rows of `row_bytes` each within a budget of `mib` MiB: at least one; with wgs_per_row > 0 no more
// than keep a grid of that many workgroups per row within 0x7fffffff
static size_t batch_rows(long long mib, size_t row_bytes, size_t n, size_t wgs_per_row)
{
    size_t rows = ((size_t)mib << 20) / row_bytes;
    if (rows < 1) rows = 1;
    if (rows > n) rows = n;
    if (wgs_per_row && rows > (size_t)0x7fffffff / wgs_per_row) rows = (size_t)0x7fffffff / wgs_per_row;
    return rows;
}

// the per-read checks (host arrays of n entries): lo <= a <= hi; 0 <= len <= L; 0 <= start <= end <= len; positions in [0, 2^40]
template <class T> static bool all_in(const T *a, int n, T lo, T hi)
{
    for (int r = 0; r < n; r++) if (a[r] < lo || a[r] > hi) return false;
    return true;
}
static bool lens_ok(const int32_t *len, int n, int L) { return all_in<int32_t>(len, n, 0, L); }
static bool spans_ok(const int32_t *start, const int32_t *end, const int32_t *len, int n)
{
    for (int r = 0; r < n; r++) if (start[r] < 0 || start[r] > end[r] || end[r] > len[r]) return false;
    return true;
}
static bool positions_ok(const int64_t *p, int n) { return all_in<int64_t>(p, n, 0, (int64_t)1 << 40); }

// what the row modules start with, checks done: signals float32 / float64 [n_reads, L] (ADP_MVS_F64) and a length per read
struct RowsIn { bool f64; size_t esz; Piece<char> s_sig; Piece<int32_t> dlen; const void *ds; };
// begin_call; the pieces -- the staged signal, dlen, then the call's own (`more(Carve &)`, with in.f64 / in.esz set) --; the two in
template <class F>
static int rows_begin(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, int flags, RowsIn &in, F &&more)
{
    RCCHK(begin_call(h));
    in.f64 = (flags & ADP_MVS_F64) != 0;
    in.esz = in.f64 ? 8 : 4;
    RCCHK(ws_carve(h, [&](Carve &w) {
        in.s_sig = w.take<char>((size_t)L * in.esz * n_reads, !(flags & ADP_IN_DEVICE));
        in.dlen = w.take<int32_t>(n_reads);
        more(w);
    }));
    RCCHK(stage_in(h, flags, sig, in.s_sig, &in.ds));
    return h2d(h, in.dlen, len);
}

// ---- the signal statistics modules (sigstats_api.h)

// the segments of a call, checked: rows in [0, n_reads), positions <= 2^40
static int seg_check(const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg)
{
    if (!sig || !len || !segs || n_reads < 1 || L < 1 || n_seg < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!lens_ok(len, n_reads, L)) { g_err = "need 0 <= len <= L for every read"; return ADP_ERR_INVALID; }
    const int64_t pmax = (int64_t)1 << 40;
    for (int g = 0; g < n_seg; g++) {
        if (segs[g].row < 0 || segs[g].row >= n_reads) { g_err = "need 0 <= row < n_reads for every segment"; return ADP_ERR_INVALID; }
        if (segs[g].start > pmax || segs[g].end > pmax) { g_err = "positions must lie in [0, 2^40]"; return ADP_ERR_INVALID; }
    }
    return ADP_OK;
}

// what the segment modules start with, checks done (seg_check, then their own): the rows (rows_begin) and the segments behind them
struct SegIn : RowsIn { Piece<SsSeg> dsegs; };
template <class F>
static int seg_begin(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg, int flags,
                     SegIn &in, F &&more)
{
    RCCHK(rows_begin(h, sig, len, n_reads, L, flags, in, [&](Carve &w) { in.dsegs = w.take<SsSeg>(n_seg); more(w); }));
    return h2d(h, in.dsegs, segs);
}

// median and MAD on the device -> dmm [rows, 2] ([1, 2] with ADP_SS_WHOLE; then dlen[0] holds n_reads * L)
template <class T>
static int ss_med_mad_dev(adp_handle *h, const T *ds, const int32_t *dlen, int n_reads, int L, int flags, double *dmm, Piece<SsPop> dst,
                           Piece<uint32_t> dhist)
{
    const int skip = (flags & ADP_SS_NANSKIP) != 0;
    if (!(flags & ADP_SS_WHOLE)) {
        Scope s(h, "k_row_med_mad");
        hipLaunchKernelGGL(k_row_med_mad<T>, dim3(n_reads), dim3(SS_BLOCK), 0, h->stream, ds, dlen, n_reads, (long long)L, skip, dmm);
        return ADP_OK;
    }
    const long long N = (long long)n_reads * L;
    const bool grid = (flags & ADP_SS_FORCE_GRID) || (!(flags & ADP_SS_FORCE_WAVE) && N > ADP_SS_GRID_MIN);
    if (!grid) {
        Scope s(h, "k_row_med_mad");
        hipLaunchKernelGGL(k_row_med_mad<T>, dim3(1), dim3(SS_BLOCK), 0, h->stream, ds, dlen, 1, N, skip, dmm);
        return ADP_OK;
    }
    long long nb = (N + 4095) / 4096;
    if (nb > (long long)h->n_cu * 8) nb = (long long)h->n_cu * 8;
    RCCHK(zero(h, dhist));
    for (int sel = 0; sel < 2; sel++) {
        RCCHK(zero(h, dst));
        for (int pass = 0; pass < (int)sizeof(typename SsKey<T>::type); pass++) {
            { Scope s(h, "k_pop_hist");
              hipLaunchKernelGGL(k_pop_hist<T>, dim3((unsigned)nb), dim3(SS_POP_BLOCK), 0, h->stream, ds, N, sel ? dmm : (const double *)nullptr, pass, skip, dst, dhist); }
            { Scope s(h, "k_pop_pick");
              hipLaunchKernelGGL(k_pop_pick<T>, dim3(1), dim3(64), 0, h->stream, pass, skip, dst, dhist, dmm + sel); }
        }
    }
    return ADP_OK;
}

extern "C" {

// c_llr_trace / c_llr_trace_gains / _gains for a batch of float64 signals (trace_api.h)
int adp_c_llr_trace(adp_handle *h, const double *raw, const int32_t *len, const int32_t *start, const int32_t *end, int n_reads,
                    int L, const adp_trace_args *args, int flags, double *gain_out, double *c_io, double *c2_io)
{
    if (!h || !len || !start || !end || !args || !gain_out || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    const bool from_sums = (flags & ADP_TRACE_FROM_SUMS) != 0, in_dev = (flags & ADP_IN_DEVICE) != 0, out_dev = (flags & ADP_OUT_DEVICE) != 0;
    if (from_sums ? (!c_io || !c2_io) : !raw) { g_err = "bad argument: no input signal / sums"; return ADP_ERR_INVALID; }
    if (!from_sums && ((c_io == nullptr) != (c2_io == nullptr))) { g_err = "bad argument: c and c2 go together"; return ADP_ERR_INVALID; }
    const adp_trace_args &a = *args;
    if (a.stride < 1 || a.min_obs < 0 || a.border_trim < 0) { g_err = "stride must be >= 1, offsets >= 0"; return ADP_ERR_INVALID; }
    if (a.polya_early_stopping > 0) {
        if (a.adapter_early_stop_stride < 1 || a.polya_early_stop_stride < 1 || a.adapter_early_stop_window < 0 || a.polya_early_stop_window < 0) { g_err = "early-stop windows / strides out of range"; return ADP_ERR_INVALID; }
        if (a.adapter_early_stop_stride % a.stride || a.polya_early_stop_stride % a.stride) { g_err = "early-stop stride is not a multiple of stride (the reference asserts, _c_llr.pyx:137-138)"; return ADP_ERR_INVALID; }
    } else if (a.adapter_early_stopping > 0) {
        if (a.adapter_early_stop_stride < 1 || a.adapter_early_stop_window < 0) { g_err = "early-stop window / stride out of range"; return ADP_ERR_INVALID; }
        if (a.adapter_early_stop_stride % a.stride) { g_err = "early-stop stride is not a multiple of stride (the reference asserts, _c_llr.pyx:102)"; return ADP_ERR_INVALID; }
    }
    if (!lens_ok(len, n_reads, L) || !spans_ok(start, end, len, n_reads)) { g_err = "need 0 <= start <= end <= len <= L for every read"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const size_t cells = (size_t)L * n_reads;
    // the sums a raw call computes go to the caller's arrays when those are device outputs, else to the workspace
    const bool own_c = !from_sums && !(c_io && out_dev);
    Piece<int32_t> dlen, dstart, dend; Piece<double> s_raw, s_c, s_c2, w_c, w_c2, w_g;
    RCCHK(ws_carve(h, [&](Carve &w) {
        dlen = w.take<int32_t>(n_reads); dstart = w.take<int32_t>(n_reads); dend = w.take<int32_t>(n_reads);
        s_raw = w.take<double>(cells, !from_sums && !in_dev);
        s_c = w.take<double>(cells, from_sums && !in_dev); s_c2 = w.take<double>(cells, from_sums && !in_dev);
        w_c = w.take<double>(cells, own_c); w_c2 = w.take<double>(cells, own_c);
        w_g = w.take<double>(cells, !out_dev);
    }));
    RCCHK(h2d(h, dlen, len)); RCCHK(h2d(h, dstart, start)); RCCHK(h2d(h, dend, end));
    const double *dc, *dc2;
    if (from_sums) {
        RCCHK(stage_in<double>(h, flags, c_io, s_c, &dc));
        RCCHK(stage_in<double>(h, flags, c2_io, s_c2, &dc2));
    } else {
        const double *draw;
        RCCHK(stage_in(h, flags, raw, s_raw, &draw));
        double *wc = own_c ? w_c.p : c_io, *wc2 = own_c ? w_c2.p : c2_io;
        { Scope s(h, "k_trace_cumsum");
          hipLaunchKernelGGL(k_trace_cumsum<double>, dim3(n_reads), dim3(64), 0, h->stream, draw, dlen, L, n_reads, wc, wc2); }
        dc = wc; dc2 = wc2;
    }
    double *dg = out_dev ? gain_out : w_g.p;
    TraceArgs ta = {a.min_obs, a.border_trim, a.stride, a.adapter_early_stopping, a.adapter_early_stop_window, a.adapter_early_stop_stride,
                    a.polya_early_stopping, a.polya_early_stop_window, a.polya_early_stop_stride};
    { Scope s(h, "k_trace_gains");
      hipLaunchKernelGGL(k_trace_gains, dim3(n_reads), dim3(64), 0, h->stream, dc, dc2, dlen, dstart, dend, L, ta, dg); }
    HIPCHK(hipGetLastError());
    if (!out_dev) { // (the sums of a raw call are then the workspace's: own_c)
        RCCHK(d2h(h, gain_out, w_g));
        if (!from_sums && c_io) { RCCHK(d2h(h, c_io, w_c)); RCCHK(d2h(h, c2_io, w_c2)); }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// the split searches of one level: chunk winners, then per segment (llr_detect_api.h)
static void cd_splits(adp_handle *h, const double *dc, const double *dc2, int L, const CdSeg *segs, int n_seg, double *part_g,
                      int32_t *part_x, int32_t *st_x, double *st_g)
{
    const int nck = (L + CD_CHUNK - 1) / CD_CHUNK;
    { Scope s(h, "k_split_part");
      hipLaunchKernelGGL(k_split_part, dim3(n_seg, nck), dim3(CD_BLOCK), 0, h->stream, dc, dc2, L, segs, nck, part_g, part_x); }
    { Scope s(h, "k_split_reduce");
      hipLaunchKernelGGL(k_split_reduce, dim3(n_seg), dim3(64), 0, h->stream, segs, nck, part_g, part_x, st_x, st_g); }
}

// _best_split (_c_llr.pyx:40-64) for a batch of rows of given sums: one segment per row
int adp_c_llr_best_split(adp_handle *h, const double *c, const double *c2, const int32_t *len, const int32_t *start, const int32_t *end,
                         const int32_t *offset_head, const int32_t *offset_tail, int n_reads, int L, int flags, int64_t *x_out, double *gain_out)
{
    if (!h || !c || !c2 || !len || !start || !end || !offset_head || !offset_tail || !x_out || !gain_out || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!lens_ok(len, n_reads, L) || !spans_ok(start, end, len, n_reads) || !all_in(offset_head, n_reads, 0, INT32_MAX) ||
        !all_in(offset_tail, n_reads, 0, INT32_MAX)) {
        g_err = "need 0 <= start <= end <= len <= L and offsets >= 0 for every row"; return ADP_ERR_INVALID;
    }
    const bool in_dev = (flags & ADP_IN_DEVICE) != 0;
    RCCHK(begin_call(h));
    const size_t cells = (size_t)L * n_reads, nck = (size_t)(L + CD_CHUNK - 1) / CD_CHUNK;
    Piece<double> s_c, s_c2, part_g, st_g; Piece<int32_t> part_x, st_x; Piece<CdSeg> dsegs;
    RCCHK(ws_carve(h, [&](Carve &w) {
        dsegs = w.take<CdSeg>(n_reads);
        part_g = w.take<double>(n_reads * nck); part_x = w.take<int32_t>(n_reads * nck);
        st_x = w.take<int32_t>(n_reads); st_g = w.take<double>(n_reads);
        s_c = w.take<double>(cells, !in_dev); s_c2 = w.take<double>(cells, !in_dev);
    }));
    const double *dc, *dc2;
    RCCHK(stage_in(h, flags, c, s_c, &dc));
    RCCHK(stage_in(h, flags, c2, s_c2, &dc2));
    std::vector<CdSeg> segs(n_reads);
    for (int r = 0; r < n_reads; r++) {
        long lo = (long)start[r] + offset_head[r], hi = (long)end[r] - offset_tail[r];
        if (lo > end[r]) lo = end[r];
        if (hi < lo) hi = lo; // (an empty range: the reference's loop does not run)
        segs[r] = CdSeg{r, start[r], end[r], (int32_t)lo, (int32_t)hi, r};
    }
    RCCHK(h2d(h, dsegs, segs.data()));
    cd_splits(h, dc, dc2, L, dsegs, n_reads, part_g, part_x, st_x, st_g);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> x(n_reads);
    RCCHK(d2h(h, x.data(), st_x));
    RCCHK(d2h(h, gain_out, st_g));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int r = 0; r < n_reads; r++) x_out[r] = x[r];
    return ADP_OK;
}

// c_llr_detect_adapter (_c_llr.pyx:239-287) / c_llr_detect_adapter_polya (:290-365) for a batch (llr_detect_api.h)
int adp_c_llr_detect(adp_handle *h, const void *raw, const int32_t *len, int n_reads, int L, int32_t min_obs_adapter, int32_t border_trim,
                     int32_t min_obs_polya, int flags, int64_t *rows_out, int64_t *splits_out, double *stats_out)
{
    if (!h || !raw || !len || !rows_out || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (min_obs_adapter < 0 || border_trim < 0 || min_obs_polya < 0) { g_err = "offsets must be >= 0"; return ADP_ERR_INVALID; }
    if (!all_in(len, n_reads, 1, L)) { g_err = "need 1 <= len <= L for every read"; return ADP_ERR_INVALID; }
    const bool in_dev = (flags & ADP_IN_DEVICE) != 0, f32 = (flags & ADP_CLLR_F32) != 0, polya = (flags & ADP_CLLR_POLYA) != 0;
    RCCHK(begin_call(h));
    const size_t n = n_reads, cells = (size_t)L * n, esz = f32 ? 4 : 8, nck = (size_t)(L + CD_CHUNK - 1) / CD_CHUNK;
    // the sums, the staged signal; segments (2 per read), chunk winners, the per-read state
    Piece<double> dc, dc2, part_g, st_g, med; Piece<int32_t> part_x, st_x, res, dlen; Piece<CdSeg> segs, psegs; Piece<char> s_raw;
    RCCHK(ws_carve(h, [&](Carve &w) {
        dc = w.take<double>(cells); dc2 = w.take<double>(cells); s_raw = w.take<char>(cells * esz, !in_dev);
        segs = w.take<CdSeg>(2 * n); psegs = w.take<CdSeg>(n);
        part_g = w.take<double>(2 * n * nck); part_x = w.take<int32_t>(2 * n * nck);
        st_x = w.take<int32_t>(4 * n); st_g = w.take<double>(4 * n); med = w.take<double>(4 * n); res = w.take<int32_t>(4 * n);
        dlen = w.take<int32_t>(n);
    }));
    const void *draw;
    RCCHK(stage_in(h, flags, raw, s_raw, &draw));
    RCCHK(h2d(h, dlen, len));
    const CdArgs a = {min_obs_adapter, border_trim, min_obs_polya, polya ? 1 : 0};
    const int rb = (n_reads + 255) / 256;
    { Scope s(h, "k_trace_cumsum");
      by_elem(!f32, draw, [&](auto sig) { hipLaunchKernelGGL(k_trace_cumsum<elem_t<decltype(sig)>>, dim3(n_reads), dim3(64), 0, h->stream, sig, dlen, L, n_reads, dc, dc2); }); }
    { Scope s(h, "k_cd_plan");
      hipLaunchKernelGGL(k_cd_plan, dim3(rb), dim3(256), 0, h->stream, 0, dlen, n_reads, a, st_x, segs); }
    cd_splits(h, dc, dc2, L, segs, n_reads, part_g, part_x, st_x, st_g);
    { Scope s(h, "k_cd_plan");
      hipLaunchKernelGGL(k_cd_plan, dim3(rb), dim3(256), 0, h->stream, 1, dlen, n_reads, a, st_x, segs); }
    cd_splits(h, dc, dc2, L, segs, 2 * n_reads, part_g, part_x, st_x, st_g);
    { Scope s(h, "k_cd_medians");
      by_elem(!f32, draw, [&](auto sig) { hipLaunchKernelGGL(k_cd_medians<elem_t<decltype(sig)>>, dim3(n_reads), dim3(CD_MED_BLOCK), 0, h->stream, sig, dlen, L, a, st_x, st_g, res, med, psegs); }); }
    if (polya) {
        cd_splits(h, dc, dc2, L, psegs, n_reads, part_g, part_x, st_x, st_g);
        { Scope s(h, "k_cd_finish");
          hipLaunchKernelGGL(k_cd_finish, dim3(rb), dim3(256), 0, h->stream, n_reads, st_x, res); }
    }
    HIPCHK(hipGetLastError());
    std::vector<int32_t> hres(n * 4), sx;
    std::vector<double> sg, hmed;
    RCCHK(d2h(h, hres.data(), res));
    if (splits_out) { sx.resize(n * 4); RCCHK(d2h(h, sx.data(), st_x)); }
    if (stats_out) {
        sg.resize(n * 4); hmed.resize(n * 4);
        RCCHK(d2h(h, sg.data(), st_g));
        RCCHK(d2h(h, hmed.data(), med));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < hres.size(); i++) rows_out[i] = hres[i];
    for (int r = 0; r < n_reads; r++) {
        const bool searched = hres[r * 4 + 3] == 3 && hres[r * 4 + 1] != 0;
        if (splits_out) for (int k = 0; k < 4; k++) splits_out[r * 4 + k] = (k == 3 && !searched) ? -1 : sx[r * 4 + k];
        if (stats_out) for (int k = 0; k < 4; k++) {
            stats_out[r * 8 + k] = (k == 3 && !searched) ? 0.0 : sg[r * 4 + k];
            stats_out[r * 8 + 4 + k] = hmed[r * 4 + k];
        }
    }
    return ADP_OK;
}

// ---- the reference's Python LLR module (adapted/detect/llr.py) on device traces (trace_peaks_api.h)

// block summaries of the trace rows: nsum blocks of SUMBLK points per row
static void trace_blocksum(adp_handle *h, const double *dtr, const int32_t *dlen, int n_reads, int L, int nsum, int sanitize, double *bx, double *bn)
{
    Scope s(h, "k_trace_blocksum");
    hipLaunchKernelGGL(k_trace_blocksum, dim3(n_reads), dim3(64), 0, h->stream, dtr, dlen, L, nsum, sanitize, bx, bn);
}

int adp_llr_trace_bounds(adp_handle *h, double *trace, const int32_t *len, const int32_t *min_obs, const int32_t *tail_trim, int stride,
                         int n_reads, int L, int flags, int32_t *start_out, int32_t *end_out, int32_t *early_stop_out)
{
    if (!h || !trace || !len || !min_obs || !tail_trim || !start_out || !end_out || !early_stop_out || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (stride < 1) { g_err = "stride must be >= 1"; return ADP_ERR_INVALID; }
    if (!lens_ok(len, n_reads, L)) { g_err = "need 0 <= len <= L for every read"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const size_t n = n_reads;
    Piece<double> s_tr; Piece<int32_t> dlen, dmo, dtt, ds, de, des;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_tr = w.take<double>((size_t)L * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dmo = w.take<int32_t>(n); dtt = w.take<int32_t>(n);
        ds = w.take<int32_t>(n); de = w.take<int32_t>(n); des = w.take<int32_t>(n);
    }));
    const double *dtr;
    RCCHK(stage_in<double>(h, flags, trace, s_tr, &dtr));
    RCCHK(h2d(h, dlen, len)); RCCHK(h2d(h, dmo, min_obs)); RCCHK(h2d(h, dtt, tail_trim));
    const int interp = (flags & ADP_LLR_INTERP) && stride > 1;
    { Scope s(h, "k_trace_bounds");
      hipLaunchKernelGGL(k_trace_bounds, dim3(n_reads), dim3(64), 0, h->stream, const_cast<double *>(dtr), dlen, L, dmo, dtt, stride, interp, ds, de, des); }
    HIPCHK(hipGetLastError());
    if (interp && !(flags & ADP_IN_DEVICE)) RCCHK(d2h(h, trace, s_tr));
    RCCHK(d2h(h, start_out, ds)); RCCHK(d2h(h, end_out, de)); RCCHK(d2h(h, early_stop_out, des));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_llr_trace_peaks(adp_handle *h, const double *trace, const int32_t *len, const int32_t *clip_lo, const int32_t *clip_hi, int n_reads,
                        int L, const adp_peak_args *args, int flags, int cap, int64_t *peaks_out, int64_t *count_out)
{
    if (!h || !trace || !len || !clip_lo || !clip_hi || !args || !peaks_out || !count_out || n_reads < 1 || L < 1 || cap < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!lens_ok(len, n_reads, L)) { g_err = "need 0 <= len <= L for every read"; return ADP_ERR_INVALID; }
    const int given = (flags & ADP_LLR_GIVEN_PEAK) != 0;
    bool clips_ok = given || spans_ok(clip_lo, clip_hi, len, n_reads);
    for (int r = 0; given && r < n_reads; r++) clips_ok = clips_ok && clip_lo[r] >= 0 && clip_lo[r] < len[r];
    if (!clips_ok) { g_err = "need 0 <= clip_lo <= clip_hi <= len (with ADP_LLR_GIVEN_PEAK: 0 <= clip_lo < len) for every read"; return ADP_ERR_INVALID; }
    const adp_peak_args &a = *args;
    if ((a.plateau_on && a.plateau_s < 1) || (a.split_on && a.split_s < 0)) { g_err = "plateau s must be >= 1, split s >= 0"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const size_t n = n_reads;
    const int nsum = (L + SUMBLK - 1) / SUMBLK;
    Piece<double> s_tr, bx, bn; Piece<int32_t> dlen, dlo, dhi; Piece<int64_t> dcnt, dpk;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_tr = w.take<double>((size_t)L * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dlo = w.take<int32_t>(n); dhi = w.take<int32_t>(n);
        dcnt = w.take<int64_t>(n); dpk = w.take<int64_t>(n * cap);
        bx = w.take<double>(nsum * n); bn = w.take<double>(nsum * n);
    }));
    const double *dtr;
    RCCHK(stage_in(h, flags, trace, s_tr, &dtr));
    RCCHK(h2d(h, dlen, len)); RCCHK(h2d(h, dlo, clip_lo)); RCCHK(h2d(h, dhi, clip_hi));
    trace_blocksum(h, dtr, dlen, n_reads, L, nsum, 0, bx, bn);
    { Scope s(h, "k_trace_peaks");
      hipLaunchKernelGGL(k_trace_peaks, dim3(n_reads), dim3(64), 0, h->stream, dtr, dlen, L, dlo, dhi, bx, bn, nsum, a, given, cap, dpk, dcnt); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, count_out, dcnt));
    RCCHK(d2h(h, peaks_out, dpk));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_llr_spike_peak(adp_handle *h, const double *trace, const int32_t *len, int n_reads, int L, const adp_spike_args *args, int flags,
                       int64_t *out)
{
    if (!h || !trace || !len || !args || !out || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!lens_ok(len, n_reads, L)) { g_err = "need 0 <= len <= L for every read"; return ADP_ERR_INVALID; }
    const adp_spike_args &a = *args;
    if (!(a.min_peak_distance >= 1.0)) { g_err = "min_peak_distance must be >= 1 (scipy: `distance` must be greater or equal to 1)"; return ADP_ERR_INVALID; }
    const double dd = ceil(a.min_peak_distance);
    const int dist = dd > (double)L ? L + 1 : (int)dd; // (beyond the row: every pair of maxima is within it)
    RCCHK(begin_call(h));
    const size_t n = n_reads;
    const int nsum = (L + SUMBLK - 1) / SUMBLK, half = L / 2 + 1;
    Piece<double> s_tr, bx, bn; Piece<int32_t> dlen; Piece<int64_t> dres;
    Piece<uint32_t> pk, wl; // the maxima and the work lists of k_trace_spike, half entries per read each
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_tr = w.take<double>((size_t)L * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dres = w.take<int64_t>(n);
        bx = w.take<double>(nsum * n); bn = w.take<double>(nsum * n);
        pk = w.take<uint32_t>(half * n); wl = w.take<uint32_t>(half * n);
    }));
    const double *dtr;
    RCCHK(stage_in(h, flags, trace, s_tr, &dtr));
    RCCHK(h2d(h, dlen, len));
    trace_blocksum(h, dtr, dlen, n_reads, L, nsum, 1, bx, bn);
    { Scope s(h, "k_trace_spike");
      hipLaunchKernelGGL(k_trace_spike, dim3(n_reads), dim3(64), 0, h->stream, dtr, dlen, L, bx, bn, nsum, a, dist, pk, wl, half, dres); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, out, dres));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// ---- the reference's MVS poly(A) module (adapted/detect/mvs.py) on batched signals (mvs_api.h)

static int mv_check_args(const void *sig, const int32_t *len, int n_reads, int L, const adp_mvs_args *a, std::initializer_list<const int64_t *> pos)
{
    if (!sig || !len || !a || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!lens_ok(len, n_reads, L)) { g_err = "need 0 <= len <= L for every read"; return ADP_ERR_INVALID; }
    for (const int64_t *p : pos) {
        if (!p) { g_err = "bad argument"; return ADP_ERR_INVALID; }
        if (!positions_ok(p, n_reads)) { g_err = "positions must lie in [0, 2^40]"; return ADP_ERR_INVALID; }
    }
    if (a->pA_mean_window < 1 || a->pA_var_window < 1 || a->s_pA_mean_window < 1 || a->s_pA_var_window < 1) {
        g_err = "moving windows must be >= 1"; return ADP_ERR_INVALID;
    }
    if (a->search_increment_step < 1) { g_err = "search_increment_step must be >= 1"; return ADP_ERR_INVALID; }
    return ADP_OK;
}

// slots of the series kernels: one wave each, [2, L] elements of scratch per slot (at most ~512 MiB in all)
static size_t mv_slots(int n_reads, int L, size_t esz)
{
    size_t slots = ((size_t)512 << 20) / ((size_t)2 * L * esz);
    if (slots < 64) slots = 64;
    if (slots > (size_t)n_reads) slots = n_reads;
    if (slots > 8192) slots = 8192;
    return slots;
}

int adp_mvs_check(adp_handle *h, const void *sig, const int32_t *len, const int64_t *adapter_end, const int64_t *polya_end, int n_reads,
                  int L, const adp_mvs_args *args, int flags, int32_t *info_out, double *vals_out)
{
    if (!h || !info_out || !vals_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(mv_check_args(sig, len, n_reads, L, args, {adapter_end, polya_end}));
    const size_t n = n_reads;
    RowsIn in; size_t slots; Piece<char> scr; Piece<int32_t> dinfo; Piece<int64_t> dae, dpe; Piece<double> dvals;
    RCCHK(rows_begin(h, sig, len, n_reads, L, flags, in, [&](Carve &w) {
        slots = mv_slots(n_reads, L, in.esz);
        dae = w.take<int64_t>(n); dpe = w.take<int64_t>(n);
        dinfo = w.take<int32_t>(n * 8); dvals = w.take<double>(n * 5);
        scr = w.take<char>(slots * 2 * L * in.esz);
    }));
    RCCHK(h2d(h, dae, adapter_end)); RCCHK(h2d(h, dpe, polya_end));
    { Scope s(h, "k_mvs_check");
      by_elem(in.f64, in.ds, [&](auto sig) { using T = elem_t<decltype(sig)>;
          hipLaunchKernelGGL(k_mvs_check<T>, dim3(slots), dim3(64), 0, h->stream, sig, in.dlen, n_reads, L, dae, dpe, *args, (T *)scr.p, dinfo, dvals); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo));
    RCCHK(d2h(h, vals_out, dvals));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_mvs_detect_at_loc(adp_handle *h, const void *sig, const int32_t *len, const int64_t *loc, int n_reads, int L,
                          const adp_mvs_args *args, int flags, int32_t *info_out, int64_t *idx_out, double *vals_out)
{
    if (!h || !info_out || !idx_out || !vals_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(mv_check_args(sig, len, n_reads, L, args, {loc}));
    const size_t n = n_reads;
    RowsIn in; size_t slots; Piece<char> scr; Piece<int32_t> dinfo; Piece<int64_t> dloc, didx; Piece<double> dvals;
    RCCHK(rows_begin(h, sig, len, n_reads, L, flags, in, [&](Carve &w) {
        slots = mv_slots(n_reads, L, in.esz);
        dloc = w.take<int64_t>(n);
        dinfo = w.take<int32_t>(n * 8); didx = w.take<int64_t>(n); dvals = w.take<double>(n * 5);
        scr = w.take<char>(slots * 2 * L * in.esz);
    }));
    RCCHK(h2d(h, dloc, loc));
    { Scope s(h, "k_mvs_at_loc");
      by_elem(in.f64, in.ds, [&](auto sig) { using T = elem_t<decltype(sig)>;
          hipLaunchKernelGGL(k_mvs_at_loc<T>, dim3(slots), dim3(64), 0, h->stream, sig, in.dlen, n_reads, L, dloc, *args, (T *)scr.p, dinfo, didx, dvals); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo));
    RCCHK(d2h(h, idx_out, didx));
    RCCHK(d2h(h, vals_out, dvals));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_mvs_detect(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_mvs_args *args, int flags,
                   int64_t *out)
{
    if (!h || !out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(mv_check_args(sig, len, n_reads, L, args, {}));
    if (args->min_obs_adapter < 0 || args->min_obs_post_loc < 0 || args->s_median_shift_window < 0 || args->s_polyA_window < 0) {
        g_err = "min_obs_adapter, min_obs_post_loc and the windows must be >= 0"; return ADP_ERR_INVALID;
    }
    RowsIn in; Piece<int64_t> dres;
    RCCHK(rows_begin(h, sig, len, n_reads, L, flags, in, [&](Carve &w) { dres = w.take<int64_t>(n_reads); }));
    // (one wave per read: a persistent grid of at most 16 waves per CU takes longer batches)
    const int grid = n_reads < h->n_cu * 16 ? n_reads : h->n_cu * 16;
    { Scope s(h, "k_mvs_stream");
      by_elem(in.f64, in.ds, [&](auto sig) { hipLaunchKernelGGL(k_mvs_stream<elem_t<decltype(sig)>>, dim3(grid), dim3(64), 0, h->stream, sig, in.dlen, n_reads, L, *args, dres); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, out, dres));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// ---- the reference's partition statistics (adapted/partition/signal_partitions.py) on batched segments (sigstats_api.h)

int adp_sizeof_seg(void) { return (int)sizeof(adp_seg); }

int adp_seg_stats(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg, int flags,
                  double *stats_out, int64_t *count_out)
{
    if (!h || !stats_out || !count_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(seg_check(sig, len, n_reads, L, segs, n_seg));
    const size_t ns = n_seg;
    SegIn in; Piece<double> dstats; Piece<int64_t> dcnt;
    RCCHK(seg_begin(h, sig, len, n_reads, L, segs, n_seg, flags, in, [&](Carve &w) { dstats = w.take<double>(ns * 4); dcnt = w.take<int64_t>(ns); }));
    { Scope s(h, "k_seg_stats");
      by_elem(in.f64, in.ds, [&](auto sig) { hipLaunchKernelGGL(k_seg_stats<elem_t<decltype(sig)>>, dim3(n_seg), dim3(SS_BLOCK), 0, h->stream, sig, in.dlen, n_reads, L, in.dsegs, n_seg, dstats, dcnt); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, stats_out, dstats));
    RCCHK(d2h(h, count_out, dcnt));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_sizeof_real_range_args(void) { return (int)sizeof(adp_real_range_args); }

static int ss_rows_check(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, int flags)
{
    if (!h || !sig || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (flags & ADP_SS_WHOLE) {
        if ((long long)n_reads * L > 0x7fffffffLL) { g_err = "a population of at most 2^31 - 1 samples"; return ADP_ERR_INVALID; }
    } else if (!len || !lens_ok(len, n_reads, L)) { g_err = "need 0 <= len <= L for every read"; return ADP_ERR_INVALID; }
    return ADP_OK;
}

int adp_med_mad(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, int flags, double *out)
{
    RCCHK(ss_rows_check(h, sig, len, n_reads, L, flags));
    if (!out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0, whole = (flags & ADP_SS_WHOLE) != 0;
    const size_t n = n_reads, esz = f64 ? 8 : 4, rows = whole ? 1 : n;
    Piece<char> s_sig; Piece<int32_t> dlen; Piece<double> dmm; Piece<SsPop> dst; Piece<uint32_t> dhist;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dmm = w.take<double>(rows * 2); dst = w.take<SsPop>(1); dhist = w.take<uint32_t>(512);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, &ds));
    const int32_t total = (int32_t)((long long)n_reads * L * (whole ? 1 : 0));
    if (whole) RCCHK(h2d(h, dlen, &total, 1)); else RCCHK(h2d(h, dlen, len));
    RCCHK(by_elem(f64, ds, [&](auto sig) { return ss_med_mad_dev(h, sig, dlen, n_reads, L, flags, dmm, dst, dhist); }));
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, out, dmm));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_normalize(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, double outlier_thresh, int flags,
                  double *medmad_io, void *out, int32_t *status_out)
{
    RCCHK(ss_rows_check(h, sig, len, n_reads, L, flags));
    if (!medmad_io || !out || !status_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    const bool f64 = (flags & ADP_MVS_F64) != 0, whole = (flags & ADP_SS_WHOLE) != 0, clip = (flags & ADP_SS_CLIP) != 0, out_dev = (flags & ADP_OUT_DEVICE) != 0;
    int nbx = (L + 1023) / 1024;
    if (nbx > 64) nbx = 64;
    if ((long long)n_reads * nbx > 0x7fffffffLL) { g_err = "too many rows"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const size_t n = n_reads, esz = f64 ? 8 : 4, rows = whole ? 1 : n, mat = (size_t)L * esz * n;
    Piece<char> s_sig, w_out; Piece<int32_t> dlen, dstat; Piece<double> dmm; Piece<SsPop> dst; Piece<uint32_t> dhist;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>(mat, !(flags & ADP_IN_DEVICE)); w_out = w.take<char>(mat, !out_dev);
        dlen = w.take<int32_t>(n); dstat = w.take<int32_t>(rows); dmm = w.take<double>(rows * 2); dst = w.take<SsPop>(1); dhist = w.take<uint32_t>(512);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, &ds));
    const int32_t total = (int32_t)((long long)n_reads * L * (whole ? 1 : 0));
    if (whole) RCCHK(h2d(h, dlen, &total, 1)); else RCCHK(h2d(h, dlen, len));
    if (clip) RCCHK(h2d(h, dmm, medmad_io));
    else RCCHK(by_elem(f64, ds, [&](auto sig) { return ss_med_mad_dev(h, sig, dlen, n_reads, L, flags, dmm, dst, dhist); }));
    void *dout = out_dev ? out : w_out.p;
    if (!out_dev) RCCHK(zero(h, w_out)); // (cells behind a read's end, rows of MAD 0: zeros on the host)
    const int32_t *klen = whole ? nullptr : dlen.p;
    { Scope s(h, "k_clip_scale");
      by_elem(f64, ds, [&](auto sig) { using T = elem_t<decltype(sig)>;
          hipLaunchKernelGGL(k_clip_scale<T>, dim3((unsigned)(n * nbx)), dim3(256), 0, h->stream, sig, klen, (long long)L, dmm, outlier_thresh, whole ? 1 : 0, clip ? 1 : 0, nbx, (T *)dout, dstat); }); }
    HIPCHK(hipGetLastError());
    if (!out_dev) RCCHK(d2h(h, out, w_out));
    if (!clip) RCCHK(d2h(h, medmad_io, dmm));
    RCCHK(d2h(h, status_out, dstat));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_pool_mean(adp_handle *h, const void *data, int n_rows, int n_cols, int pool_size, int flags, void *out)
{
    if (!h || !data || !out || n_rows < 1 || n_cols < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (pool_size < 1) { g_err = "pool_size must be >= 1"; return ADP_ERR_INVALID; }
    const bool f64 = (flags & ADP_MVS_F64) != 0, out_dev = (flags & ADP_OUT_DEVICE) != 0;
    const long long n_out = ((long long)n_cols + pool_size - 1) / pool_size;
    const int nbx = (int)((n_out + 255) / 256);
    const long long grid = pool_size <= 128 ? (long long)n_rows * nbx : (long long)n_rows * n_out;
    if (grid > 0x7fffffffLL) { g_err = "too many outputs for one call"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const size_t esz = f64 ? 8 : 4, in_b = (size_t)n_rows * n_cols * esz, out_b = (size_t)n_rows * n_out * esz;
    Piece<char> s_in, w_out;
    RCCHK(ws_carve(h, [&](Carve &w) { s_in = w.take<char>(in_b, !(flags & ADP_IN_DEVICE)); w_out = w.take<char>(out_b, !out_dev); }));
    const void *dd;
    RCCHK(stage_in(h, flags, data, s_in, &dd));
    void *dout = out_dev ? out : w_out.p;
    if (pool_size <= 128) {
        Scope s(h, "k_pool_mean");
        by_elem(f64, dd, [&](auto in) { using T = elem_t<decltype(in)>;
            hipLaunchKernelGGL(k_pool_mean<T>, dim3((unsigned)grid), dim3(256), 0, h->stream, in, n_rows, (long long)n_cols, pool_size, n_out, nbx, (T *)dout); });
    } else {
        Scope s(h, "k_pool_mean_wave");
        by_elem(f64, dd, [&](auto in) { using T = elem_t<decltype(in)>;
            hipLaunchKernelGGL(k_pool_mean_wave<T>, dim3((unsigned)grid), dim3(64), 0, h->stream, in, n_rows, (long long)n_cols, pool_size, n_out, (T *)dout); });
    }
    HIPCHK(hipGetLastError());
    if (!out_dev) RCCHK(d2h(h, out, w_out));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_real_range(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                   const adp_real_range_args *args, int flags, int32_t *info_out, double *vals_out)
{
    if (!h || !args || !info_out || !vals_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(seg_check(sig, len, n_reads, L, segs, n_seg));
    if (args->mean_window < 1 || args->max_obs_local_range < 1) { g_err = "mean_window and max_obs_local_range must be >= 1"; return ADP_ERR_INVALID; }
    const size_t ns = n_seg;
    SegIn in; Piece<int32_t> dinfo; Piece<double> dvals;
    RCCHK(seg_begin(h, sig, len, n_reads, L, segs, n_seg, flags, in, [&](Carve &w) { dinfo = w.take<int32_t>(ns * 2); dvals = w.take<double>(ns * 3); }));
    { Scope s(h, "k_real_range");
      by_elem(in.f64, in.ds, [&](auto sig) { hipLaunchKernelGGL(k_real_range<elem_t<decltype(sig)>>, dim3(n_seg), dim3(SS_BLOCK), 0, h->stream, sig, in.dlen, n_reads, L, in.dsegs, n_seg, *args, dinfo, dvals); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo));
    RCCHK(d2h(h, vals_out, dvals));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_open_pores(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg, double lo,
                   double hi, double min_obs_diff, int flags, int cap, int64_t *pos_out, int64_t *count_out)
{
    if (!h || !pos_out || !count_out || cap < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(seg_check(sig, len, n_reads, L, segs, n_seg));
    if (lo != lo || hi != hi || min_obs_diff != min_obs_diff) { g_err = "the range and min_obs_diff must be numbers"; return ADP_ERR_INVALID; }
    const size_t ns = n_seg;
    SegIn in; Piece<int64_t> dpos, dcnt;
    RCCHK(seg_begin(h, sig, len, n_reads, L, segs, n_seg, flags, in, [&](Carve &w) { dpos = w.take<int64_t>(ns * cap); dcnt = w.take<int64_t>(ns * 3); }));
    { Scope s(h, "k_open_pores");
      by_elem(in.f64, in.ds, [&](auto sig) { hipLaunchKernelGGL(k_open_pores<elem_t<decltype(sig)>>, dim3(n_seg), dim3(64), 0, h->stream, sig, in.dlen, n_reads, L, in.dsegs, n_seg, lo, hi, min_obs_diff, cap, dpos, dcnt); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, pos_out, dpos));
    RCCHK(d2h(h, count_out, dcnt));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// ---- the reference's start-peak and adapter-start modules (adapted/detect/start_peak.py, adapter_start.py; startmods_api.h)

int adp_sizeof_start_peak_args(void) { return (int)sizeof(adp_start_peak_args); }
int adp_sizeof_adapter_start_args(void) { return (int)sizeof(adp_adapter_start_args); }

int adp_start_peak(adp_handle *h, const void *sig, const int32_t *full_len, int n_reads, int m, const adp_start_peak_args *args,
                   int flags, int32_t *info_out, double *vals_out)
{
    if (!h || !sig || !full_len || !args || !info_out || !vals_out || n_reads < 1 || m < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!all_in<int32_t>(full_len, n_reads, 0, INT32_MAX)) { g_err = "need full_len >= 0 for every read"; return ADP_ERR_INVALID; }
    if (args->downscale_factor < 1) { g_err = "downscale_factor must be >= 1"; return ADP_ERR_INVALID; }
    if (args->offset1 < 0 || args->offset2 < 0 || args->start_peak_max_idx < 0) { g_err = "offset1, offset2 and start_peak_max_idx must be >= 0"; return ADP_ERR_INVALID; }
    const size_t n = n_reads;
    RowsIn in; Piece<int32_t> dinfo; Piece<double> dvals;
    RCCHK(rows_begin(h, sig, full_len, n_reads, m, flags, in, [&](Carve &w) { dinfo = w.take<int32_t>(n * 5); dvals = w.take<double>(n * 2); }));
    // (one wave per read: a persistent grid of at most 16 waves per CU takes longer batches)
    const int grid = n_reads < h->n_cu * 16 ? n_reads : h->n_cu * 16;
    { Scope s(h, "k_startpeak_mod");
      by_elem(in.f64, in.ds, [&](auto sig) { hipLaunchKernelGGL(k_startpeak_mod<elem_t<decltype(sig)>>, dim3(grid), dim3(64), 0, h->stream, sig, in.dlen, n_reads, m, *args, dinfo, dvals); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo));
    RCCHK(d2h(h, vals_out, dvals));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_adapter_start(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_adapter_start_args *args,
                      int flags, int32_t *info_out, int64_t *out, int64_t *cand_out, double *diff_out)
{
    if (!h || !sig || !len || !args || !info_out || !out || !cand_out || !diff_out || n_reads < 1 || L < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!lens_ok(len, n_reads, L)) { g_err = "need 0 <= len <= L for every read"; return ADP_ERR_INVALID; }
    if (args->window < 1) { g_err = "moving windows must be >= 1"; return ADP_ERR_INVALID; }
    if (args->min_obs_adapter < 0) { g_err = "min_obs_adapter must be >= 0"; return ADP_ERR_INVALID; }
    const size_t n = n_reads;
    RowsIn in; size_t slots; Piece<char> scr; Piece<int32_t> dinfo; Piece<int64_t> dout, dcand; Piece<double> ddiff;
    RCCHK(rows_begin(h, sig, len, n_reads, L, flags, in, [&](Carve &w) {
        slots = mv_slots(n_reads, L, in.esz); // (a slot holds both series of one read, as the MVS series kernels' do: the same byte budget)
        dinfo = w.take<int32_t>(n * 4); dout = w.take<int64_t>(n); dcand = w.take<int64_t>(n); ddiff = w.take<double>(n);
        scr = w.take<char>(slots * 2 * L * in.esz);
    }));
    { Scope s(h, "k_adapter_start");
      by_elem(in.f64, in.ds, [&](auto sig) { using T = elem_t<decltype(sig)>;
          hipLaunchKernelGGL(k_adapter_start<T>, dim3(slots), dim3(64), 0, h->stream, sig, in.dlen, n_reads, L, *args, (T *)scr.p, dinfo, dout, dcand, ddiff); }); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo));
    RCCHK(d2h(h, out, dout));
    RCCHK(d2h(h, cand_out, dcand));
    RCCHK(d2h(h, diff_out, ddiff));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// ---- event segmentation of signal segments (an extension; events_api.h)

int adp_sizeof_event_args(void) { return (int)sizeof(adp_event_args); }

// what adp_event_levels asks of a segmentation call beside adp_segment_events' outputs (fingerprint_api.h): the widest event
// table and where its pieces go -- count and fp to device memory with ADP_OUT_DEVICE, lengths / levels / norm nowhere when NULL
struct EvLevels { int E; int32_t *count, *fpstatus, *lengths; double *levels, *fp, *norm; };

static int ev_args_check(const adp_event_args *args)
{
    if (args->window < 2 || args->window > EV_WMAX) { g_err = "window must lie in [2, 64]"; return ADP_ERR_INVALID; }
    if (args->min_distance < 1) { g_err = "min_distance must be >= 1 (scipy: `distance` must be greater or equal to 1)"; return ADP_ERR_INVALID; }
    if (!std::isfinite(args->threshold) || !(args->threshold > 0.0)) { g_err = "threshold must be finite and > 0"; return ADP_ERR_INVALID; }
    if (!std::isfinite(args->var_floor) || !(args->var_floor > 0.0)) { g_err = "var_floor must be finite and > 0"; return ADP_ERR_INVALID; }
    return ADP_OK;
}

// the body of the four segmentation calls, checks done: es[g] is segment g's slice of in.sig (host values) and lmax the longest;
// slots and batches; k_ev_levels behind k_ev_bounds with `lv`
static int ev_segment(adp_handle *h, const EvIn &in, const std::vector<EvSeg> &es, int lmax, const adp_event_args *args, int flags,
                      int cap, int64_t *pos_out, int64_t *info_out, double *stats_out, const EvLevels *lv)
{
    RCCHK(begin_call(h));
    const size_t ns = es.size();
    // a slot: the scores of one segment and its two lists of maxima; slots within a byte budget -- EV_SCRATCH_MIB, as the series
    // kernels' (mv_slots), or ADP_EVENTS_SCRATCH_MIB from the environment, read per call -- and batches of slots
    const size_t stride = ((size_t)(lmax > 0 ? lmax : 1) + 1) & ~(size_t)1, half = stride / 2 + 1;
    long long mib;
    RCCHK(scratch_mib("ADP_EVENTS_SCRATCH_MIB", getenv("ADP_EVENTS_SCRATCH_MIB"), EV_SCRATCH_MIB, &mib));
    size_t slots = ((size_t)mib << 20) / (stride * 8 + half * 8);
    if (slots < 1) slots = 1;
    if (slots > ns) slots = ns;
    if (slots > 32768) slots = 32768;
    Piece<char> s_sig; Piece<float> s_scale, s_offset; Piece<EvSeg> dsegs; Piece<int32_t> dnan; Piece<double> dscore, dstats; Piece<uint32_t> pk, wl; Piece<int64_t> dpos, dinfo;
    // (the event tables: in the workspace, but for the two that stay on the device with ADP_OUT_DEVICE)
    const bool lv_dev = lv && (flags & ADP_OUT_DEVICE);
    const size_t E = lv ? lv->E : 0;
    Piece<int32_t> dcount, dfst, dlens; Piece<double> dlev, dfp, dnorm;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>(in.bytes, !(flags & ADP_IN_DEVICE));
        s_scale = w.take<float>(ns, in.i16 && !(flags & ADP_IN_DEVICE)); s_offset = w.take<float>(ns, in.i16 && !(flags & ADP_IN_DEVICE));
        dsegs = w.take<EvSeg>(ns); dnan = w.take<int32_t>(ns);
        dpos = w.take<int64_t>(ns * cap); dinfo = w.take<int64_t>(ns * 2); dstats = w.take<double>(ns * 2);
        dscore = w.take<double>(slots * stride); pk = w.take<uint32_t>(slots * half); wl = w.take<uint32_t>(slots * half);
        if (lv) {
            dcount = w.take<int32_t>(ns, !lv_dev); dfst = w.take<int32_t>(ns); dlens = w.take<int32_t>(ns * E);
            dlev = w.take<double>(ns * E); dfp = w.take<double>(ns * E, !lv_dev); dnorm = w.take<double>(ns * 2);
        }
    }));
    int32_t *kcount = lv_dev ? lv->count : dcount.p; double *kfp = lv_dev ? lv->fp : dfp.p; // (what k_ev_levels writes)
    const void *ds; const float *dscale = nullptr, *doffset = nullptr;
    RCCHK(stage_in(h, flags, in.sig, s_sig, &ds));
    if (in.i16) { RCCHK(stage_in(h, flags, in.scale, s_scale, &dscale)); RCCHK(stage_in(h, flags, in.offset, s_offset, &doffset)); }
    RCCHK(h2d(h, dsegs, es.data()));
    RCCHK(zero(h, dnan));
    const adp_event_args &a = *args;
    for (size_t g0 = 0; g0 < ns; g0 += slots) {
        const size_t nb = ns - g0 < slots ? ns - g0 : slots;
        int bmax = 0;
        for (size_t g = g0; g < g0 + nb; g++) if (es[g].n > bmax) bmax = es[g].n;
        const int ntile = (bmax + EV_TILE - 1) / EV_TILE;
        if (ntile > 0) {
            Scope s(h, "k_ev_scores");
            by_source(in, ds, dscale, doffset, [&](auto src) { hipLaunchKernelGGL(k_ev_scores<decltype(src)>, dim3(ntile, (unsigned)nb), dim3(EV_BLOCK), 0, h->stream, src, dsegs, (int)g0, a.window, a.var_floor, stride, dscore, dnan); });
        }
        { Scope s(h, "k_ev_bounds");
          hipLaunchKernelGGL(k_ev_bounds, dim3((unsigned)nb), dim3(64), 0, h->stream, dscore, stride, dsegs, (int)g0, a.window, a.min_distance, a.threshold, cap, pk, wl, (int)half, dnan, dpos, dinfo, dstats); }
        if (lv) {
            Scope s(h, "k_ev_levels");
            by_source(in, ds, dscale, doffset, [&](auto src) { hipLaunchKernelGGL(k_ev_levels<decltype(src)>, dim3((unsigned)nb), dim3(64), 0, h->stream, src, dsegs, (int)g0, dscore, stride, wl, (int)half, dinfo, lv->E, kcount, dfst, dlens, dlev, kfp, dnorm); });
        }
    }
    HIPCHK(hipGetLastError());
    if (cap > 0) RCCHK(d2h(h, pos_out, dpos));
    RCCHK(d2h(h, info_out, dinfo));
    RCCHK(d2h(h, stats_out, dstats));
    if (lv) {
        RCCHK(d2h(h, lv->fpstatus, dfst));
        if (!lv_dev) { RCCHK(d2h(h, lv->count, dcount)); RCCHK(d2h(h, lv->fp, dfp)); }
        if (lv->lengths) RCCHK(d2h(h, lv->lengths, dlens));
        if (lv->levels) RCCHK(d2h(h, lv->levels, dlev));
        if (lv->norm) RCCHK(d2h(h, lv->norm, dnorm));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// adp_segment_events and, with `lv`, adp_event_levels: the checks and the clipped slices of the signal matrix, then ev_segment
static int ev_matrix(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                     const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out, double *stats_out,
                     const EvLevels *lv)
{
    RCCHK(seg_check(sig, len, n_reads, L, segs, n_seg));
    RCCHK(ev_args_check(args));
    if (L >= (1 << 30)) { g_err = "rows of fewer than 2^30 samples"; return ADP_ERR_INVALID; } // (positions share a word with 2 state bits)
    // the clipped slices (sigstats_api.h's ss_slice, on the host: len and segs are host arrays) and the longest one
    std::vector<EvSeg> es(n_seg);
    int lmax = 0;
    for (int g = 0; g < n_seg; g++) {
        const adp_seg &sg = segs[g];
        es[g] = EvSeg{0, 0, 0};
        if (sg.start < 0 || sg.end <= sg.start) continue;
        const long long S = len[sg.row];
        const long long a = sg.start < S ? sg.start : S, b = sg.end < S ? sg.end : S;
        es[g] = EvSeg{(long long)sg.row * L + a, (int32_t)(b - a), 0};
        if (es[g].n > lmax) lmax = es[g].n;
    }
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const EvIn in{sig, (size_t)L * (f64 ? 8 : 4) * n_reads, f64, false, nullptr, nullptr};
    return ev_segment(h, in, es, lmax, args, flags, cap, pos_out, info_out, stats_out, lv);
}

// adp_segment_events_packed and, with `lv`, adp_event_levels_packed: segment g is packed[offsets[g] : offsets[g + 1]), float32 pA or,
// with ADP_PACKED_I16, raw int16 samples with a calibration per segment; then ev_segment
static int ev_packed(adp_handle *h, const void *packed, const int64_t *offsets, const float *scale, const float *offset, int n_seg,
                     const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out, double *stats_out,
                     const EvLevels *lv)
{
    if (!packed || !offsets || n_seg < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    const bool i16 = (flags & ADP_PACKED_I16) != 0;
    if (i16 && (!scale || !offset)) { g_err = "ADP_PACKED_I16 needs a scale and an offset per segment"; return ADP_ERR_INVALID; }
    if (flags & ADP_MVS_F64) { g_err = "the packed calls take float32 or int16 samples, not float64"; return ADP_ERR_INVALID; }
    RCCHK(ev_args_check(args));
    if (offsets[0] < 0) { g_err = "offsets[0] must be >= 0"; return ADP_ERR_INVALID; }
    std::vector<EvSeg> es(n_seg);
    int lmax = 0;
    for (int g = 0; g < n_seg; g++) {
        if (offsets[g + 1] < offsets[g]) { g_err = "offsets must not decrease"; return ADP_ERR_INVALID; }
        const int64_t n = offsets[g + 1] - offsets[g];
        if (n >= ((int64_t)1 << 30)) { g_err = "segments of fewer than 2^30 samples"; return ADP_ERR_INVALID; } // (as ev_matrix's rows)
        es[g] = EvSeg{(long long)offsets[g], (int32_t)n, 0};
        if (es[g].n > lmax) lmax = es[g].n;
    }
    size_t bytes = (size_t)offsets[n_seg] * (i16 ? 2 : 4);
    if (bytes < 1) bytes = 1; // (every segment empty: nothing is read)
    const EvIn in{packed, bytes, false, i16, scale, offset};
    return ev_segment(h, in, es, lmax, args, flags, cap, pos_out, info_out, stats_out, lv);
}

static bool ev_levels_args(adp_handle *h, const adp_event_args *args, int64_t *info_out, double *stats_out, int32_t *count_out,
                           int32_t *fpstatus_out, double *fp_out)
{
    return h && args && info_out && stats_out && count_out && fpstatus_out && fp_out;
}

int adp_segment_events(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                       const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out, double *stats_out)
{
    if (!h || !args || !info_out || !stats_out || cap < 0 || (cap > 0 && !pos_out)) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    return ev_matrix(h, sig, len, n_reads, L, segs, n_seg, args, flags, cap, pos_out, info_out, stats_out, nullptr);
}

int adp_segment_events_packed(adp_handle *h, const void *packed, const int64_t *offsets, const float *scale, const float *offset,
                              int n_seg, const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out,
                              double *stats_out)
{
    if (!h || !args || !info_out || !stats_out || cap < 0 || (cap > 0 && !pos_out)) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    return ev_packed(h, packed, offsets, scale, offset, n_seg, args, flags, cap, pos_out, info_out, stats_out, nullptr);
}

// ---- adapter event fingerprints and their DTW distances to templates (an extension; fingerprint_api.h)

int adp_event_levels(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                     const adp_event_args *args, int flags, int max_events, int64_t *info_out, double *stats_out, int32_t *count_out,
                     int32_t *fpstatus_out, int32_t *lengths_out, double *levels_out, double *fp_out, double *norm_out)
{
    if (!ev_levels_args(h, args, info_out, stats_out, count_out, fpstatus_out, fp_out)) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (max_events < 2 || max_events > FP_EMAX) { g_err = "max_events must lie in [2, 512]"; return ADP_ERR_INVALID; }
    const EvLevels lv{max_events, count_out, fpstatus_out, lengths_out, levels_out, fp_out, norm_out};
    return ev_matrix(h, sig, len, n_reads, L, segs, n_seg, args, flags, 0, nullptr, info_out, stats_out, &lv);
}

int adp_event_levels_packed(adp_handle *h, const void *packed, const int64_t *offsets, const float *scale, const float *offset,
                            int n_seg, const adp_event_args *args, int flags, int max_events, int64_t *info_out, double *stats_out,
                            int32_t *count_out, int32_t *fpstatus_out, int32_t *lengths_out, double *levels_out, double *fp_out,
                            double *norm_out)
{
    if (!ev_levels_args(h, args, info_out, stats_out, count_out, fpstatus_out, fp_out)) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (max_events < 2 || max_events > FP_EMAX) { g_err = "max_events must lie in [2, 512]"; return ADP_ERR_INVALID; }
    const EvLevels lv{max_events, count_out, fpstatus_out, lengths_out, levels_out, fp_out, norm_out};
    return ev_packed(h, packed, offsets, scale, offset, n_seg, args, flags, 0, nullptr, info_out, stats_out, &lv);
}

int adp_dtw_assign(adp_handle *h, const double *q, const int32_t *q_count, int nq, int Eq, const double *t, const int32_t *t_count,
                   int nt, int Et, int band, int flags, double *dist_out, int32_t *best_out, double *bestdist_out)
{
    if (!h || !q || !q_count || !t || !t_count || !best_out || !bestdist_out || nq < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(dtw_templates_check(Eq, t, t_count, nt, Et, band, nullptr));
    // the distance matrix of a batch of queries within a byte budget: DTW_SCRATCH_MIB, or ADP_DTW_SCRATCH_MIB from the environment,
    // read per call
    long long mib;
    RCCHK(scratch_mib("ADP_DTW_SCRATCH_MIB", getenv("ADP_DTW_SCRATCH_MIB"), DTW_SCRATCH_MIB, &mib));
    const size_t nqs = nq, nts = nt;
    const size_t rows = batch_rows(mib, nts * 8, nqs, nts); // (a workgroup per pair of the batch)
    RCCHK(begin_call(h));
    Piece<double> s_q, dt, ddist, dbd; Piece<int32_t> s_qc, dtc, dbest;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_q = w.take<double>(nqs * Eq, !(flags & ADP_IN_DEVICE)); s_qc = w.take<int32_t>(nqs, !(flags & ADP_IN_DEVICE));
        dt = w.take<double>(nts * Et); dtc = w.take<int32_t>(nts);
        ddist = w.take<double>(rows * nts); dbest = w.take<int32_t>(nqs * 2); dbd = w.take<double>(nqs * 2);
    }));
    const double *dq; const int32_t *dqc;
    RCCHK(stage_in(h, flags, q, s_q, &dq));
    RCCHK(stage_in(h, flags, q_count, s_qc, &dqc));
    RCCHK(h2d(h, dt, t));
    RCCHK(h2d(h, dtc, t_count));
    for (size_t p0 = 0; p0 < nqs; p0 += rows) {
        const size_t nb = nqs - p0 < rows ? nqs - p0 : rows;
        const dim3 grid((unsigned)(nb * nts)), block(64);
        { Scope s(h, "k_dtw");
          by_width(Et, [&](auto c) { hipLaunchKernelGGL(k_dtw<decltype(c)::value>, grid, block, 0, h->stream, dq, dqc, (int)p0, Eq, dt, dtc, nt, Et, band, ddist); }); }
        { Scope s(h, "k_dtw_best");
          hipLaunchKernelGGL(k_dtw_best, dim3((unsigned)((nb + 63) / 64)), block, 0, h->stream, ddist, (int)nb, nt, dbest + p0 * 2, dbd + p0 * 2); }
        if (dist_out) RCCHK(d2h(h, dist_out + p0 * nts, ddist, nb * nts));
    }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, best_out, dbest));
    RCCHK(d2h(h, bestdist_out, dbd));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

} // extern "C"

// ---- building barcode templates: the warping path of a DTW alignment and one DBA iteration (an extension; dtw_align_api.h)

// what adp_dtw_align fills (host memory; lo, hi and sum may be null), or -- with t_new -- what adp_dba_step fills
struct DaOut { double *dist; int32_t *status, *lo, *hi; double *sum; double *t_new; int32_t *members; double *inertia; };

// both calls: adp_dtw_assign's checks and which in [-1, nt); the queries in batches within the byte budget; per batch k_dtw_align
// and either the copies of its path outputs or k_dba_reduce
static int da_run(adp_handle *h, const double *q, const int32_t *q_count, const int32_t *which, int nq, int Eq, const double *t,
                  const int32_t *t_count, int nt, int Et, int band, int flags, const DaOut &o)
{
    const bool dba = o.t_new != nullptr;
    if (!h || !q || !q_count || !which || !t || !t_count || nq < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    int mmax;
    RCCHK(dtw_templates_check(Eq, t, t_count, nt, Et, band, &mmax));
    if (!all_in<int32_t>(which, nq, -1, nt - 1)) { g_err = "need -1 <= which < nt for every query"; return ADP_ERR_INVALID; }
    long long mib;
    RCCHK(scratch_mib("ADP_DTW_SCRATCH_MIB", getenv("ADP_DTW_SCRATCH_MIB"), DTW_SCRATCH_MIB, &mib));
    // the direction codes: Eq rows of W units of C cells each (dtw_align_api.h), in LDS where they fit
    const int C = dtw_width(Et);
    const int W = (mmax + C - 1) / C;
    const size_t nqs = nq, nts = nt, Ets = Et;
    const size_t code_bytes = (size_t)Eq * W * (C == 8 ? 2 : 1);
    const bool global_codes = code_bytes > DA_LDS_CODES;
    const size_t rows = batch_rows(mib, Ets * 16 + (global_codes ? code_bytes : 0), nqs, 0);
    // the members of every template in ascending order (adp_dba_step)
    std::vector<int32_t> offs, list;
    if (dba) {
        offs.assign(nts + 1, 0);
        for (size_t p = 0; p < nqs; p++) if (which[p] >= 0) offs[which[p] + 1]++;
        for (size_t k = 0; k < nts; k++) offs[k + 1] += offs[k];
        list.resize(offs[nts] > 0 ? offs[nts] : 1);
        std::vector<int32_t> at(offs.begin(), offs.end() - 1);
        for (size_t p = 0; p < nqs; p++) if (which[p] >= 0) list[at[which[p]]++] = (int32_t)p;
    }
    RCCHK(begin_call(h));
    Piece<double> s_q, dt, ddist, dsum, dT, dinert, dtnew; Piece<int32_t> s_qc, dwhich, dtc, dstatus, dlo, dhi, doffs, dlist, dmem;
    Piece<long long> dN; Piece<unsigned char> dcodes;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_q = w.take<double>(nqs * Eq, !(flags & ADP_IN_DEVICE)); s_qc = w.take<int32_t>(nqs, !(flags & ADP_IN_DEVICE));
        dwhich = w.take<int32_t>(nqs); dt = w.take<double>(nts * Ets); dtc = w.take<int32_t>(nts);
        ddist = w.take<double>(nqs); dstatus = w.take<int32_t>(nqs);
        dlo = w.take<int32_t>(rows * Ets); dhi = w.take<int32_t>(rows * Ets); dsum = w.take<double>(rows * Ets);
        dcodes = w.take<unsigned char>(rows * code_bytes, global_codes);
        doffs = w.take<int32_t>(nts + 1, dba); dlist = w.take<int32_t>(list.size(), dba);
        dT = w.take<double>(nts * Ets, dba); dN = w.take<long long>(nts * Ets, dba); dmem = w.take<int32_t>(nts, dba);
        dinert = w.take<double>(nts, dba); dtnew = w.take<double>(nts * Ets, dba);
    }));
    const double *dq; const int32_t *dqc;
    RCCHK(stage_in(h, flags, q, s_q, &dq));
    RCCHK(stage_in(h, flags, q_count, s_qc, &dqc));
    RCCHK(h2d(h, dwhich, which));
    RCCHK(h2d(h, dt, t));
    RCCHK(h2d(h, dtc, t_count));
    if (dba) {
        RCCHK(h2d(h, doffs, offs.data()));
        RCCHK(h2d(h, dlist, list.data()));
        RCCHK(zero(h, dT)); RCCHK(zero(h, dN)); RCCHK(zero(h, dmem)); RCCHK(zero(h, dinert));
    }
    const size_t lds = global_codes ? 0 : (code_bytes + 15) & ~(size_t)15;
    const unsigned cells = (unsigned)((nts * Ets + 63) / 64);
    for (size_t p0 = 0; p0 < nqs; p0 += rows) {
        const size_t nb = nqs - p0 < rows ? nqs - p0 : rows;
        { Scope s(h, "k_dtw_align");
          by_width(Et, [&](auto c) {
              auto go = [&](auto g) {
                  hipLaunchKernelGGL((k_dtw_align<decltype(c)::value, decltype(g)::value>), dim3((unsigned)nb), dim3(64), lds, h->stream, dq, dqc,
                                     dwhich.p, (int)p0, Eq, dt, dtc.p, Et, band, W, dcodes.p, ddist.p, dstatus.p, dlo.p, dhi.p, dsum.p);
              };
              if (global_codes) go(std::true_type()); else go(std::false_type());
          }); }
        if (dba) {
            Scope s(h, "k_dba_reduce");
            hipLaunchKernelGGL(k_dba_reduce, dim3(cells), dim3(64), 0, h->stream, doffs, dlist, (int)p0, (int)nb, nt, Et, dtc, dstatus,
                               ddist, dlo, dhi, dsum, dT, dN, dmem, dinert);
        } else {
            if (o.lo) RCCHK(d2h(h, o.lo + p0 * Ets, dlo, nb * Ets));
            if (o.hi) RCCHK(d2h(h, o.hi + p0 * Ets, dhi, nb * Ets));
            if (o.sum) RCCHK(d2h(h, o.sum + p0 * Ets, dsum, nb * Ets));
        }
    }
    if (dba) {
        { Scope s(h, "k_dba_finish");
          hipLaunchKernelGGL(k_dba_finish, dim3(cells), dim3(64), 0, h->stream, dt, dtc, nt, Et, dT, dN, dmem, dtnew); }
        RCCHK(d2h(h, o.t_new, dtnew));
        RCCHK(d2h(h, o.members, dmem));
        RCCHK(d2h(h, o.inertia, dinert));
    }
    HIPCHK(hipGetLastError());
    if (o.dist) RCCHK(d2h(h, o.dist, ddist));
    if (o.status) RCCHK(d2h(h, o.status, dstatus));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

extern "C" {

int adp_dtw_align(adp_handle *h, const double *q, const int32_t *q_count, const int32_t *which, int nq, int Eq, const double *t,
                  const int32_t *t_count, int nt, int Et, int band, int flags, double *dist_out, int32_t *status_out, int32_t *lo_out,
                  int32_t *hi_out, double *sum_out)
{
    if (!dist_out || !status_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    return da_run(h, q, q_count, which, nq, Eq, t, t_count, nt, Et, band, flags, DaOut{dist_out, status_out, lo_out, hi_out, sum_out, nullptr, nullptr, nullptr});
}

int adp_dba_step(adp_handle *h, const double *q, const int32_t *q_count, const int32_t *which, int nq, int Eq, const double *t,
                 const int32_t *t_count, int nt, int Et, int band, int flags, double *t_new_out, int32_t *members_out,
                 double *inertia_out, double *dist_out)
{
    if (!t_new_out || !members_out || !inertia_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    return da_run(h, q, q_count, which, nq, Eq, t, t_count, nt, Et, band, flags,
                  DaOut{dist_out, nullptr, nullptr, nullptr, nullptr, t_new_out, members_out, inertia_out});
}

} // extern "C"

// ---- clustering fingerprints without labels: the all-pairs DTW matrix, BUILD, k-medoids, the silhouette (an extension;
// dtw_cluster_api.h)

// a [n, n] matrix that is device memory with ADP_IN_DEVICE, else staged into `piece`; refused where an entry is NaN, negative or
// infinite (k_cl_check: on the device, before anything else; the handle stays usable)
static int cl_matrix_in(adp_handle *h, int flags, const double *dist, size_t n, Piece<double> piece, Piece<int32_t> dflag, const double **dev)
{
    RCCHK(stage_in(h, flags, dist, piece, dev));
    RCCHK(zero(h, dflag));
    const size_t count = n * n, blocks = (count + 255) / 256;
    { Scope s(h, "k_cl_check");
      hipLaunchKernelGGL(k_cl_check, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, h->stream, *dev, count, dflag.p); }
    HIPCHK(hipGetLastError());
    int32_t flag = 0;
    RCCHK(d2h(h, &flag, dflag));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (flag) { g_err = "the distance matrix holds a NaN, a negative value or an infinity"; return ADP_ERR_INVALID; }
    return ADP_OK;
}

static bool cl_sizes_ok(int n, int k) { return n >= 1 && n <= CL_NMAX && k >= 1 && k <= CL_KMAX && k <= n; }

extern "C" {

int adp_dtw_pairwise(adp_handle *h, const double *q, const int32_t *q_count, int n, int E, int band, int flags, double *dist_out)
{
    if (!h || !q || !q_count || !dist_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (E < 1 || E > FP_EMAX) { g_err = "E must lie in [1, 512]"; return ADP_ERR_INVALID; }
    if (n < 1 || n > CL_NMAX) { g_err = "n must lie in [1, 16384]"; return ADP_ERR_INVALID; }
    if (band < 0) { g_err = "band must be >= 0"; return ADP_ERR_INVALID; }
    long long mib;
    RCCHK(scratch_mib("ADP_DTW_SCRATCH_MIB", getenv("ADP_DTW_SCRATCH_MIB"), DTW_SCRATCH_MIB, &mib));
    // scratch is needed for a host matrix only: the whole matrix where it fits the budget (every pair once, both entries written),
    // else bands of its rows (a pair once per band its rows lie in: the same bits, the recurrence being symmetric)
    const bool out_dev = (flags & ADP_OUT_DEVICE) != 0;
    const size_t ns = n;
    size_t rows = batch_rows(mib, ns * 8, ns, 0);
    const bool whole = out_dev || rows == ns;
    if (whole) rows = ns;
    RCCHK(begin_call(h));
    Piece<double> s_q, dmat; Piece<int32_t> s_qc;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_q = w.take<double>(ns * E, !(flags & ADP_IN_DEVICE)); s_qc = w.take<int32_t>(ns, !(flags & ADP_IN_DEVICE));
        dmat = w.take<double>(rows * ns, !out_dev);
    }));
    const double *dq; const int32_t *dqc;
    RCCHK(stage_in(h, flags, q, s_q, &dq));
    RCCHK(stage_in(h, flags, q_count, s_qc, &dqc));
    double *dout = out_dev ? dist_out : dmat.p;
    const int partners = whole ? n / 2 : n - 1;
    const int nchunks = partners < 1 ? 1 : (partners + CL_STRIP - 1) / CL_STRIP;
    for (size_t r0 = 0; r0 < ns; r0 += rows) {
        const size_t nb = ns - r0 < rows ? ns - r0 : rows;
        const dim3 grid((unsigned)(nb * nchunks)), block(64);
        { Scope s(h, "k_dtw_pairs");
          by_width(E, [&](auto c) { hipLaunchKernelGGL(k_dtw_pairs<decltype(c)::value>, grid, block, 0, h->stream, dq, dqc, n, E, band, (int)r0, nchunks, whole ? 1 : 0, dout); }); }
        if (!out_dev) RCCHK(d2h(h, dist_out + r0 * ns, dmat, nb * ns));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_kmedoids_build(adp_handle *h, const double *dist, int n, int kmax, int flags, int32_t *medoids_out, double *gain_out)
{
    if (!h || !dist || !medoids_out || !gain_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!cl_sizes_ok(n, kmax)) { g_err = "need 1 <= n <= 16384 and 1 <= kmax <= min(n, 4096)"; return ADP_ERR_INVALID; }
    const size_t ns = n, ks = kmax;
    RCCHK(begin_call(h));
    Piece<double> s_d, dvals, ddmin, dgain; Piece<int32_t> dflag, dismed, dmed;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_d = w.take<double>(ns * ns, !(flags & ADP_IN_DEVICE)); dflag = w.take<int32_t>(1);
        dvals = w.take<double>(ns); ddmin = w.take<double>(ns); dismed = w.take<int32_t>(ns);
        dmed = w.take<int32_t>(ks); dgain = w.take<double>(ks);
    }));
    const double *dd;
    RCCHK(cl_matrix_in(h, flags, dist, ns, s_d, dflag, &dd));
    RCCHK(zero(h, dismed));
    for (int c = 0; c < kmax; c++) {
        { Scope s(h, "k_cl_rowsum");
          if (c == 0) hipLaunchKernelGGL(k_cl_rowsum<false>, dim3((unsigned)n), dim3(64), 0, h->stream, dd, n, ddmin.p, dvals.p);
          else hipLaunchKernelGGL(k_cl_rowsum<true>, dim3((unsigned)n), dim3(64), 0, h->stream, dd, n, ddmin.p, dvals.p); }
        { Scope s(h, "k_cl_pick");
          hipLaunchKernelGGL(k_cl_pick, dim3(1), dim3(256), 0, h->stream, dd, n, c, dvals.p, dismed.p, dmed.p, dgain.p, ddmin.p); }
    }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, medoids_out, dmed));
    RCCHK(d2h(h, gain_out, dgain));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_kmedoids(adp_handle *h, const double *dist, int n, int k, int max_iter, int flags, int32_t *medoids_io, int32_t *assign_out,
                 double *sums_out, double *cost_out, int32_t *iters_out)
{
    if (!h || !dist || !medoids_io || !assign_out || !cost_out || !iters_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!cl_sizes_ok(n, k)) { g_err = "need 1 <= n <= 16384 and 1 <= k <= min(n, 4096)"; return ADP_ERR_INVALID; }
    if (max_iter < 0 || max_iter > (1 << 20)) { g_err = "max_iter must lie in [0, 2^20]"; return ADP_ERR_INVALID; }
    {
        std::vector<char> seen(n, 0);
        for (int c = 0; c < k; c++) {
            const int m = medoids_io[c];
            if (m < 0 || m >= n || seen[m]) { g_err = "the medoids must be k different rows"; return ADP_ERR_INVALID; }
            seen[m] = 1;
        }
    }
    const size_t ns = n, ks = k;
    RCCHK(begin_call(h));
    Piece<double> s_d, dnear, dsums, dcost; Piece<int32_t> dflag, dmed, dnew, dassign, dchanged;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_d = w.take<double>(ns * ns, !(flags & ADP_IN_DEVICE)); dflag = w.take<int32_t>(1);
        dmed = w.take<int32_t>(ks); dnew = w.take<int32_t>(ks); dassign = w.take<int32_t>(ns); dnear = w.take<double>(ns);
        dsums = w.take<double>(ns * ks); dcost = w.take<double>((size_t)max_iter + 1); dchanged = w.take<int32_t>(1);
    }));
    const double *dd;
    RCCHK(cl_matrix_in(h, flags, dist, ns, s_d, dflag, &dd));
    RCCHK(h2d(h, dmed, medoids_io));
    int it = 0;
    for (;;) {
        { Scope s(h, "k_cl_assign");
          hipLaunchKernelGGL(k_cl_assign, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, dd, n, dmed.p, k, dassign.p, dnear.p); }
        { Scope s(h, "k_cl_total");
          hipLaunchKernelGGL(k_cl_total, dim3(1), dim3(64), 0, h->stream, dnear.p, n, dcost.p + it); }
        if (it == max_iter && !sums_out) break;
        { Scope s(h, "k_cl_sums");
          hipLaunchKernelGGL(k_cl_sums, dim3((unsigned)n), dim3(64), 0, h->stream, dd, n, dassign.p, k, dsums.p); }
        if (it == max_iter) break;
        RCCHK(zero(h, dchanged));
        { Scope s(h, "k_cl_update");
          hipLaunchKernelGGL(k_cl_update, dim3((unsigned)k), dim3(256), 0, h->stream, dsums.p, n, k, dassign.p, dmed.p, dnew.p, dchanged.p); }
        HIPCHK(hipGetLastError());
        int32_t changed = 0;
        RCCHK(d2h(h, &changed, dchanged));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (!changed) break;
        std::swap(dmed, dnew);
        it++;
    }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, medoids_io, dmed));
    RCCHK(d2h(h, assign_out, dassign));
    if (sums_out) RCCHK(d2h(h, sums_out, dsums));
    RCCHK(d2h(h, cost_out, dcost, (size_t)it + 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    *iters_out = it;
    return ADP_OK;
}

int adp_silhouette(adp_handle *h, const double *dist, int n, const int32_t *assign, int k, int flags, double *sil_out)
{
    if (!h || !dist || !assign || !sil_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!cl_sizes_ok(n, k)) { g_err = "need 1 <= n <= 16384 and 1 <= k <= min(n, 4096)"; return ADP_ERR_INVALID; }
    if (!all_in<int32_t>(assign, n, 0, k - 1)) { g_err = "need 0 <= assign < k for every row"; return ADP_ERR_INVALID; }
    std::vector<int32_t> size(k, 0);
    for (int i = 0; i < n; i++) size[assign[i]]++;
    for (int c = 0; c < k; c++) if (!size[c]) { g_err = "a cluster without a member"; return ADP_ERR_INVALID; }
    const size_t ns = n, ks = k;
    RCCHK(begin_call(h));
    Piece<double> s_d, dsums, dsil; Piece<int32_t> dflag, dassign, dsize;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_d = w.take<double>(ns * ns, !(flags & ADP_IN_DEVICE)); dflag = w.take<int32_t>(1);
        dassign = w.take<int32_t>(ns); dsize = w.take<int32_t>(ks); dsums = w.take<double>(ns * ks); dsil = w.take<double>(ns);
    }));
    const double *dd;
    RCCHK(cl_matrix_in(h, flags, dist, ns, s_d, dflag, &dd));
    RCCHK(h2d(h, dassign, assign));
    RCCHK(h2d(h, dsize, size.data()));
    { Scope s(h, "k_cl_sums");
      hipLaunchKernelGGL(k_cl_sums, dim3((unsigned)n), dim3(64), 0, h->stream, dd, n, dassign.p, k, dsums.p); }
    { Scope s(h, "k_cl_sil");
      hipLaunchKernelGGL(k_cl_sil, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, dsums.p, n, k, dassign.p, dsize.p, dsil.p); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, sil_out, dsil));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

} // extern "C"

// ---- the k nearest labelled fingerprints of every query under DTW, pairs abandoned behind a lower bound (an extension;
// dtw_knn_api.h)

// a number the environment may hold under `name` (`value`: its getenv, read per call): `dflt` without it, else within [lo, hi]
static int knn_env(const char *name, const char *value, long long dflt, long long lo, long long hi, bool pow2, long long *out)
{
    *out = value ? atoll(value) : dflt;
    if (value && (*out < lo || *out > hi || (pow2 && (*out & (*out - 1))))) {
        g_err = std::string(name) + " must " + (pow2 ? "be a power of two and " : "") + "lie in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]";
        return ADP_ERR_INVALID;
    }
    return ADP_OK;
}

extern "C" {

int adp_dtw_knn(adp_handle *h, const double *q, const int32_t *q_count, int nq, int Eq, const double *r, const int32_t *r_count, int nr,
                int Er, int k, int band, int flags, const int32_t *exclude, int32_t *idx_out, double *dist_out, int64_t *work_out)
{
    if (!h || !q || !q_count || !r || !r_count || !idx_out || !dist_out || nq < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (Eq < 1 || Eq > FP_EMAX || Er < 1 || Er > FP_EMAX) { g_err = "Eq and Er must lie in [1, 512]"; return ADP_ERR_INVALID; }
    if (k < 1 || k > KNN_KMAX) { g_err = "k must lie in [1, 32]"; return ADP_ERR_INVALID; }
    if (nr < 1 || nr > KNN_NR_MAX) { g_err = "nr must lie in [1, 262144]"; return ADP_ERR_INVALID; }
    if (band < 0) { g_err = "band must be >= 0"; return ADP_ERR_INVALID; }
    RCCHK(table_check(r, r_count, nr, Er, "r_count", "Er", "reference", nullptr));
    if (exclude && !all_in<int32_t>(exclude, nq, -1, nr - 1)) { g_err = "every exclude must lie in [-1, nr)"; return ADP_ERR_INVALID; }
    long long mib, seg_env, period;
    RCCHK(scratch_mib("ADP_DTW_SCRATCH_MIB", getenv("ADP_DTW_SCRATCH_MIB"), DTW_SCRATCH_MIB, &mib));
    RCCHK(knn_env("ADP_KNN_SEGMENT_REFS", getenv("ADP_KNN_SEGMENT_REFS"), 0, 1, KNN_NR_MAX, false, &seg_env));
    RCCHK(knn_env("ADP_KNN_CHECK_PERIOD", getenv("ADP_KNN_CHECK_PERIOD"), KNN_CHECK_PERIOD, 1, 64, true, &period));
    // the segments of a query's references, a workgroup each: as many as make KNN_TARGET_WGS workgroups of all queries, of at least
    // KNN_SEG_MIN references (the fewer the segments, the more of a query's pairs tighten one threshold)
    int seg_refs = (int)seg_env;
    if (!seg_refs) {
        const int want = (KNN_TARGET_WGS + nq - 1) / nq;
        seg_refs = (nr + want - 1) / want;
        if (seg_refs < KNN_SEG_MIN) seg_refs = KNN_SEG_MIN;
    }
    if (seg_refs > nr) seg_refs = nr;
    const int nseg = (nr + seg_refs - 1) / seg_refs;
    // the segments' lists of a batch of queries within the byte budget
    const size_t nqs = nq, nrs = nr, ks = k, per_query = (size_t)nseg * (ks * 12 + 24);
    const size_t rows = batch_rows(mib, per_query, nqs, (size_t)nseg); // (a workgroup per segment of the batch)
    RCCHK(begin_call(h));
    Piece<double> s_q, dr, dsd, ddist; Piece<int32_t> s_qc, drc, dex, dsi, didx; Piece<long long> dsw, dwork;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_q = w.take<double>(nqs * Eq, !(flags & ADP_IN_DEVICE)); s_qc = w.take<int32_t>(nqs, !(flags & ADP_IN_DEVICE));
        dr = w.take<double>(nrs * Er); drc = w.take<int32_t>(nrs); dex = w.take<int32_t>(nqs, exclude != nullptr);
        dsd = w.take<double>(rows * nseg * ks); dsi = w.take<int32_t>(rows * nseg * ks); dsw = w.take<long long>(rows * nseg * 3);
        didx = w.take<int32_t>(nqs * ks); ddist = w.take<double>(nqs * ks); dwork = w.take<long long>(nqs * 3, work_out != nullptr);
    }));
    const double *dq; const int32_t *dqc;
    RCCHK(stage_in(h, flags, q, s_q, &dq));
    RCCHK(stage_in(h, flags, q_count, s_qc, &dqc));
    RCCHK(h2d(h, dr, r));
    RCCHK(h2d(h, drc, r_count));
    if (exclude) RCCHK(h2d(h, dex, exclude));
    const int pmask = (int)period - 1, prune = (flags & ADP_KNN_NO_PRUNE) ? 0 : 1;
    for (size_t p0 = 0; p0 < nqs; p0 += rows) {
        const size_t nb = nqs - p0 < rows ? nqs - p0 : rows;
        const dim3 grid((unsigned)(nb * nseg)), block(64 * KNN_WAVES);
        { Scope s(h, "k_dtw_knn");
          by_width(Er, [&](auto c) { hipLaunchKernelGGL(k_dtw_knn<decltype(c)::value>, grid, block, 0, h->stream, dq, dqc, (int)p0, Eq, dr.p, drc.p, nr, Er, band, k, seg_refs, nseg, pmask, prune, dex.p, dsd.p, dsi.p, dsw.p); }); }
        { Scope s(h, "k_knn_merge");
          hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)nb), dim3(64), 0, h->stream, dsd.p, dsi.p, dsw.p, nseg, k, (int)p0, didx.p, ddist.p, dwork.p); }
    }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, idx_out, didx));
    RCCHK(d2h(h, dist_out, ddist));
    if (work_out) RCCHK(d2h(h, work_out, dwork));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

} // extern "C"

// ---- the adapter's front boundary over the rows of a detect call (an extension; adapter_front.h)

// what both forms check before anything is launched
int af_check(adp_handle *h, const void *sig, int n_reads, int m, const adp_row *rows, const adp_adapter_front_args *args,
             const int32_t *info_out, const int64_t *shift_out, const int64_t *cand_out, const double *diff_out)
{
    if (!h || !sig || !rows || !args || !info_out || !shift_out || !cand_out || !diff_out || n_reads < 1 || m < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (args->window < 1) { g_err = "moving windows must be >= 1"; return ADP_ERR_INVALID; }
    if (args->min_obs_adapter < 0 || args->min_adapter_len < 0) { g_err = "min_obs_adapter and min_adapter_len must be >= 0"; return ADP_ERR_INVALID; }
    if (h->layout == ADP_LAYOUT_SINGLE_READ) { g_err = "adp_adapter_front: not with ADP_LAYOUT_SINGLE_READ"; return ADP_ERR_UNSUPPORTED; }
    return ADP_OK;
}

// a call's pieces of the workspace behind its staged signal: the rows (host rows only), the side outputs, the segments and their
// statistics, and the detector's slots ([2, m] floats each, the series kernels' byte budget: mv_slots)
struct AfBufs { Piece<adp_row> rows; Piece<int32_t> info; Piece<int64_t> shift, cand, cnt; Piece<double> diff, stats; Piece<SsSeg> segs; Piece<float> scr; size_t slots; };
static void af_pieces(Carve &w, AfBufs &b, int n_reads, int m, bool rows_dev)
{
    const size_t n = n_reads;
    b.slots = mv_slots(n_reads, m, 4);
    b.rows = w.take<adp_row>(n, !rows_dev);
    b.info = w.take<int32_t>(n * 4); b.shift = w.take<int64_t>(n); b.cand = w.take<int64_t>(n); b.diff = w.take<double>(n);
    b.segs = w.take<SsSeg>(n); b.stats = w.take<double>(n * 4); b.cnt = w.take<int64_t>(n);
    b.scr = w.take<float>(b.slots * 2 * m);
}

// the three kernels over a resident matrix of either kind, and the results back
template <class Sig>
static int af_run(adp_handle *h, Sig sig, int n_reads, int m, adp_row *rows, const adp_adapter_front_args *args, int flags, const AfBufs &b,
                  int32_t *info_out, int64_t *shift_out, int64_t *cand_out, double *diff_out)
{
    const bool rows_dev = (flags & ADP_OUT_DEVICE) != 0;
    adp_row *drows = rows_dev ? rows : b.rows.p;
    if (!rows_dev) RCCHK(h2d(h, b.rows, rows));
    { Scope s(h, "k_adapter_front");
      hipLaunchKernelGGL(k_adapter_front<Sig>, dim3((unsigned)b.slots), dim3(64), 0, h->stream, sig, n_reads, m, drows, *args, b.scr, b.info, b.shift, b.cand, b.diff, b.segs); }
    { Scope s(h, "k_seg_stats_sig");
      hipLaunchKernelGGL(k_seg_stats_sig<Sig>, dim3(n_reads), dim3(SS_BLOCK), 0, h->stream, sig, n_reads, m, b.segs, n_reads, b.stats, b.cnt); }
    { Scope s(h, "k_adapter_front_patch");
      hipLaunchKernelGGL(k_adapter_front_patch, dim3((n_reads + 255) / 256), dim3(256), 0, h->stream, drows, n_reads, b.segs, b.stats); }
    HIPCHK(hipGetLastError());
    if (!rows_dev) RCCHK(d2h(h, rows, b.rows));
    RCCHK(d2h(h, info_out, b.info));
    RCCHK(d2h(h, shift_out, b.shift));
    RCCHK(d2h(h, cand_out, b.cand));
    RCCHK(d2h(h, diff_out, b.diff));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// (handle.h) the detector alone for the re-validating forms: staged rows stay as they came, the patch is the validation's
int af_detect_staged(adp_handle *h, const float *sig, const int16_t *raw, const int32_t *full_len, const float *scale,
                     const float *offset, int n_reads, int m, const adp_row *rows, const adp_adapter_front_args *args, int flags,
                     AfStaged *out)
{
    AfBufs b;
    Piece<float> s_sig;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<float>((size_t)m * n_reads, !raw && !(flags & ADP_IN_DEVICE));
        af_pieces(w, b, n_reads, m, false);
    }));
    const float *ds = nullptr;
    if (!raw) RCCHK(stage_in(h, flags, sig, s_sig, &ds));
    RCCHK(h2d(h, b.rows, rows));
    { Scope s(h, "k_adapter_front");
      if (raw)
          hipLaunchKernelGGL(k_adapter_front<SigI16>, dim3((unsigned)b.slots), dim3(64), 0, h->stream, SigI16{raw, scale, offset, full_len}, n_reads, m,
                             (const adp_row *)b.rows.p, *args, b.scr, b.info, b.shift, b.cand, b.diff, b.segs);
      else
          hipLaunchKernelGGL(k_adapter_front<SigF32>, dim3((unsigned)b.slots), dim3(64), 0, h->stream, SigF32{ds}, n_reads, m,
                             (const adp_row *)b.rows.p, *args, b.scr, b.info, b.shift, b.cand, b.diff, b.segs); }
    HIPCHK(hipGetLastError());
    *out = AfStaged{ds, b.rows.p, b.info.p, b.shift.p, b.cand.p, b.diff.p};
    return ADP_OK;
}

extern "C" {

int adp_sizeof_adapter_front_args(void) { return (int)sizeof(adp_adapter_front_args); }

int adp_adapter_front(adp_handle *h, const float *sig, const int32_t *full_len, int n_reads, int m, adp_row *rows,
                      const adp_adapter_front_args *args, int flags, int32_t *info_out, int64_t *shift_out, int64_t *cand_out,
                      double *diff_out)
{
    (void)full_len; // (the matrix is read as it lies)
    RCCHK(af_check(h, sig, n_reads, m, rows, args, info_out, shift_out, cand_out, diff_out));
    RCCHK(begin_call(h));
    AfBufs b;
    Piece<float> s_sig;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<float>((size_t)m * n_reads, !(flags & ADP_IN_DEVICE));
        af_pieces(w, b, n_reads, m, (flags & ADP_OUT_DEVICE) != 0);
    }));
    const float *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, &ds));
    return af_run(h, SigF32{ds}, n_reads, m, rows, args, flags, b, info_out, shift_out, cand_out, diff_out);
}

int adp_adapter_front_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset,
                          int n_reads, int m, adp_row *rows, const adp_adapter_front_args *args, int flags, int32_t *info_out,
                          int64_t *shift_out, int64_t *cand_out, double *diff_out)
{
    RCCHK(af_check(h, raw, n_reads, m, rows, args, info_out, shift_out, cand_out, diff_out));
    if (!full_len || !scale || !offset) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!(flags & ADP_IN_DEVICE)) { g_err = "adp_adapter_front_i16 takes device pointers (ADP_IN_DEVICE)"; return ADP_ERR_INVALID; }
    if (m % 4 != 0) { g_err = "adp_adapter_front_i16: m must be a multiple of 4"; return ADP_ERR_UNSUPPORTED; }
    RCCHK(begin_call(h));
    AfBufs b;
    RCCHK(ws_carve(h, [&](Carve &w) { af_pieces(w, b, n_reads, m, (flags & ADP_OUT_DEVICE) != 0); }));
    return af_run(h, SigI16{raw, scale, offset, full_len}, n_reads, m, rows, args, flags, b, info_out, shift_out, cand_out, diff_out);
}

} // extern "C"

// ---- the rows of one output file to that file's CSV text (an extension; csv_api.h)

static bool csv_offsets_ok(const int64_t *off, int n)
{
    if (off[0] != 0) return false;
    for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return true;
}

extern "C" {

int adp_format_rows(adp_handle *h, const adp_row *rows, int n, int fail, int primary, const void *ids, const int64_t *id_off,
                    const int64_t *more, const int64_t *more_off, const void *strings, const int32_t *str_off, int n_str,
                    void *text_out, uint64_t text_cap, uint64_t *len_out, int32_t *n_fallback_out)
{
    if (!h || n < 0 || !len_out || !n_fallback_out || (!text_out && text_cap) || primary < 0 || primary > 2) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    *n_fallback_out = 0;
    if (n == 0) { // (no rows, no columns: the frame's text is a line break)
        *len_out = 1;
        if (text_cap >= 1) *(char *)text_out = '\n';
        return ADP_OK;
    }
    if (!rows || !ids || !id_off || !more_off || !strings || !str_off) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (n_str != CSV_N_STR || str_off[0] != 0) { g_err = "the string table must hold 69 entries from offset 0"; return ADP_ERR_INVALID; }
    for (int k = 0; k < n_str; k++) if (str_off[k + 1] < str_off[k]) { g_err = "the string table's offsets must ascend"; return ADP_ERR_INVALID; }
    if (!csv_offsets_ok(id_off, n) || !csv_offsets_ok(more_off, n)) { g_err = "offsets must ascend from 0"; return ADP_ERR_INVALID; }
    if (more_off[n] && !more) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    for (int i = 0; i < n; i++) {
        const adp_row &r = rows[i];
        if (r.fail_code < 0 || r.fail_code > 15 || r.start_peak_type < 0 || r.start_peak_type > 2) { g_err = "a row's fail_code or start_peak_type names no text"; return ADP_ERR_INVALID; }
        if (r.n_cand < -1 || r.n_cand > ADP_MAX_CAND || r.n_open_pores < -1) { g_err = "a row's list counts are out of range"; return ADP_ERR_INVALID; }
        const bool whole = r.n_open_pores > ADP_MAX_OPEN_PORES && !ADP_F_IS_EXCEPTION(r.fail_code); // (an exception row prints no list)
        if (more_off[i + 1] - more_off[i] != (whole ? r.n_open_pores : 0)) {
            g_err = "a row with more open pores than it holds needs its whole list, every other row none";
            return ADP_ERR_INVALID;
        }
    }
    const size_t ns = n, head = (size_t)(str_off[CSV_S_HEAD + (fail ? 1 : 0) + 1] - str_off[CSV_S_HEAD + (fail ? 1 : 0)]);
    const size_t body_cap = text_cap > head ? text_cap - head : 0;
    RCCHK(begin_call(h));
    Piece<adp_row> drows; Piece<unsigned char> dids, dstr, dtext; Piece<int64_t> did_off, dmore, dmore_off; Piece<int32_t> dstr_off;
    Piece<unsigned long long> dstate; Piece<unsigned int> dbad; Piece<uint32_t> dlen; Piece<uint64_t> doff;
    RCCHK(ws_carve(h, [&](Carve &w) {
        drows = w.take<adp_row>(ns); dids = w.take<unsigned char>((size_t)id_off[n] + 1); did_off = w.take<int64_t>(ns + 1);
        dmore = w.take<int64_t>((size_t)more_off[n] + 1); dmore_off = w.take<int64_t>(ns + 1);
        dstr = w.take<unsigned char>((size_t)str_off[n_str] + 1); dstr_off = w.take<int32_t>((size_t)n_str + 1);
        dstate = w.take<unsigned long long>(1); dbad = w.take<unsigned int>(1); dlen = w.take<uint32_t>(ns); doff = w.take<uint64_t>(ns + 1);
        dtext = w.take<unsigned char>(body_cap + 1);
    }));
    RCCHK(h2d(h, drows, rows));
    if (id_off[n]) RCCHK(h2d(h, dids, ids, (size_t)id_off[n]));
    RCCHK(h2d(h, did_off, id_off));
    if (more_off[n]) RCCHK(h2d(h, dmore, more, (size_t)more_off[n]));
    RCCHK(h2d(h, dmore_off, more_off));
    if (str_off[n_str]) RCCHK(h2d(h, dstr, strings, (size_t)str_off[n_str]));
    RCCHK(h2d(h, dstr_off, str_off));
    RCCHK(zero(h, dstate));
    RCCHK(zero(h, dbad));
    const CsvIn in{drows, n, fail ? 1 : 0, primary, dids, did_off, dmore, dmore_off, dstr, dstr_off};
    const unsigned nb = (unsigned)((ns + 255) / 256);
    { Scope s(h, "k_csv_state");
      hipLaunchKernelGGL(k_csv_state, dim3(nb), dim3(256), 0, h->stream, in, dstate.p); }
    { Scope s(h, "k_csv_rows");
      hipLaunchKernelGGL(k_csv_rows<false>, dim3(nb), dim3(256), 0, h->stream, in, (const unsigned long long *)dstate.p, dlen.p, dbad.p,
                         (const uint64_t *)nullptr, (unsigned char *)nullptr, (uint64_t)0); }
    { Scope s(h, "k_csv_scan");
      hipLaunchKernelGGL(k_csv_scan, dim3(1), dim3(256), 0, h->stream, (const uint32_t *)dlen.p, n, doff.p); }
    HIPCHK(hipGetLastError());
    uint64_t body = 0;
    unsigned int bad = 0;
    RCCHK(d2h(h, &body, Piece<uint64_t>{doff.p + ns, 1})); // (the sum behind the offsets)
    RCCHK(d2h(h, &bad, dbad));
    HIPCHK(hipStreamSynchronize(h->stream));
    *len_out = head + body;
    *n_fallback_out = (int32_t)bad;
    if (head + body > text_cap) return ADP_OK; // (nothing written: the caller comes again with that many bytes)
    { Scope s(h, "k_csv_rows");
      hipLaunchKernelGGL(k_csv_rows<true>, dim3(nb), dim3(256), 0, h->stream, in, (const unsigned long long *)dstate.p, dlen.p, dbad.p,
                         (const uint64_t *)doff.p, dtext.p, (uint64_t)body_cap); }
    HIPCHK(hipGetLastError());
    memcpy(text_out, (const char *)strings + str_off[CSV_S_HEAD + (fail ? 1 : 0)], head);
    if (body) RCCHK(d2h(h, (char *)text_out + head, dtext, (size_t)body));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

} // extern "C"
