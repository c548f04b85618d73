// modules.hip -- the reference-module drop-ins (adp_c_llr_*, adp_llr_*, adp_mvs_*, the signal statistics, the start peak, the adapter start, the event segmentation, the event fingerprints and the adapter-front post-pass): their kernels and entry points, a
// translation unit of their own, so that nothing here can move the code the compiler makes for the detect path's kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <initializer_list>
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
#include "adapter_front.h"

// ---- workspace, staging and per-read checks of the entry points

// 256-byte aligned pieces of the handle's workspace `ws`; a Carve without a base only adds up their sizes
struct Carve {
    char *base = nullptr;
    size_t off = 0;
    // `count` elements of T -- none (nullptr) unless `want`
    template <class T> T *take(size_t count, bool want = true)
    {
        if (!want) return nullptr;
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// a call's pieces of the workspace: `pieces(Carve &)` takes them all and runs twice -- first to add up the sizes, so that ws
// grows once, before anything is enqueued (ensure() moves the buffer), then to hand out the pointers.  Every module call
// completes before it returns, so the next one takes the same memory: a process holds the largest single call's need.
template <class F> static int ws_carve(adp_handle *h, F &&pieces)
{
    Carve c;
    pieces(c);
    if (h->ws.ensure(c.off)) { g_err = "device allocation failed"; return ADP_ERR_HIP; }
    c = Carve{h->ws.as<char>(), 0};
    pieces(c);
    return ADP_OK;
}

// copies on the handle's stream: a host array in, a result back
static int h2d(adp_handle *h, void *dst, const void *src, size_t bytes) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream)); return ADP_OK; }
static int d2h(adp_handle *h, void *dst, const void *src, size_t bytes) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream)); return ADP_OK; }

// the device pointer of an input that is device memory with ADP_IN_DEVICE, else host memory: then copied to `piece` (a
// workspace piece taken for it only in that case)
template <class T> static int stage_in(adp_handle *h, int flags, const T *src, T *piece, size_t bytes, const T **dev)
{
    if (flags & ADP_IN_DEVICE) { *dev = src; return ADP_OK; }
    *dev = piece;
    return h2d(h, piece, src, bytes);
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

// median and MAD on the device -> dmm [rows, 2] ([1, 2] with ADP_SS_WHOLE; then dlen[0] holds n_reads * L)
template <class T>
static int ss_med_mad_dev(adp_handle *h, const T *ds, const int32_t *dlen, int n_reads, int L, int flags, double *dmm, SsPop *dst,
                           uint32_t *dhist)
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
    HIPCHK(hipMemsetAsync(dhist, 0, 512 * sizeof(uint32_t), h->stream));
    for (int sel = 0; sel < 2; sel++) {
        HIPCHK(hipMemsetAsync(dst, 0, sizeof(SsPop), h->stream));
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
    const size_t cells = (size_t)L * n_reads, mat = cells * 8, n4 = (size_t)n_reads * 4;
    // the sums a raw call computes go to the caller's arrays when those are device outputs, else to the workspace
    const bool own_c = !from_sums && !(c_io && out_dev);
    int32_t *dlen, *dstart, *dend; double *s_raw, *s_c, *s_c2, *w_c, *w_c2, *w_g;
    RCCHK(ws_carve(h, [&](Carve &w) {
        dlen = w.take<int32_t>(n_reads); dstart = w.take<int32_t>(n_reads); dend = w.take<int32_t>(n_reads);
        s_raw = w.take<double>(cells, !from_sums && !in_dev);
        s_c = w.take<double>(cells, from_sums && !in_dev); s_c2 = w.take<double>(cells, from_sums && !in_dev);
        w_c = w.take<double>(cells, own_c); w_c2 = w.take<double>(cells, own_c);
        w_g = w.take<double>(cells, !out_dev);
    }));
    RCCHK(h2d(h, dlen, len, n4)); RCCHK(h2d(h, dstart, start, n4)); RCCHK(h2d(h, dend, end, n4));
    const double *dc, *dc2;
    if (from_sums) {
        RCCHK(stage_in(h, flags, c_io, s_c, mat, &dc));
        RCCHK(stage_in(h, flags, c2_io, s_c2, mat, &dc2));
    } else {
        const double *draw;
        RCCHK(stage_in(h, flags, raw, s_raw, mat, &draw));
        double *wc = own_c ? w_c : c_io, *wc2 = own_c ? w_c2 : c2_io;
        { Scope s(h, "k_trace_cumsum");
          hipLaunchKernelGGL(k_trace_cumsum<double>, dim3(n_reads), dim3(64), 0, h->stream, draw, dlen, L, n_reads, wc, wc2); }
        dc = wc; dc2 = wc2;
    }
    double *dg = out_dev ? gain_out : w_g;
    TraceArgs ta = {a.min_obs, a.border_trim, a.stride, a.adapter_early_stopping, a.adapter_early_stop_window, a.adapter_early_stop_stride,
                    a.polya_early_stopping, a.polya_early_stop_window, a.polya_early_stop_stride};
    { Scope s(h, "k_trace_gains");
      hipLaunchKernelGGL(k_trace_gains, dim3(n_reads), dim3(64), 0, h->stream, dc, dc2, dlen, dstart, dend, L, ta, dg); }
    HIPCHK(hipGetLastError());
    if (!out_dev) {
        RCCHK(d2h(h, gain_out, dg, mat));
        if (!from_sums && c_io) { RCCHK(d2h(h, c_io, dc, mat)); RCCHK(d2h(h, c2_io, dc2, mat)); }
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
    double *s_c, *s_c2, *part_g, *st_g; int32_t *part_x, *st_x; CdSeg *dsegs;
    RCCHK(ws_carve(h, [&](Carve &w) {
        dsegs = w.take<CdSeg>(n_reads);
        part_g = w.take<double>(n_reads * nck); part_x = w.take<int32_t>(n_reads * nck);
        st_x = w.take<int32_t>(n_reads); st_g = w.take<double>(n_reads);
        s_c = w.take<double>(cells, !in_dev); s_c2 = w.take<double>(cells, !in_dev);
    }));
    const double *dc, *dc2;
    RCCHK(stage_in(h, flags, c, s_c, cells * 8, &dc));
    RCCHK(stage_in(h, flags, c2, s_c2, cells * 8, &dc2));
    std::vector<CdSeg> segs(n_reads);
    for (int r = 0; r < n_reads; r++) {
        long lo = (long)start[r] + offset_head[r], hi = (long)end[r] - offset_tail[r];
        if (lo > end[r]) lo = end[r];
        if (hi < lo) hi = lo; // (an empty range: the reference's loop does not run)
        segs[r] = CdSeg{r, start[r], end[r], (int32_t)lo, (int32_t)hi, r};
    }
    RCCHK(h2d(h, dsegs, segs.data(), segs.size() * sizeof(CdSeg)));
    cd_splits(h, dc, dc2, L, dsegs, n_reads, part_g, part_x, st_x, st_g);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> x(n_reads);
    RCCHK(d2h(h, x.data(), st_x, (size_t)n_reads * 4));
    RCCHK(d2h(h, gain_out, st_g, (size_t)n_reads * 8));
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
    double *dc, *dc2, *part_g, *st_g, *med; int32_t *part_x, *st_x, *res, *dlen; CdSeg *segs, *psegs; void *s_raw;
    RCCHK(ws_carve(h, [&](Carve &w) {
        dc = w.take<double>(cells); dc2 = w.take<double>(cells); s_raw = w.take<char>(cells * esz, !in_dev);
        segs = w.take<CdSeg>(2 * n); psegs = w.take<CdSeg>(n);
        part_g = w.take<double>(2 * n * nck); part_x = w.take<int32_t>(2 * n * nck);
        st_x = w.take<int32_t>(4 * n); st_g = w.take<double>(4 * n); med = w.take<double>(4 * n); res = w.take<int32_t>(4 * n);
        dlen = w.take<int32_t>(n);
    }));
    const void *draw;
    RCCHK(stage_in(h, flags, raw, s_raw, cells * esz, &draw));
    RCCHK(h2d(h, dlen, len, n * 4));
    const CdArgs a = {min_obs_adapter, border_trim, min_obs_polya, polya ? 1 : 0};
    const int rb = (n_reads + 255) / 256;
    { Scope s(h, "k_trace_cumsum");
      if (f32) hipLaunchKernelGGL(k_trace_cumsum<float>, dim3(n_reads), dim3(64), 0, h->stream, (const float *)draw, dlen, L, n_reads, dc, dc2);
      else hipLaunchKernelGGL(k_trace_cumsum<double>, dim3(n_reads), dim3(64), 0, h->stream, (const double *)draw, dlen, L, n_reads, dc, dc2); }
    { Scope s(h, "k_cd_plan");
      hipLaunchKernelGGL(k_cd_plan, dim3(rb), dim3(256), 0, h->stream, 0, dlen, n_reads, a, st_x, segs); }
    cd_splits(h, dc, dc2, L, segs, n_reads, part_g, part_x, st_x, st_g);
    { Scope s(h, "k_cd_plan");
      hipLaunchKernelGGL(k_cd_plan, dim3(rb), dim3(256), 0, h->stream, 1, dlen, n_reads, a, st_x, segs); }
    cd_splits(h, dc, dc2, L, segs, 2 * n_reads, part_g, part_x, st_x, st_g);
    { Scope s(h, "k_cd_medians");
      if (f32) hipLaunchKernelGGL(k_cd_medians<float>, dim3(n_reads), dim3(CD_MED_BLOCK), 0, h->stream, (const float *)draw, dlen, L, a, st_x, st_g, res, med, psegs);
      else hipLaunchKernelGGL(k_cd_medians<double>, dim3(n_reads), dim3(CD_MED_BLOCK), 0, h->stream, (const double *)draw, dlen, L, a, st_x, st_g, res, med, psegs); }
    if (polya) {
        cd_splits(h, dc, dc2, L, psegs, n_reads, part_g, part_x, st_x, st_g);
        { Scope s(h, "k_cd_finish");
          hipLaunchKernelGGL(k_cd_finish, dim3(rb), dim3(256), 0, h->stream, n_reads, st_x, res); }
    }
    HIPCHK(hipGetLastError());
    std::vector<int32_t> hres(n * 4), sx;
    std::vector<double> sg, hmed;
    RCCHK(d2h(h, hres.data(), res, n * 16));
    if (splits_out) { sx.resize(n * 4); RCCHK(d2h(h, sx.data(), st_x, n * 16)); }
    if (stats_out) {
        sg.resize(n * 4); hmed.resize(n * 4);
        RCCHK(d2h(h, sg.data(), st_g, n * 32));
        RCCHK(d2h(h, hmed.data(), med, n * 32));
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
    const size_t n = n_reads, mat = (size_t)L * 8 * n;
    double *s_tr; int32_t *dlen, *dmo, *dtt, *ds, *de, *des;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_tr = w.take<double>((size_t)L * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dmo = w.take<int32_t>(n); dtt = w.take<int32_t>(n);
        ds = w.take<int32_t>(n); de = w.take<int32_t>(n); des = w.take<int32_t>(n);
    }));
    const double *dtr;
    RCCHK(stage_in(h, flags, trace, s_tr, mat, &dtr));
    RCCHK(h2d(h, dlen, len, n * 4)); RCCHK(h2d(h, dmo, min_obs, n * 4)); RCCHK(h2d(h, dtt, tail_trim, n * 4));
    const int interp = (flags & ADP_LLR_INTERP) && stride > 1;
    { Scope s(h, "k_trace_bounds");
      hipLaunchKernelGGL(k_trace_bounds, dim3(n_reads), dim3(64), 0, h->stream, const_cast<double *>(dtr), dlen, L, dmo, dtt, stride, interp, ds, de, des); }
    HIPCHK(hipGetLastError());
    if (interp && !(flags & ADP_IN_DEVICE)) RCCHK(d2h(h, trace, dtr, mat));
    RCCHK(d2h(h, start_out, ds, n * 4)); RCCHK(d2h(h, end_out, de, n * 4)); RCCHK(d2h(h, early_stop_out, des, n * 4));
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
    double *s_tr, *bx, *bn; int32_t *dlen, *dlo, *dhi; int64_t *dcnt, *dpk;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_tr = w.take<double>((size_t)L * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dlo = w.take<int32_t>(n); dhi = w.take<int32_t>(n);
        dcnt = w.take<int64_t>(n); dpk = w.take<int64_t>(n * cap);
        bx = w.take<double>(nsum * n); bn = w.take<double>(nsum * n);
    }));
    const double *dtr;
    RCCHK(stage_in(h, flags, trace, s_tr, (size_t)L * 8 * n, &dtr));
    RCCHK(h2d(h, dlen, len, n * 4)); RCCHK(h2d(h, dlo, clip_lo, n * 4)); RCCHK(h2d(h, dhi, clip_hi, n * 4));
    trace_blocksum(h, dtr, dlen, n_reads, L, nsum, 0, bx, bn);
    { Scope s(h, "k_trace_peaks");
      hipLaunchKernelGGL(k_trace_peaks, dim3(n_reads), dim3(64), 0, h->stream, dtr, dlen, L, dlo, dhi, bx, bn, nsum, a, given, cap, dpk, dcnt); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, count_out, dcnt, n * 8));
    RCCHK(d2h(h, peaks_out, dpk, n * 8 * cap));
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
    double *s_tr, *bx, *bn; int32_t *dlen; int64_t *dres;
    uint32_t *pk, *wl; // the maxima and the work lists of k_trace_spike, half entries per read each
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_tr = w.take<double>((size_t)L * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dres = w.take<int64_t>(n);
        bx = w.take<double>(nsum * n); bn = w.take<double>(nsum * n);
        pk = w.take<uint32_t>(half * n); wl = w.take<uint32_t>(half * n);
    }));
    const double *dtr;
    RCCHK(stage_in(h, flags, trace, s_tr, (size_t)L * 8 * n, &dtr));
    RCCHK(h2d(h, dlen, len, n * 4));
    trace_blocksum(h, dtr, dlen, n_reads, L, nsum, 1, bx, bn);
    { Scope s(h, "k_trace_spike");
      hipLaunchKernelGGL(k_trace_spike, dim3(n_reads), dim3(64), 0, h->stream, dtr, dlen, L, bx, bn, nsum, a, dist, pk, wl, half, dres); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, out, dres, n * 8));
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
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, esz = f64 ? 8 : 4, slots = mv_slots(n_reads, L, esz);
    void *s_sig, *scr; int32_t *dlen, *dinfo; int64_t *dae, *dpe; double *dvals;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dae = w.take<int64_t>(n); dpe = w.take<int64_t>(n);
        dinfo = w.take<int32_t>(n * 8); dvals = w.take<double>(n * 5);
        scr = w.take<char>(slots * 2 * L * esz);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dlen, len, n * 4)); RCCHK(h2d(h, dae, adapter_end, n * 8)); RCCHK(h2d(h, dpe, polya_end, n * 8));
    { Scope s(h, "k_mvs_check");
      if (f64) hipLaunchKernelGGL(k_mvs_check<double>, dim3(slots), dim3(64), 0, h->stream, (const double *)ds, dlen, n_reads, L, dae, dpe, *args, (double *)scr, dinfo, dvals);
      else hipLaunchKernelGGL(k_mvs_check<float>, dim3(slots), dim3(64), 0, h->stream, (const float *)ds, dlen, n_reads, L, dae, dpe, *args, (float *)scr, dinfo, dvals); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo, n * 32));
    RCCHK(d2h(h, vals_out, dvals, n * 40));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_mvs_detect_at_loc(adp_handle *h, const void *sig, const int32_t *len, const int64_t *loc, int n_reads, int L,
                          const adp_mvs_args *args, int flags, int32_t *info_out, int64_t *idx_out, double *vals_out)
{
    if (!h || !info_out || !idx_out || !vals_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(mv_check_args(sig, len, n_reads, L, args, {loc}));
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, esz = f64 ? 8 : 4, slots = mv_slots(n_reads, L, esz);
    void *s_sig, *scr; int32_t *dlen, *dinfo; int64_t *dloc, *didx; double *dvals;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dloc = w.take<int64_t>(n);
        dinfo = w.take<int32_t>(n * 8); didx = w.take<int64_t>(n); dvals = w.take<double>(n * 5);
        scr = w.take<char>(slots * 2 * L * esz);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dlen, len, n * 4)); RCCHK(h2d(h, dloc, loc, n * 8));
    { Scope s(h, "k_mvs_at_loc");
      if (f64) hipLaunchKernelGGL(k_mvs_at_loc<double>, dim3(slots), dim3(64), 0, h->stream, (const double *)ds, dlen, n_reads, L, dloc, *args, (double *)scr, dinfo, didx, dvals);
      else hipLaunchKernelGGL(k_mvs_at_loc<float>, dim3(slots), dim3(64), 0, h->stream, (const float *)ds, dlen, n_reads, L, dloc, *args, (float *)scr, dinfo, didx, dvals); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo, n * 32));
    RCCHK(d2h(h, idx_out, didx, n * 8));
    RCCHK(d2h(h, vals_out, dvals, n * 40));
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
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, esz = f64 ? 8 : 4;
    void *s_sig; int32_t *dlen; int64_t *dres;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dres = w.take<int64_t>(n);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dlen, len, n * 4));
    // (one wave per read: a persistent grid of at most 16 waves per CU takes longer batches)
    const int grid = n_reads < h->n_cu * 16 ? n_reads : h->n_cu * 16;
    { Scope s(h, "k_mvs_stream");
      if (f64) hipLaunchKernelGGL(k_mvs_stream<double>, dim3(grid), dim3(64), 0, h->stream, (const double *)ds, dlen, n_reads, L, *args, dres);
      else hipLaunchKernelGGL(k_mvs_stream<float>, dim3(grid), dim3(64), 0, h->stream, (const float *)ds, dlen, n_reads, L, *args, dres); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, out, dres, n * 8));
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
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, ns = n_seg, esz = f64 ? 8 : 4;
    void *s_sig; int32_t *dlen; SsSeg *dsegs; double *dstats; int64_t *dcnt;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dsegs = w.take<SsSeg>(ns);
        dstats = w.take<double>(ns * 4); dcnt = w.take<int64_t>(ns);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dlen, len, n * 4)); RCCHK(h2d(h, dsegs, segs, ns * sizeof(SsSeg)));
    { Scope s(h, "k_seg_stats");
      if (f64) hipLaunchKernelGGL(k_seg_stats<double>, dim3(n_seg), dim3(SS_BLOCK), 0, h->stream, (const double *)ds, dlen, n_reads, L, dsegs, n_seg, dstats, dcnt);
      else hipLaunchKernelGGL(k_seg_stats<float>, dim3(n_seg), dim3(SS_BLOCK), 0, h->stream, (const float *)ds, dlen, n_reads, L, dsegs, n_seg, dstats, dcnt); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, stats_out, dstats, ns * 32));
    RCCHK(d2h(h, count_out, dcnt, ns * 8));
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
    void *s_sig; int32_t *dlen; double *dmm; SsPop *dst; uint32_t *dhist;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dmm = w.take<double>(rows * 2); dst = w.take<SsPop>(1); dhist = w.take<uint32_t>(512);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    const int32_t total = (int32_t)((long long)n_reads * L * (whole ? 1 : 0));
    if (whole) RCCHK(h2d(h, dlen, &total, 4)); else RCCHK(h2d(h, dlen, len, n * 4));
    if (f64) RCCHK(ss_med_mad_dev(h, (const double *)ds, dlen, n_reads, L, flags, dmm, dst, dhist));
    else RCCHK(ss_med_mad_dev(h, (const float *)ds, dlen, n_reads, L, flags, dmm, dst, dhist));
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, out, dmm, rows * 16));
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
    void *s_sig, *w_out; int32_t *dlen, *dstat; double *dmm; SsPop *dst; uint32_t *dhist;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>(mat, !(flags & ADP_IN_DEVICE)); w_out = w.take<char>(mat, !out_dev);
        dlen = w.take<int32_t>(n); dstat = w.take<int32_t>(rows); dmm = w.take<double>(rows * 2); dst = w.take<SsPop>(1); dhist = w.take<uint32_t>(512);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, mat, &ds));
    const int32_t total = (int32_t)((long long)n_reads * L * (whole ? 1 : 0));
    if (whole) RCCHK(h2d(h, dlen, &total, 4)); else RCCHK(h2d(h, dlen, len, n * 4));
    if (clip) RCCHK(h2d(h, dmm, medmad_io, rows * 16));
    else if (f64) RCCHK(ss_med_mad_dev(h, (const double *)ds, dlen, n_reads, L, flags, dmm, dst, dhist));
    else RCCHK(ss_med_mad_dev(h, (const float *)ds, dlen, n_reads, L, flags, dmm, dst, dhist));
    void *dout = out_dev ? out : w_out;
    if (!out_dev) HIPCHK(hipMemsetAsync(dout, 0, mat, h->stream)); // (cells behind a read's end, rows of MAD 0: zeros on the host)
    const int32_t *klen = whole ? nullptr : dlen;
    { Scope s(h, "k_clip_scale");
      if (f64) hipLaunchKernelGGL(k_clip_scale<double>, dim3((unsigned)(n * nbx)), dim3(256), 0, h->stream, (const double *)ds, klen, (long long)L, dmm, outlier_thresh, whole ? 1 : 0, clip ? 1 : 0, nbx, (double *)dout, dstat);
      else hipLaunchKernelGGL(k_clip_scale<float>, dim3((unsigned)(n * nbx)), dim3(256), 0, h->stream, (const float *)ds, klen, (long long)L, dmm, outlier_thresh, whole ? 1 : 0, clip ? 1 : 0, nbx, (float *)dout, dstat); }
    HIPCHK(hipGetLastError());
    if (!out_dev) RCCHK(d2h(h, out, dout, mat));
    if (!clip) RCCHK(d2h(h, medmad_io, dmm, rows * 16));
    RCCHK(d2h(h, status_out, dstat, rows * 4));
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
    void *s_in, *w_out;
    RCCHK(ws_carve(h, [&](Carve &w) { s_in = w.take<char>(in_b, !(flags & ADP_IN_DEVICE)); w_out = w.take<char>(out_b, !out_dev); }));
    const void *dd;
    RCCHK(stage_in(h, flags, data, s_in, in_b, &dd));
    void *dout = out_dev ? out : w_out;
    if (pool_size <= 128) {
        Scope s(h, "k_pool_mean");
        if (f64) hipLaunchKernelGGL(k_pool_mean<double>, dim3((unsigned)grid), dim3(256), 0, h->stream, (const double *)dd, n_rows, (long long)n_cols, pool_size, n_out, nbx, (double *)dout);
        else hipLaunchKernelGGL(k_pool_mean<float>, dim3((unsigned)grid), dim3(256), 0, h->stream, (const float *)dd, n_rows, (long long)n_cols, pool_size, n_out, nbx, (float *)dout);
    } else {
        Scope s(h, "k_pool_mean_wave");
        if (f64) hipLaunchKernelGGL(k_pool_mean_wave<double>, dim3((unsigned)grid), dim3(64), 0, h->stream, (const double *)dd, n_rows, (long long)n_cols, pool_size, n_out, (double *)dout);
        else hipLaunchKernelGGL(k_pool_mean_wave<float>, dim3((unsigned)grid), dim3(64), 0, h->stream, (const float *)dd, n_rows, (long long)n_cols, pool_size, n_out, (float *)dout);
    }
    HIPCHK(hipGetLastError());
    if (!out_dev) RCCHK(d2h(h, out, dout, out_b));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_real_range(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                   const adp_real_range_args *args, int flags, int32_t *info_out, double *vals_out)
{
    if (!h || !args || !info_out || !vals_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(seg_check(sig, len, n_reads, L, segs, n_seg));
    if (args->mean_window < 1 || args->max_obs_local_range < 1) { g_err = "mean_window and max_obs_local_range must be >= 1"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, ns = n_seg, esz = f64 ? 8 : 4;
    void *s_sig; int32_t *dlen, *dinfo; SsSeg *dsegs; double *dvals;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dsegs = w.take<SsSeg>(ns); dinfo = w.take<int32_t>(ns * 2); dvals = w.take<double>(ns * 3);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dlen, len, n * 4)); RCCHK(h2d(h, dsegs, segs, ns * sizeof(SsSeg)));
    { Scope s(h, "k_real_range");
      if (f64) hipLaunchKernelGGL(k_real_range<double>, dim3(n_seg), dim3(SS_BLOCK), 0, h->stream, (const double *)ds, dlen, n_reads, L, dsegs, n_seg, *args, dinfo, dvals);
      else hipLaunchKernelGGL(k_real_range<float>, dim3(n_seg), dim3(SS_BLOCK), 0, h->stream, (const float *)ds, dlen, n_reads, L, dsegs, n_seg, *args, dinfo, dvals); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo, ns * 8));
    RCCHK(d2h(h, vals_out, dvals, ns * 24));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_open_pores(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg, double lo,
                   double hi, double min_obs_diff, int flags, int cap, int64_t *pos_out, int64_t *count_out)
{
    if (!h || !pos_out || !count_out || cap < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(seg_check(sig, len, n_reads, L, segs, n_seg));
    if (lo != lo || hi != hi || min_obs_diff != min_obs_diff) { g_err = "the range and min_obs_diff must be numbers"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, ns = n_seg, esz = f64 ? 8 : 4;
    void *s_sig; int32_t *dlen; SsSeg *dsegs; int64_t *dpos, *dcnt;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dsegs = w.take<SsSeg>(ns); dpos = w.take<int64_t>(ns * cap); dcnt = w.take<int64_t>(ns * 3);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dlen, len, n * 4)); RCCHK(h2d(h, dsegs, segs, ns * sizeof(SsSeg)));
    { Scope s(h, "k_open_pores");
      if (f64) hipLaunchKernelGGL(k_open_pores<double>, dim3(n_seg), dim3(64), 0, h->stream, (const double *)ds, dlen, n_reads, L, dsegs, n_seg, lo, hi, min_obs_diff, cap, dpos, dcnt);
      else hipLaunchKernelGGL(k_open_pores<float>, dim3(n_seg), dim3(64), 0, h->stream, (const float *)ds, dlen, n_reads, L, dsegs, n_seg, lo, hi, min_obs_diff, cap, dpos, dcnt); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, pos_out, dpos, ns * 8 * cap));
    RCCHK(d2h(h, count_out, dcnt, ns * 24));
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
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, esz = f64 ? 8 : 4;
    void *s_sig; int32_t *dlen, *dinfo; double *dvals;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)m * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dinfo = w.take<int32_t>(n * 5); dvals = w.take<double>(n * 2);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)m * esz * n, &ds));
    RCCHK(h2d(h, dlen, full_len, n * 4));
    // (one wave per read: a persistent grid of at most 16 waves per CU takes longer batches)
    const int grid = n_reads < h->n_cu * 16 ? n_reads : h->n_cu * 16;
    { Scope s(h, "k_startpeak_mod");
      if (f64) hipLaunchKernelGGL(k_startpeak_mod<double>, dim3(grid), dim3(64), 0, h->stream, (const double *)ds, dlen, n_reads, m, *args, dinfo, dvals);
      else hipLaunchKernelGGL(k_startpeak_mod<float>, dim3(grid), dim3(64), 0, h->stream, (const float *)ds, dlen, n_reads, m, *args, dinfo, dvals); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo, n * 20));
    RCCHK(d2h(h, vals_out, dvals, n * 16));
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
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    // (a slot holds both series of one read, as the MVS series kernels' do: the same byte budget)
    const size_t n = n_reads, esz = f64 ? 8 : 4, slots = mv_slots(n_reads, L, esz);
    void *s_sig, *scr; int32_t *dlen, *dinfo; int64_t *dout, *dcand; double *ddiff;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dlen = w.take<int32_t>(n); dinfo = w.take<int32_t>(n * 4); dout = w.take<int64_t>(n); dcand = w.take<int64_t>(n); ddiff = w.take<double>(n);
        scr = w.take<char>(slots * 2 * L * esz);
    }));
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dlen, len, n * 4));
    { Scope s(h, "k_adapter_start");
      if (f64) hipLaunchKernelGGL(k_adapter_start<double>, dim3(slots), dim3(64), 0, h->stream, (const double *)ds, dlen, n_reads, L, *args, (double *)scr, dinfo, dout, dcand, ddiff);
      else hipLaunchKernelGGL(k_adapter_start<float>, dim3(slots), dim3(64), 0, h->stream, (const float *)ds, dlen, n_reads, L, *args, (float *)scr, dinfo, dout, dcand, ddiff); }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, info_out, dinfo, n * 16));
    RCCHK(d2h(h, out, dout, n * 8));
    RCCHK(d2h(h, cand_out, dcand, n * 8));
    RCCHK(d2h(h, diff_out, ddiff, n * 8));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// ---- event segmentation of signal segments (an extension; events_api.h)

int adp_sizeof_event_args(void) { return (int)sizeof(adp_event_args); }

// what adp_event_levels asks of a segmentation call beside adp_segment_events' outputs (fingerprint_api.h): the widest event
// table and where its pieces go -- count and fp to device memory with ADP_OUT_DEVICE, lengths / levels / norm nowhere when NULL
struct EvLevels { int E; int32_t *count, *fpstatus, *lengths; double *levels, *fp, *norm; };

// adp_segment_events and, with `lv`, adp_event_levels: the same checks, slots and batches; k_ev_levels behind k_ev_bounds
static int ev_segment(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                      const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out, double *stats_out,
                      const EvLevels *lv)
{
    RCCHK(seg_check(sig, len, n_reads, L, segs, n_seg));
    if (args->window < 2 || args->window > EV_WMAX) { g_err = "window must lie in [2, 64]"; return ADP_ERR_INVALID; }
    if (args->min_distance < 1) { g_err = "min_distance must be >= 1 (scipy: `distance` must be greater or equal to 1)"; return ADP_ERR_INVALID; }
    if (!std::isfinite(args->threshold) || !(args->threshold > 0.0)) { g_err = "threshold must be finite and > 0"; return ADP_ERR_INVALID; }
    if (!std::isfinite(args->var_floor) || !(args->var_floor > 0.0)) { g_err = "var_floor must be finite and > 0"; return ADP_ERR_INVALID; }
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
    RCCHK(begin_call(h));
    const bool f64 = (flags & ADP_MVS_F64) != 0;
    const size_t n = n_reads, ns = n_seg, esz = f64 ? 8 : 4;
    // a slot: the scores of one segment and its two lists of maxima; slots within a byte budget -- EV_SCRATCH_MIB, as the series
    // kernels' (mv_slots), or ADP_EVENTS_SCRATCH_MIB from the environment, read per call -- and batches of slots
    const size_t stride = ((size_t)(lmax > 0 ? lmax : 1) + 1) & ~(size_t)1, half = stride / 2 + 1;
    long long mib = EV_SCRATCH_MIB;
    if (const char *v = getenv("ADP_EVENTS_SCRATCH_MIB")) { mib = atoll(v); if (mib < 1 || mib > (1 << 20)) { g_err = "ADP_EVENTS_SCRATCH_MIB must lie in [1, 2^20]"; return ADP_ERR_INVALID; } }
    size_t slots = ((size_t)mib << 20) / (stride * 8 + half * 8);
    if (slots < 1) slots = 1;
    if (slots > ns) slots = ns;
    if (slots > 32768) slots = 32768;
    void *s_sig; EvSeg *dsegs; int32_t *dnan; double *dscore, *dstats; uint32_t *pk, *wl; int64_t *dpos, *dinfo;
    // (the event tables: in the workspace, but for the two that stay on the device with ADP_OUT_DEVICE)
    const bool lv_dev = lv && (flags & ADP_OUT_DEVICE);
    const size_t E = lv ? lv->E : 0;
    int32_t *dcount = nullptr, *dfst = nullptr, *dlens = nullptr; double *dlev = nullptr, *dfp = nullptr, *dnorm = nullptr;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<char>((size_t)L * esz * n, !(flags & ADP_IN_DEVICE));
        dsegs = w.take<EvSeg>(ns); dnan = w.take<int32_t>(ns);
        dpos = w.take<int64_t>(ns * cap); dinfo = w.take<int64_t>(ns * 2); dstats = w.take<double>(ns * 2);
        dscore = w.take<double>(slots * stride); pk = w.take<uint32_t>(slots * half); wl = w.take<uint32_t>(slots * half);
        if (lv) {
            dcount = w.take<int32_t>(ns, !lv_dev); dfst = w.take<int32_t>(ns); dlens = w.take<int32_t>(ns * E);
            dlev = w.take<double>(ns * E); dfp = w.take<double>(ns * E, !lv_dev); dnorm = w.take<double>(ns * 2);
        }
    }));
    if (lv_dev) { dcount = lv->count; dfp = lv->fp; }
    const void *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)L * esz * n, &ds));
    RCCHK(h2d(h, dsegs, es.data(), ns * sizeof(EvSeg)));
    HIPCHK(hipMemsetAsync(dnan, 0, ns * 4, h->stream));
    const adp_event_args &a = *args;
    for (size_t g0 = 0; g0 < ns; g0 += slots) {
        const size_t nb = ns - g0 < slots ? ns - g0 : slots;
        int bmax = 0;
        for (size_t g = g0; g < g0 + nb; g++) if (es[g].n > bmax) bmax = es[g].n;
        const int ntile = (bmax + EV_TILE - 1) / EV_TILE;
        if (ntile > 0) {
            Scope s(h, "k_ev_scores");
            if (f64) hipLaunchKernelGGL(k_ev_scores<double>, dim3(ntile, (unsigned)nb), dim3(EV_BLOCK), 0, h->stream, (const double *)ds, dsegs, (int)g0, a.window, a.var_floor, stride, dscore, dnan);
            else hipLaunchKernelGGL(k_ev_scores<float>, dim3(ntile, (unsigned)nb), dim3(EV_BLOCK), 0, h->stream, (const float *)ds, dsegs, (int)g0, a.window, a.var_floor, stride, dscore, dnan);
        }
        { Scope s(h, "k_ev_bounds");
          hipLaunchKernelGGL(k_ev_bounds, dim3((unsigned)nb), dim3(64), 0, h->stream, dscore, stride, dsegs, (int)g0, a.window, a.min_distance, a.threshold, cap, pk, wl, (int)half, dnan, dpos, dinfo, dstats); }
        if (lv) {
            Scope s(h, "k_ev_levels");
            if (f64) hipLaunchKernelGGL(k_ev_levels<double>, dim3((unsigned)nb), dim3(64), 0, h->stream, (const double *)ds, dsegs, (int)g0, dscore, stride, wl, (int)half, dinfo, lv->E, dcount, dfst, dlens, dlev, dfp, dnorm);
            else hipLaunchKernelGGL(k_ev_levels<float>, dim3((unsigned)nb), dim3(64), 0, h->stream, (const float *)ds, dsegs, (int)g0, dscore, stride, wl, (int)half, dinfo, lv->E, dcount, dfst, dlens, dlev, dfp, dnorm);
        }
    }
    HIPCHK(hipGetLastError());
    if (cap > 0) RCCHK(d2h(h, pos_out, dpos, ns * 8 * cap));
    RCCHK(d2h(h, info_out, dinfo, ns * 16));
    RCCHK(d2h(h, stats_out, dstats, ns * 16));
    if (lv) {
        RCCHK(d2h(h, lv->fpstatus, dfst, ns * 4));
        if (!lv_dev) { RCCHK(d2h(h, lv->count, dcount, ns * 4)); RCCHK(d2h(h, lv->fp, dfp, ns * E * 8)); }
        if (lv->lengths) RCCHK(d2h(h, lv->lengths, dlens, ns * E * 4));
        if (lv->levels) RCCHK(d2h(h, lv->levels, dlev, ns * E * 8));
        if (lv->norm) RCCHK(d2h(h, lv->norm, dnorm, ns * 16));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_segment_events(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                       const adp_event_args *args, int flags, int cap, int64_t *pos_out, int64_t *info_out, double *stats_out)
{
    if (!h || !args || !info_out || !stats_out || cap < 0 || (cap > 0 && !pos_out)) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    return ev_segment(h, sig, len, n_reads, L, segs, n_seg, args, flags, cap, pos_out, info_out, stats_out, nullptr);
}

// ---- adapter event fingerprints and their DTW distances to templates (an extension; fingerprint_api.h)

int adp_event_levels(adp_handle *h, const void *sig, const int32_t *len, int n_reads, int L, const adp_seg *segs, int n_seg,
                     const adp_event_args *args, int flags, int max_events, int64_t *info_out, double *stats_out, int32_t *count_out,
                     int32_t *fpstatus_out, int32_t *lengths_out, double *levels_out, double *fp_out, double *norm_out)
{
    if (!h || !args || !info_out || !stats_out || !count_out || !fpstatus_out || !fp_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (max_events < 2 || max_events > FP_EMAX) { g_err = "max_events must lie in [2, 512]"; return ADP_ERR_INVALID; }
    const EvLevels lv{max_events, count_out, fpstatus_out, lengths_out, levels_out, fp_out, norm_out};
    return ev_segment(h, sig, len, n_reads, L, segs, n_seg, args, flags, 0, nullptr, info_out, stats_out, &lv);
}

int adp_dtw_assign(adp_handle *h, const double *q, const int32_t *q_count, int nq, int Eq, const double *t, const int32_t *t_count,
                   int nt, int Et, int band, int flags, double *dist_out, int32_t *best_out, double *bestdist_out)
{
    if (!h || !q || !q_count || !t || !t_count || !best_out || !bestdist_out || nq < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (Eq < 1 || Eq > FP_EMAX || Et < 1 || Et > FP_EMAX) { g_err = "Eq and Et must lie in [1, 512]"; return ADP_ERR_INVALID; }
    if (nt < 1 || nt > DTW_NT_MAX) { g_err = "nt must lie in [1, 4096]"; return ADP_ERR_INVALID; }
    if (band < 0) { g_err = "band must be >= 0"; return ADP_ERR_INVALID; }
    for (int k = 0; k < nt; k++) {
        if (t_count[k] < 1 || t_count[k] > Et) { g_err = "need 1 <= t_count <= Et for every template"; return ADP_ERR_INVALID; }
        for (int j = 0; j < t_count[k]; j++)
            if (!std::isfinite(t[(size_t)k * Et + j])) { g_err = "template values inside their count must be finite"; return ADP_ERR_INVALID; }
    }
    // the distance matrix of a batch of queries within a byte budget: DTW_SCRATCH_MIB, or ADP_DTW_SCRATCH_MIB from the environment,
    // read per call
    long long mib = DTW_SCRATCH_MIB;
    if (const char *v = getenv("ADP_DTW_SCRATCH_MIB")) { mib = atoll(v); if (mib < 1 || mib > (1 << 20)) { g_err = "ADP_DTW_SCRATCH_MIB must lie in [1, 2^20]"; return ADP_ERR_INVALID; } }
    const size_t nqs = nq, nts = nt;
    size_t rows = ((size_t)mib << 20) / (nts * 8);
    if (rows < 1) rows = 1;
    if (rows > nqs) rows = nqs;
    if (rows > (size_t)0x7fffffff / nts) rows = (size_t)0x7fffffff / nts; // (a workgroup per pair of the batch)
    RCCHK(begin_call(h));
    double *s_q, *dt, *ddist, *dbd; int32_t *s_qc, *dtc, *dbest;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_q = w.take<double>(nqs * Eq, !(flags & ADP_IN_DEVICE)); s_qc = w.take<int32_t>(nqs, !(flags & ADP_IN_DEVICE));
        dt = w.take<double>(nts * Et); dtc = w.take<int32_t>(nts);
        ddist = w.take<double>(rows * nts); dbest = w.take<int32_t>(nqs * 2); dbd = w.take<double>(nqs * 2);
    }));
    const double *dq; const int32_t *dqc;
    RCCHK(stage_in(h, flags, q, s_q, nqs * Eq * 8, &dq));
    RCCHK(stage_in(h, flags, q_count, s_qc, nqs * 4, &dqc));
    RCCHK(h2d(h, dt, t, nts * Et * 8));
    RCCHK(h2d(h, dtc, t_count, nts * 4));
    const int C = (Et + 63) / 64;
    for (size_t p0 = 0; p0 < nqs; p0 += rows) {
        const size_t nb = nqs - p0 < rows ? nqs - p0 : rows;
        const dim3 grid((unsigned)(nb * nts)), block(64);
        { Scope s(h, "k_dtw");
          if (C <= 1) hipLaunchKernelGGL(k_dtw<1>, grid, block, 0, h->stream, dq, dqc, (int)p0, Eq, dt, dtc, nt, Et, band, ddist);
          else if (C <= 2) hipLaunchKernelGGL(k_dtw<2>, grid, block, 0, h->stream, dq, dqc, (int)p0, Eq, dt, dtc, nt, Et, band, ddist);
          else if (C <= 4) hipLaunchKernelGGL(k_dtw<4>, grid, block, 0, h->stream, dq, dqc, (int)p0, Eq, dt, dtc, nt, Et, band, ddist);
          else hipLaunchKernelGGL(k_dtw<8>, grid, block, 0, h->stream, dq, dqc, (int)p0, Eq, dt, dtc, nt, Et, band, ddist); }
        { Scope s(h, "k_dtw_best");
          hipLaunchKernelGGL(k_dtw_best, dim3((unsigned)((nb + 63) / 64)), block, 0, h->stream, ddist, (int)nb, nt, dbest + p0 * 2, dbd + p0 * 2); }
        if (dist_out) RCCHK(d2h(h, dist_out + p0 * nts, ddist, nb * nts * 8));
    }
    HIPCHK(hipGetLastError());
    RCCHK(d2h(h, best_out, dbest, nqs * 8));
    RCCHK(d2h(h, bestdist_out, dbd, nqs * 16));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

} // extern "C"

// ---- the adapter's front boundary over the rows of a detect call (an extension; adapter_front.h)

// what both forms check before anything is launched
static int af_check(adp_handle *h, const void *sig, int n_reads, int m, const adp_row *rows, const adp_adapter_front_args *args,
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
struct AfBufs { adp_row *rows; int32_t *info; int64_t *shift, *cand, *cnt; double *diff, *stats; SsSeg *segs; float *scr; size_t slots; };
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
    const size_t n = n_reads;
    const bool rows_dev = (flags & ADP_OUT_DEVICE) != 0;
    adp_row *drows = rows_dev ? rows : b.rows;
    if (!rows_dev) RCCHK(h2d(h, drows, rows, n * sizeof(adp_row)));
    { Scope s(h, "k_adapter_front");
      hipLaunchKernelGGL(k_adapter_front<Sig>, dim3((unsigned)b.slots), dim3(64), 0, h->stream, sig, n_reads, m, drows, *args, b.scr, b.info, b.shift, b.cand, b.diff, b.segs); }
    { Scope s(h, "k_seg_stats_sig");
      hipLaunchKernelGGL(k_seg_stats_sig<Sig>, dim3(n_reads), dim3(SS_BLOCK), 0, h->stream, sig, n_reads, m, b.segs, n_reads, b.stats, b.cnt); }
    { Scope s(h, "k_adapter_front_patch");
      hipLaunchKernelGGL(k_adapter_front_patch, dim3((n_reads + 255) / 256), dim3(256), 0, h->stream, drows, n_reads, b.segs, b.stats); }
    HIPCHK(hipGetLastError());
    if (!rows_dev) RCCHK(d2h(h, rows, drows, n * sizeof(adp_row)));
    RCCHK(d2h(h, info_out, b.info, n * 16));
    RCCHK(d2h(h, shift_out, b.shift, n * 8));
    RCCHK(d2h(h, cand_out, b.cand, n * 8));
    RCCHK(d2h(h, diff_out, b.diff, n * 8));
    HIPCHK(hipStreamSynchronize(h->stream));
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
    float *s_sig;
    RCCHK(ws_carve(h, [&](Carve &w) {
        s_sig = w.take<float>((size_t)m * n_reads, !(flags & ADP_IN_DEVICE));
        af_pieces(w, b, n_reads, m, (flags & ADP_OUT_DEVICE) != 0);
    }));
    const float *ds;
    RCCHK(stage_in(h, flags, sig, s_sig, (size_t)m * 4 * n_reads, &ds));
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
