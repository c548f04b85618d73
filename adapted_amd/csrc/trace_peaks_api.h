// trace_peaks_api.h -- the reference's Python LLR module (adapted/detect/llr.py) above its native one, as batched device
// operators with every parameter (the fused detect path's k_adapter_peak / k_polya_peak hard-code them, peaks.h):
//
//   k_trace_bounds      LLRTrace: _trace_start_end, early_stop, interp_stride       llr.py:53-142
//   k_trace_blocksum    per-64 block max / min of the traces (the cooperative walks' summaries; k_gains leaves them on the
//                     fused path)
//   k_trace_peaks       find_peaks_in_trace + correct_for_plateau + correct_for_split_peak, EVERY peak   llr.py:145-248
//   k_trace_spike       detect_full_polya_trace_peak_with_spike                      llr.py:406-479
//
// One wave per read throughout.  The find_peaks restatement (local maxima, prominence and width walks, cooperative long
// walks) is peaks.h's, unchanged; what differs from the fused kernels: the peaks kernel evaluates every strict local maximum
// of the clip and keeps every survivor (not the first), computes np.nanstd of the clip in numpy's summation order (the fused
// kernel's one-pass moments may move a threshold by an ulp), and the spike kernel's minimum-distance selection takes any
// distance: its fixed point walks each maximum's neighbours by position instead of a fixed 4-ordinal window.
#pragma once
#include "common.h"
#include "find_peaks.h"
#include "np_sum.h"

// np.nanstd(x[lo:hi]) (numpy/lib/_nanfunctions_impl.py _nanvar: NaNs -> 0, the mean over the non-NaN count, squared
// deviations with the NaN slots zeroed again, ddof 0); NaN for an empty or all-NaN slice
static __device__ double np_nanstd_wave(const double *x, long lo, long hi, LDS NpSumLds *s)
{
    const long n = hi - lo;
    if (n <= 0) return __builtin_nan("");
    int c = 0;
    for (long i = lo + lane_id(); i < hi; i += 64) c += (x[i] == x[i]);
    const long cnt = wave_sum(c);
    const double avg = np_sum_wave(n, [&](long k) { const double v = x[lo + k]; return v == v ? v : 0.0; }, s) / (double)cnt;
    const double var = np_sum_wave(n, [&](long k) { const double v = x[lo + k]; if (v != v) return 0.0; const double d = v - avg; return d * d; }, s)
                       / (double)cnt;
    if (cnt == 0) return __builtin_nan("");
    return sqrt(var);
}

// ---------------------------------------------------------------- B: LLRTrace bounds, early stop, stride interpolation
// start = np.argmin(signal <= 0), end = size - np.argmin(signal[::-1] <= 0) - 1 (NaN counts as positive; 0 and size - 1 when
// every value is <= 0); early_stop = end < np.arange(min_obs, size - 1 - tail_trim, stride)[-1] (size - 1 - tail_trim for an
// empty range); with ADP_LLR_INTERP and stride > 1, interp_stride in place: np.interp(arange(size), knots, signal[knots], left=0,
// right=0) with knots = the indices in [start, end) whose value is != 0 (NaN included).  Every output position has its own
// formula (numpy's arr_interp: slope = (y1 - y0) / (x1 - x0), slope * (x - x0) + y0, retried from the right knot when NaN,
// then y0 when both knots are equal), so the lanes take 64 positions at a time; the knots around them come from a ballot,
// the nearest knots outside the tile are carried (a stored value is never a knot's: only positions between knots change).
// early_stop_out bit 1: the knot set was empty (numpy raises; the trace is left as it was).  grid = n_reads, block = 64.
__global__ void __launch_bounds__(64) k_trace_bounds(double *__restrict__ trace, const int32_t *__restrict__ len, int L,
                                                   const int32_t *__restrict__ min_obs, const int32_t *__restrict__ tail_trim, int stride,
                                                   int interp, int32_t *__restrict__ start_out, int32_t *__restrict__ end_out,
                                                   int32_t *__restrict__ es_out)
{
    const int r = blockIdx.x, ln = lane_id();
    const int n = len[r];
    double *g = trace + (size_t)r * L;
    if (n < 1) { if (ln == 0) { start_out[r] = 0; end_out[r] = -1; es_out[r] = 0; } return; }
    int start = -1, end = -1;
    for (int b = 0; b < n && start < 0; b += 64) {
        const int i = b + ln;
        const unsigned long long m = __ballot(i < n && !(g[i] <= 0.0));
        if (m) start = b + __ffsll((long long)m) - 1;
    }
    for (int b = n - 1; b >= 0 && end < 0; b -= 64) {
        const int i = b - ln;
        const unsigned long long m = __ballot(i >= 0 && !(g[i] <= 0.0));
        if (m) end = b - (__ffsll((long long)m) - 1);
    }
    if (start < 0) { start = 0; end = n - 1; }
    const long hi = (long)n - 1 - tail_trim[r], mo = min_obs[r];
    const long mlnes = hi > mo ? mo + ((hi - mo - 1) / stride) * stride : hi;
    int es = (long)end < mlnes ? 1 : 0;
    if (interp && stride > 1) {
        // is the knot set empty?  (numpy raises: the trace stays as it was)
        bool any = false;
        for (int c = start; c < end && !any; c += 64) {
            const int j = c + ln;
            any = __ballot(j < end && g[j] != 0.0) != 0ull;
        }
        if (!any) es |= 2;
        int kp = -1, kn = -1;  // carried: the last knot below the tile; the first knot at or beyond the tile's end (-1: not
        double yp = 0.0, yn = 0.0; // searched yet, 0x7fffffff: none)
        for (int b = 0; any && b < n; b += 64) {
            const int i = b + ln;
            const double v = i < n ? g[i] : 0.0;
            const bool isk = i >= start && i < end && v != 0.0;
            const unsigned long long mk = __ballot(isk);
            const unsigned long long below = mk & ((2ull << ln) - 1ull); // (ln = 63: every bit)
            const unsigned long long above = mk & ~((2ull << ln) - 1ull);
            // (shuffles from every lane alike; the lanes pick what applies to them)
            const double vb = __shfl(v, below ? 63 - __clzll((long long)below) : 0);
            const double va = __shfl(v, above ? __ffsll((long long)above) - 1 : 0);
            int p0 = below ? b + 63 - __clzll((long long)below) : kp;
            double y0 = below ? vb : yp;
            int p1 = above ? b + __ffsll((long long)above) - 1 : -1;
            double y1 = above ? va : 0.0;
            // the first knot at or beyond b + 64, for the lanes above the tile's last knot
            if (__ballot(i < n && !isk && !above && p0 >= 0)) {
                if (kn != 0x7fffffff && kn < b + 64) {
                    kn = 0x7fffffff;
                    for (int c = b + 64; c < end && kn == 0x7fffffff; c += 64) {
                        const int j = c + ln;
                        const double w = j < end ? g[j] : 0.0;
                        const unsigned long long m2 = __ballot(j < end && w != 0.0);
                        const double wf = __shfl(w, m2 ? __ffsll((long long)m2) - 1 : 0);
                        if (m2) { kn = c + __ffsll((long long)m2) - 1; yn = wf; }
                    }
                }
                if (!above && kn != 0x7fffffff) { p1 = kn; y1 = yn; }
            }
            if (i < n && !isk) {
                double res = 0.0;
                if (p0 >= 0 && p1 >= 0) {
                    const double slope = (y1 - y0) / ((double)p1 - (double)p0);
                    res = slope * ((double)i - (double)p0) + y0;
                    if (res != res) {
                        res = slope * ((double)i - (double)p1) + y1;
                        if (res != res && y0 == y1) res = y0;
                    }
                }
                g[i] = res;
            }
            const double vl = __shfl(v, mk ? 63 - __clzll((long long)mk) : 0);
            if (mk) { kp = b + 63 - __clzll((long long)mk); yp = vl; }
        }
    }
    if (ln == 0) { start_out[r] = start; end_out[r] = end; es_out[r] = es; }
}

// ---------------------------------------------------------------- block summaries
// per-64 block max / min of each read's trace (TraceViewT::bmax / bmin: NaN -> +inf in the max, ignored by the min), or of
// np.nan_to_num(trace) with `sanitize` (the view find_peaks sees in the spike test).  grid = (n_reads), block = 64.
__global__ void __launch_bounds__(64) k_trace_blocksum(const double *__restrict__ trace, const int32_t *__restrict__ len, int L, int nsum,
                                                     int sanitize, double *__restrict__ bmax, double *__restrict__ bmin)
{
    const int r = blockIdx.x, ln = lane_id();
    const int n = len[r];
    const TraceView tv{trace + (size_t)r * L, nullptr, nullptr, 0, n - 1, sanitize};
    const int nb = (n + SUMBLK - 1) / SUMBLK;
    for (int b0 = 0; b0 < nb; b0 += 4) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = (b0 + u) * SUMBLK + ln; v[u] = (b0 + u < nb && i < n) ? tv_get(tv, i) : __builtin_nan(""); }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (b0 + u >= nb) break;
            const double mx = wave_max(v[u] != v[u] ? (((b0 + u) * SUMBLK + ln) < n ? __builtin_inf() : -__builtin_inf()) : v[u]);
            const double mn = wave_min(v[u] != v[u] ? __builtin_inf() : v[u]);
            if (ln == 0) { bmax[(size_t)r * nsum + b0 + u] = mx; bmin[(size_t)r * nsum + b0 + u] = mn; }
        }
    }
}

// ---------------------------------------------------------------- K: every adapter-end peak
// correct_for_plateau (llr.py:145-177) for any s >= 1, t, window: the largest i in [0, nch - s] (nch = len(np.diff(window))) whose
// s - 1 changes from i on are all >= 0 and with w[i + s - 1] > t w[0]; peak + i + s - 1 when that is > 0.  The lanes take 64 i at a
// time from the top; "the first change < 0 at or after i" is carried down from the tiles above.  Uniform call.
static __device__ int llr_plateau(const double *g, int n, int peak, int s, double t, int window)
{
    const int ln = lane_id();
    const long wend = (long)peak + window < (long)n ? (long)peak + window : (long)n;
    const int wn = wend > peak ? (int)(wend - peak) : 0;
    const int nch = wn > 0 ? wn - 1 : 0;
    if (nch - s < 0) return peak;
    const double *w = g + peak;
    const double thr = t * w[0];
    int nbad = 0x7fffffff; // the lowest j above the tile with changes[j] < 0 (or NaN)
    for (int top = nch - 1; top >= 0; top -= 64) {
        const int j = top - ln;
        const bool bad = j >= 0 && !(w[j + 1] - w[j] >= 0.0);
        const unsigned long long mb = __ballot(bad);
        // the first bad change at or after j: the highest lane <= ln with a bad change, else the carried one
        const unsigned long long le = mb & ((2ull << ln) - 1ull);
        const int nb = le ? top - (63 - __clzll((long long)le)) : nbad;
        const bool ok = j >= 0 && j <= nch - s && (long)nb >= (long)j + s - 1 && w[j + s - 1] > thr;
        const unsigned long long mo = __ballot(ok);
        if (mo) {
            const int i = top - (__ffsll((long long)mo) - 1);
            return (i + s - 1 > 0) ? peak + i + s - 1 : peak;
        }
        if (mb) nbad = top - (63 - __clzll((long long)mb));
    }
    return peak;
}

// k_trace_peaks: per read r, find_peaks(trace[clip_lo:clip_hi], prominence=prominence * np.nanstd(clip), width, rel_height) --
// EVERY peak, in index order -- each then corrected by correct_for_plateau and correct_for_split_peak as the args ask.
// peaks_out [n_reads, cap] (full-trace indices, -1 padding), count_out [n_reads]: the true count, also past cap.
// given (ADP_LLR_GIVEN_PEAK): clip_lo[r] is a peak to correct, no search.  bmax / bmin: k_trace_blocksum's summaries of the raw
// trace.  grid = n_reads, block = 64.
__global__ void __launch_bounds__(64) k_trace_peaks(const double *__restrict__ trace, const int32_t *__restrict__ len, int L,
                                                  const int32_t *__restrict__ clip_lo, const int32_t *__restrict__ clip_hi,
                                                  const double *__restrict__ bmax, const double *__restrict__ bmin, int nsum,
                                                  adp_peak_args a, int given, int cap, int64_t *__restrict__ peaks_out,
                                                  int64_t *__restrict__ count_out)
{
    __shared__ NpSumLds sred_;
    LDS NpSumLds *sred = (LDS NpSumLds *)&sred_;
    const int r = blockIdx.x, ln = lane_id();
    const int n = len[r], lo = clip_lo[r], hi = clip_hi[r];
    const double *g = trace + (size_t)r * L;
    const double *bx = bmax + (size_t)r * nsum, *bn = bmin + (size_t)r * nsum;
    for (int k = ln; k < cap; k += 64) peaks_out[(size_t)r * cap + k] = -1;
    long count = 0;
    // (given: clip_lo is a peak of the caller's -- correct_for_plateau / correct_for_split_peak on their own)
    auto correct = [&](int peak) {
        if (a.plateau_on) peak = llr_plateau(g, n, peak, a.plateau_s, a.plateau_t, a.plateau_window);
        if (a.split_on) {
            // correct_for_split_peak (llr.py:180-201): find_peaks(trace[peak:peak + window], width=s, prominence)[0]
            const long wend = (long)peak + a.split_window < (long)n ? (long)peak + a.split_window : (long)n;
            if (wend - peak >= 3) {
                const TraceView tw{g, bx, bn, peak, (int)wend - 1, 0};
                const int pk = wave_first_peak(tw, a.split_prominence, (double)a.split_s, 0.5);
                if (pk >= 0 && g[pk] >= a.split_t * g[peak]) peak = pk;
            }
        }
        return peak;
    };
    if (given) {
        const int peak = correct(lo);
        if (ln == 0) { peaks_out[(size_t)r * cap] = peak; count_out[r] = 1; }
        return;
    }
    if (hi - lo >= 3) {
        const double pmin = a.prominence * np_nanstd_wave(g, lo, hi, sred);
        const TraceView tv{g, bx, bn, lo, hi - 1, 0};
        for (int base = lo + 1; base < hi - 1; base += 64) {
            const int i = base + ln;
            const int p = (i < hi - 1) ? tv_peak_at(tv, i) : -1;
            unsigned long long mk = __ballot(wave_peak_ok(tv, p, pmin, a.width, a.rel_height));
            while (mk) {
                const int f = __ffsll((long long)mk) - 1;
                mk &= mk - 1;
                const int peak = correct(__shfl(p, f));
                if (ln == 0 && count < cap) peaks_out[(size_t)r * cap + count] = peak;
                count++;
            }
        }
    }
    if (ln == 0) count_out[r] = count;
}

// ---------------------------------------------------------------- S: the poly(A) end with a spike
// detect_full_polya_trace_peak_with_spike (llr.py:406-479): find_peaks(np.nan_to_num(trace, nan=0), distance, prominence, width,
// rel_height=0.5), then the two-peak heuristics on the UN-sanitised trace.
//   1. the strict local maxima, in index order, into pk (per-read scratch of len / 2 + 1 entries; bits 30-31: state);
//   2. scipy's _select_by_peak_distance as its fixed point "kept iff no kept higher-priority maximum within D = ceil(distance)
//      samples" (priority: height, then the LATER index -- the tie order of orc_find_peaks and k_polya_peak): rounds over a work
//      list of the undecided maxima, each looking at its neighbours by position (|dp| < D) -- any D;
//   3. the first two kept maxima (index order) with prominence and width;
//   4. the ratio test, then np.argmin and linregress's r, as k_polya_peak's step 5.
// bmax / bmin: summaries of the SANITISED trace.  wl: per-read work list, len / 2 + 1 entries.  grid = n_reads, block = 64.
#define SPK_UND 3u
#define SPK_KEPT 2u
#define SPK_REM 1u
__global__ void __launch_bounds__(64) k_trace_spike(const double *__restrict__ trace, const int32_t *__restrict__ len, int L,
                                                  const double *__restrict__ bmax, const double *__restrict__ bmin, int nsum,
                                                  adp_spike_args a, int dist, uint32_t *__restrict__ pk_all, uint32_t *__restrict__ wl_all,
                                                  int half, int64_t *__restrict__ out)
{
    const int r = blockIdx.x, ln = lane_id();
    const int n = len[r];
    const double *g = trace + (size_t)r * L;
    uint32_t *pk = pk_all + (size_t)r * half, *wl = wl_all + (size_t)r * half;
    long result = 0;
    if (n >= 3) {
        const TraceView tv{g, bmax + (size_t)r * nsum, bmin + (size_t)r * nsum, 0, n - 1, 1};
        // 1.
        int npk = 0;
        for (int base = 1; base < n - 1; base += 64) {
            const int i = base + ln;
            const int p = (i < n - 1) ? tv_peak_at(tv, i) : -1;
            const unsigned long long m = __ballot(p >= 0);
            if (p >= 0) {
                const int k = npk + __popcll(m & ((1ull << ln) - 1ull));
                pk[k] = (uint32_t)p | (SPK_UND << 30);
                wl[k] = (uint32_t)k;
            }
            npk += __popcll(m);
        }
        __syncthreads();
        // 2.
        int nund = npk;
        while (nund > 0) {
            int w = 0;
            for (int base = 0; base < nund; base += 64) {
                const int idx = base + ln;
                bool pending = false;
                uint32_t k = 0;
                if (idx < nund) {
                    k = wl[idx];
                    const int p = (int)(pk[k] & 0x3fffffffu);
                    const double h = tv_get(tv, p);
                    bool kept_nb = false;
                    for (int j = (int)k - 1; j >= 0 && !kept_nb; j--) {
                        const uint32_t e = pk[j];
                        if (p - (int)(e & 0x3fffffffu) >= dist) break;
                        if (tv_get(tv, (int)(e & 0x3fffffffu)) > h) { // (earlier index: higher only when strictly higher)
                            const uint32_t st = e >> 30;
                            if (st == SPK_KEPT) kept_nb = true; else if (st == SPK_UND) pending = true;
                        }
                    }
                    for (int j = (int)k + 1; j < npk && !kept_nb; j++) {
                        const uint32_t e = pk[j];
                        if ((int)(e & 0x3fffffffu) - p >= dist) break;
                        if (tv_get(tv, (int)(e & 0x3fffffffu)) >= h) { // (later index: higher on equal heights too)
                            const uint32_t st = e >> 30;
                            if (st == SPK_KEPT) kept_nb = true; else if (st == SPK_UND) pending = true;
                        }
                    }
                    if (kept_nb) { pk[k] = (uint32_t)p | (SPK_REM << 30); pending = false; }
                    else if (!pending) pk[k] = (uint32_t)p | (SPK_KEPT << 30);
                }
                const unsigned long long m = __ballot(pending);
                __syncthreads(); // (this tile's list entries are read before any is overwritten)
                if (pending) wl[w + __popcll(m & ((1ull << ln) - 1ull))] = k;
                w += __popcll(m);
                __syncthreads();
            }
            if (w == nund) break; // (cannot happen: the highest undecided maximum is decided in every round)
            nund = w;
        }
        // 3.
        int p0 = -1, p1 = -1;
        for (int base = 0; base < npk && p1 < 0; base += 64) {
            const int k = base + ln;
            const uint32_t e = k < npk ? pk[k] : 0u;
            const int p = (k < npk && (e >> 30) == SPK_KEPT) ? (int)(e & 0x3fffffffu) : -1;
            unsigned long long m = __ballot(wave_peak_ok(tv, p, a.prominence_threshold, a.min_width, 0.5));
            while (m && p1 < 0) {
                const int f = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int pi = __shfl(p, f);
                if (p0 < 0) p0 = pi; else p1 = pi;
            }
        }
        // 4.
        if (p0 >= 0 && p1 < 0) result = p0;
        else if (p0 >= 0) {
            const double h0 = g[p0], h1 = g[p1];
            if (h1 > h0) result = p1;
            else if (h1 < h0 * a.threshold_prominence_ratio) result = p0;
            else {
                // idx_min = argmin(g[p0:p1]) (first minimum; a NaN wins)
                double mv = __builtin_inf(); int mi = 0x7fffffff, nan_i = 0x7fffffff;
                for (int i = p0 + ln; i < p1; i += 64) {
                    const double v = g[i];
                    if (v != v) nan_i = min(nan_i, i);
                    else if (v < mv) { mv = v; mi = i; }
                }
                nan_i = wave_min(nan_i);
                const double gm = wave_min(mv);
                int cand = wave_min((mv == gm) ? mi : 0x7fffffff);
                int idx_min = (nan_i != 0x7fffffff) ? nan_i : cand;
                if (idx_min == 0x7fffffff) idx_min = p0; // all +inf: np.argmin -> 0
                const int cnt = p1 - idx_min;
                // scipy.stats.linregress's r
                double sx = 0, sy = 0;
                for (int i = idx_min + ln; i < p1; i += 64) { sx += (double)i; sy += g[i]; }
                sx = wave_sum(sx); sy = wave_sum(sy);
                const double xm = sx / cnt, ym = sy / cnt;
                double sxx = 0, sxy = 0, syy = 0;
                for (int i = idx_min + ln; i < p1; i += 64) {
                    const double dx = (double)i - xm, dy = g[i] - ym;
                    sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
                }
                sxx = wave_sum(sxx); sxy = wave_sum(sxy); syy = wave_sum(syy);
                const double inv = 1.0 / (double)cnt;
                const double ssxm = sxx * inv, ssxym = sxy * inv, ssym = syy * inv;
                double rr;
                if (ssxm == 0.0 || ssym == 0.0) rr = 0.0;
                else { rr = ssxym / sqrt(ssxm * ssym); if (rr > 1.0) rr = 1.0; else if (rr < -1.0) rr = -1.0; }
                result = (rr * rr >= a.threshold_r_squared) ? p1 : 0;
            }
        }
    }
    if (ln == 0) out[r] = result;
}
