// events_api.h -- event segmentation of signal segments (an extension: the reference's README sends its users to another
// tool for it, "Poly(A) tail length estimation"), batched: the boundaries between the events of signal[row, start:end] and
// the median / median absolute deviation of the event lengths, which turn the adapter's length in samples into a
// translocation speed.  Compiled in modules.hip only.  Two kernels per batch of slots:
//
//   k_ev_scores   the squared two-window t-statistic of every position, float64 whatever the samples' type, in a fixed
//                 order of operations (so that a numpy restatement is its exact oracle, tests/events_oracle.py):
//                   mean[j] = (x[j] + ... + x[j + w - 1]) / w          (summed left to right)
//                   var[j]  = (sum of (x[j + k] - mean[j])^2) / w
//                   score[i] = ((mean[i - w] - mean[i])^2 * w) / max(var[i - w] + var[i], var_floor)   for w <= i <= n - w, else 0
//                 windowed sums, not differences of a running sum: no chain over the read and no cancellation on long ones.
//                 One workgroup per tile of EV_TILE positions: the tile's samples plus a halo of 2 w - 1 go to LDS once
//                 (widened), then the window statistics of its EV_TILE + w window starts, then the scores.
//   k_ev_bounds   scipy.signal.find_peaks(score, height=thr, distance=D)[0], one wave per segment: find_peaks.h's strict local
//                 maxima (plateau midpoints), the height test, then scipy's _select_by_peak_distance as the fixed point
//                 k_trace_spike uses (trace_peaks_api.h: any distance; on equal heights the later index is the higher).  Then
//                 np.median and the median absolute deviation of np.diff(boundaries): radix selections on integer keys with
//                 the histogram in LDS (the gaps themselves for the median; |2 gap - (a + b)| for the deviations about the
//                 median (a + b) / 2, so that a half-integer median needs no floating point -- every value is exact).
//                 Cost of the distance rule: every round decides at least the highest undecided maximum and usually most of
//                 them, but a run of c candidates with rising heights, each within D of the next, is decided one per round
//                 from its top: c rounds over a shrinking list, O(c^2) dependent loads in one wave (k_trace_spike's bound
//                 too).  Event scores alternate, so real adapters take a few rounds; a monotone ramp of tens of thousands of
//                 candidates would take seconds.  Heights are re-read from the scores for every neighbour (L2 hits).
#pragma once
#include "common.h"
#include "find_peaks.h"
#include "sigstats_api.h" // (ss_hist_add, ss_pick)

#define EV_TILE 1024  // positions per workgroup of k_ev_scores
#define EV_WMAX 64    // the longest window
#define EV_BLOCK 256
#define EV_SCRATCH_MIB 512 // a call's scores and lists of maxima: the default byte budget of its batch of slots (modules.hip)

// a segment as the kernels take it: the clipped slice's first sample (an element offset into the signals) and its size
struct EvSeg { long long off; int32_t n, pad; };

// Where the kernels' samples come from, their template parameter: src.seg(g, off)[k] is sample k of segment g, whose slice starts
// at element `off` of the signals, widened to a double.  EvPlain<float> / EvPlain<double>: the signals as they are.  EvI16: raw
// int16 ADC samples packed back to back and a calibration per SEGMENT, pA = scale[g] * (float32(adc) + offset[g]) as RowI16
// states it (common.h: the bits of adp_calibrate_i16).  A packed slice starts at any element, so the samples are loaded one by
// one (2-byte aligned; RowI16's vector forms want 8-byte rows); a calibration that is not finite makes NaN samples.
template <class T> struct EvPlain {
    const T *sig;
    struct Seg {
        const T *x;
        __device__ __forceinline__ double operator[](long long k) const { return (double)x[k]; }
    };
    __device__ __forceinline__ Seg seg(int, long long off) const { return Seg{sig + off}; }
};
struct EvI16 {
    const int16_t *raw;
    const float *scale, *offset;
    struct Seg {
        RowI16 r;
        __device__ __forceinline__ double operator[](long long k) const { return (double)r.cook1(r.raw1(k)); }
    };
    __device__ __forceinline__ Seg seg(int g, long long off) const { return Seg{RowI16{(const GLB int16_t *)raw + off, scale[g], offset[g], 0}}; }
};

// grid = (tiles of the longest segment of the batch, slots), block = EV_BLOCK.  Slot s holds segment g0 + s; score: [slots, stride].
// nanflag[g] (zeroed by the caller) is set when the slice holds a NaN.
template <class Src>
__global__ void __launch_bounds__(EV_BLOCK) k_ev_scores(const Src src, const EvSeg *__restrict__ segs, int g0, int w,
                                                      double var_floor, size_t stride, double *__restrict__ score,
                                                      int32_t *__restrict__ nanflag)
{
    __shared__ __attribute__((aligned(16))) double sx[EV_TILE + 2 * EV_WMAX];
    __shared__ __attribute__((aligned(16))) double sm[EV_TILE + EV_WMAX];
    __shared__ __attribute__((aligned(16))) double sv[EV_TILE + EV_WMAX];
    const int s = blockIdx.y, g = g0 + s, t = threadIdx.x;
    const int n = segs[g].n;
    const int t0 = blockIdx.x * EV_TILE;
    if (t0 >= n) return;
    const auto x = src.seg(g, segs[g].off);
    // the samples [lo, hi) behind this tile's scores
    const int lo = t0 > w ? t0 - w : 0;
    const int hi = (long long)t0 + EV_TILE + w - 1 < (long long)n ? t0 + EV_TILE + w - 1 : n;
    bool bad = false;
    for (int k = t; k < hi - lo; k += EV_BLOCK) {
        const double v = x[lo + k];
        sx[k] = v;
        bad |= v != v;
    }
    if (__syncthreads_or(bad) && t == 0) nanflag[g] = 1;
    // the window starts [lo, jhi): every j <= n - w whose window lies in [lo, hi)
    const int jhi = t0 + EV_TILE < n - w + 1 ? t0 + EV_TILE : n - w + 1;
    const double wd = (double)w;
    for (int k = t; k < jhi - lo; k += EV_BLOCK) {
        double sum = 0.0;
        for (int q = 0; q < w; q++) sum = sum + sx[k + q];
        const double mean = sum / wd;
        double sq = 0.0;
        for (int q = 0; q < w; q++) { const double d = sx[k + q] - mean; sq = sq + d * d; }
        sm[k] = mean;
        sv[k] = sq / wd;
    }
    __syncthreads();
    double *o = score + (size_t)s * stride;
    for (int k = t; k < EV_TILE && t0 + k < n; k += EV_BLOCK) {
        const int i = t0 + k;
        double sc = 0.0;
        if (i >= w && i <= n - w) {
            const double d = sm[i - w - lo] - sm[i - lo];
            double den = sv[i - w - lo] + sv[i - lo];
            if (den < var_floor) den = var_floor;
            sc = ((d * d) * wd) / den;
        }
        o[i] = sc;
    }
}

// the key of rank `rank` (0-based, ascending) among key(0), ..., key(m - 1), every key below 2^(8 passes): MSB-first radix
// selection, 8 bits per pass, the histogram in LDS.  Uniform call of a one-wave workgroup; every lane gets the key.
template <class F>
static __device__ uint32_t ev_select(int m, int rank, int passes, F key, LDS uint32_t *hist)
{
    const int ln = lane_id();
    uint32_t pre = 0, mask = 0;
    int r = rank;
    for (int pass = passes - 1; pass >= 0; pass--) {
        const int shift = 8 * pass;
        __syncthreads();
        for (int q = ln; q < 256; q += 64) hist[q] = 0;
        __syncthreads();
        for (int base = 0; base < m; base += 64) {
            const int k = base + ln;
            const bool act = k < m;
            const uint32_t v = act ? key(k) : 0u;
            ss_hist_add(hist, act && (v & mask) == pre, (v >> shift) & 255u);
        }
        __syncthreads();
        int bin, below, total;
        ss_pick(hist, r, bin, below, total);
        pre |= (uint32_t)bin << shift;
        mask |= 255u << shift;
        r -= below;
    }
    return pre;
}

#define EV_UND 3u
#define EV_KEPT 2u
#define EV_REM 1u
// grid = slots, block = 64.  pk_all / wl_all: per-slot scratch of `half` entries (a slice of n samples has fewer than n / 2 + 1
// strict local maxima; bits 30-31 of a pk entry: its state).  pos [n_seg, cap] (positions from the clipped slice's start, ascending,
// then -1), info [n_seg, 2] (the number of boundaries, also past cap; status: 0, 1 a NaN in the slice, 2 n < 2 w), stats [n_seg, 2]
// (median and MAD of the gaps; NaN with fewer than two boundaries).
__global__ void __launch_bounds__(64) k_ev_bounds(const double *__restrict__ score, size_t stride, const EvSeg *__restrict__ segs, int g0,
                                                int w, int dist, double thr, int cap, uint32_t *pk_all, uint32_t *wl_all, int half,
                                                const int32_t *__restrict__ nanflag, int64_t *__restrict__ pos, int64_t *__restrict__ info,
                                                double *__restrict__ stats)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist_[256];
    LDS uint32_t *hist = (LDS uint32_t *)hist_;
    const int s = blockIdx.x, g = g0 + s, ln = lane_id();
    const int n = segs[g].n;
    uint32_t *pk = pk_all + (size_t)s * half, *wl = wl_all + (size_t)s * half;
    int64_t *op = pos + (size_t)g * cap;
    for (int k = ln; k < cap; k += 64) op[k] = -1;
    double med = __builtin_nan(""), mad = __builtin_nan("");
    int nk = 0, status = 0;
    if (nanflag[g]) status = 1;
    else if (n < 2 * w) status = 2;
    else {
        const TraceView tv{score + (size_t)s * stride, nullptr, nullptr, 0, n - 1, 0};
        // the strict local maxima at or above thr, in index order
        int npk = 0;
        for (int base = 1; base < n - 1; base += 64) {
            const int i = base + ln;
            int p = (i < n - 1) ? tv_peak_at(tv, i) : -1;
            if (p >= 0 && !(tv_get(tv, p) >= thr)) p = -1;
            const unsigned long long m = __ballot(p >= 0);
            if (p >= 0) {
                const int k = npk + __popcll(m & ((1ull << ln) - 1ull));
                pk[k] = (uint32_t)p | (EV_UND << 30);
                wl[k] = (uint32_t)k;
            }
            npk += __popcll(m);
        }
        __syncthreads();
        // kept iff no kept higher maximum within dist samples: rounds over the work list of the undecided
        int nund = npk;
        while (nund > 0) {
            int nw = 0;
            for (int base = 0; base < nund; base += 64) {
                const int idx = base + ln;
                bool pending = false;
                uint32_t k = 0;
                if (idx < nund) {
                    k = wl[idx];
                    const int p = (int)(pk[k] & 0x3fffffffu);
                    const double hgt = tv_get(tv, p);
                    bool kept_nb = false;
                    for (int j = (int)k - 1; j >= 0 && !kept_nb; j--) {
                        const uint32_t e = pk[j];
                        if (p - (int)(e & 0x3fffffffu) >= dist) break;
                        if (tv_get(tv, (int)(e & 0x3fffffffu)) > hgt) { // (earlier index: higher only when strictly higher)
                            const uint32_t st = e >> 30;
                            if (st == EV_KEPT) kept_nb = true; else if (st == EV_UND) pending = true;
                        }
                    }
                    for (int j = (int)k + 1; j < npk && !kept_nb; j++) {
                        const uint32_t e = pk[j];
                        if ((int)(e & 0x3fffffffu) - p >= dist) break;
                        if (tv_get(tv, (int)(e & 0x3fffffffu)) >= hgt) { // (later index: higher on equal heights too)
                            const uint32_t st = e >> 30;
                            if (st == EV_KEPT) kept_nb = true; else if (st == EV_UND) pending = true;
                        }
                    }
                    if (kept_nb) { pk[k] = (uint32_t)p | (EV_REM << 30); pending = false; }
                    else if (!pending) pk[k] = (uint32_t)p | (EV_KEPT << 30);
                }
                const unsigned long long m = __ballot(pending);
                __syncthreads(); // (this tile's list entries are read before any is overwritten)
                if (pending) wl[nw + __popcll(m & ((1ull << ln) - 1ull))] = k;
                nw += __popcll(m);
                __syncthreads();
            }
            if (nw == nund) break; // (cannot happen: the highest undecided maximum is decided in every round)
            nund = nw;
        }
        __syncthreads();
        // the kept maxima, compacted in index order: the boundaries (wl: entry k <- an entry at or above k)
        for (int base = 0; base < npk; base += 64) {
            const int k = base + ln;
            const uint32_t e = k < npk ? pk[k] : 0u;
            const bool kept = k < npk && (e >> 30) == EV_KEPT;
            const unsigned long long m = __ballot(kept);
            if (kept) {
                const int q = nk + __popcll(m & ((1ull << ln) - 1ull));
                wl[q] = e & 0x3fffffffu;
                if (q < cap) op[q] = (int64_t)(e & 0x3fffffffu);
            }
            nk += __popcll(m);
        }
        __syncthreads();
        if (nk >= 2) {
            const int m = nk - 1; // gaps, each in [1, n): doubled deviations below 2 n
            const int passes = (32 - __clz((int)(2u * (unsigned)n)) + 7) / 8; // (n < 2^30)
            auto gap = [&](int k) { return wl[k + 1] - wl[k]; };
            const uint32_t a = ev_select(m, (m - 1) / 2, passes, gap, hist);
            const uint32_t b = (m & 1) ? a : ev_select(m, m / 2, passes, gap, hist);
            med = ((double)a + (double)b) / 2.0;
            const int ab = (int)(a + b);
            auto dev = [&](int k) { const int d = 2 * (int)gap(k) - ab; return (uint32_t)(d < 0 ? -d : d); };
            const uint32_t c = ev_select(m, (m - 1) / 2, passes, dev, hist);
            const uint32_t d = (m & 1) ? c : ev_select(m, m / 2, passes, dev, hist);
            mad = ((double)c + (double)d) / 4.0;
        }
    }
    if (ln == 0) {
        info[(size_t)g * 2] = nk;
        info[(size_t)g * 2 + 1] = status;
        stats[(size_t)g * 2] = med;
        stats[(size_t)g * 2 + 1] = mad;
    }
}
