// sigstats_api.h -- the reference's signal statistics modules for batches of float32 or float64 rows: partition statistics
// (adapted/partition/signal_partitions.py: np.mean, np.std, np.median and the median absolute deviation of signal[start:end]),
// median / MAD normalisation (detect/normalize.py), average pooling (detect/downscale.py), the real-range check
// (detect/real_range.py) and the open-pore positions (detect/anomalies.py).  Statistics of a segment or a row: one workgroup
// each (SS_BLOCK threads); median and MAD of one large population: many workgroups (k_pop_*).  Compiled in modules.hip only.
//
//   * selection core (ss_select2): MSB-first radix select on order-preserving integer keys, 8 bits per pass -- 4 passes for
//     float32, 8 for float64, whatever the values (a quantised or constant segment only means that the next pass looks at the
//     same samples again) -- templated on the element type and on a key functor: the sample itself, or |x - c| taken on load, so
//     that the MAD needs no array of deviations.  Both middles of an even count are followed through the same passes: one
//     histogram while their prefixes agree, two from the pass in which they part.  Pass 0 also reports a NaN among the keys.
//   * summation core: np_sum.h's np_sum_wave, numpy's add.reduce order with accumulators of the element type.
//
// A segment is read from global memory in every pass (2 sums + 2 selections: 10 passes in float32, 18 in float64); the
// partitions of one read are at most a few hundred KiB, so all passes but the first are served by the L2 / the MALL.
//   * one population larger than a wave should walk alone (the whole [N, m] minibatch of normalize_signal): the same selection
//     with the histogram of each pass gathered by many workgroups -- per-workgroup LDS histograms, flushed with vector atomics
//     to a global one (k_pop_hist) -- and a one-wave kernel that picks the bins and keeps the state on the device (k_pop_pick).
#pragma once
#include "common.h"
#include "np_sum.h"
#include "wave_stats.h" // (ws_sync)

template <class T> struct SsKey;
template <> struct SsKey<float> {
    typedef uint32_t type;
    static __device__ __forceinline__ uint32_t of(float v) { return f2key(v); }
    static __device__ __forceinline__ float back(uint32_t k) { return key2f(k); }
};
template <> struct SsKey<double> {
    typedef uint64_t type;
    static __device__ __forceinline__ uint64_t of(double v) { return d2key(v); }
    static __device__ __forceinline__ double back(uint64_t k) { return key2d(k); }
};

static __device__ __forceinline__ float ss_abs(float v) { return __builtin_fabsf(v); }
static __device__ __forceinline__ double ss_abs(double v) { return __builtin_fabs(v); }

// the key functors of the selection
template <class T> struct SsIdent { __device__ __forceinline__ T operator()(T v) const { return v; } };
template <class T> struct SsAbsDev {
    T c;
    __device__ __forceinline__ T operator()(T v) const { return ss_abs(v - c); } // (NaN stays NaN)
};

struct SsLds { uint32_t hist[2][256]; uint32_t nan; };
#define SS_BLOCK 256 // threads of the workgroup that takes a segment's or a row's statistics
// (the selections' histograms and the sums' state are never in use together: one piece of LDS serves both)
template <class T> union SsScratch { SsLds sel; NpSumLdsT<T> sum; };

// one sample into a histogram: `m` says whether this lane has one, `d` its digit.  When every lane that has one has the same
// digit (the usual case for the leading bytes, and for any byte of a constant stretch) one lane adds the count.
static __device__ __forceinline__ void ss_hist_add(LDS uint32_t *hist, bool m, unsigned d)
{
    const unsigned long long b = __ballot(m);
    if (b == 0) return;
    const int first = __ffsll((long long)b) - 1;
    const unsigned d0 = __shfl(d, first);
    if (__ballot(m && d != d0) == 0) {
        if (lane_id() == first) __hip_atomic_fetch_add(&hist[d0], (uint32_t)__popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (m) {
        __hip_atomic_fetch_add(&hist[d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// the bin of `hist` that holds rank kk, the count below that bin and the histogram's total (every lane gets them; with
// kk >= total the bin and the count mean nothing)
static __device__ __forceinline__ void ss_pick(const LDS uint32_t *hist, int kk, int &bin_out, int &below_out, int &total_out)
{
    const int ln = lane_id();
    const int c0 = hist[4 * ln], c1 = hist[4 * ln + 1], c2 = hist[4 * ln + 2], c3 = hist[4 * ln + 3];
    const int s = c0 + c1 + c2 + c3;
    const int incl = wave_scan_incl(s), excl = incl - s;
    const unsigned long long mk = __ballot(excl <= kk && kk < incl);
    const int src = mk ? __ffsll((long long)mk) - 1 : 0;
    int bin = 4 * ln, below = excl;
    if (kk >= below + c0) { below += c0; bin++; if (kk >= below + c1) { below += c1; bin++; if (kk >= below + c2) { below += c2; bin++; } } }
    bin_out = __shfl(bin, src);
    below_out = __shfl(below, src);
    total_out = __shfl(incl, 63);
}

// the order statistics k0 <= k1 of the keys f(x[0, n)) in numpy's order (a NaN key sorts behind every number) -- with
// `skipnan` of the keys that are not NaN (np.nanmedian's view); k0 < 0: the two middles of the keys counted, (cnt - 1) / 2 and
// cnt / 2.  cnt: the keys counted; nan: a key was NaN.  With cnt == 0 the values are NaN.  Uniform call of the whole workgroup
// (whole waves); every thread gets the results: each wave picks the bins from the workgroup's histograms by itself.
// x: anything that gives x[i] as a T -- a pointer, or a Row of common.h (adapter_front.h: raw int16 samples calibrated on load).
template <class T> struct SsPair { T v0, v1; int cnt; bool nan; };
template <class T, class F, class X>
static __device__ SsPair<T> ss_select2(const X x, int n, int k0, int k1, bool skipnan, F f, LDS SsLds *s)
{
    typedef typename SsKey<T>::type K;
    constexpr int NB = (int)sizeof(K);
    const int t = threadIdx.x, nt = blockDim.x;
    K pre0 = 0, pre1 = 0, mask = 0;
    int r0 = k0, r1 = k1, cnt = 0;
    bool two = false, bad = false, any_nan = false;
    const int n_up = (n + nt - 1) / nt * nt;
    for (int pass = 0; pass < NB; pass++) {
        const int shift = 8 * (NB - 1 - pass);
        __syncthreads();
        for (int q = t; q < 512; q += nt) (&s->hist[0][0])[q] = 0;
        if (pass == 0 && t == 0) s->nan = 0;
        __syncthreads();
        for (int i = t; i < n_up; i += nt) { // (every thread takes every round: ss_hist_add votes)
            const bool act = i < n;
            const T v = act ? f(x[i]) : (T)0;
            const bool isn = v != v;
            if (pass == 0) bad |= isn;
            const K key = SsKey<T>::of(v);
            const unsigned d = (unsigned)(key >> shift) & 255u;
            const bool in = act && !(skipnan && isn);
            ss_hist_add(s->hist[0], in && (key & mask) == pre0, d);
            if (two) ss_hist_add(s->hist[1], in && (key & mask) == pre1, d);
        }
        if (pass == 0 && __any(bad) && lane_id() == 0) __hip_atomic_fetch_or(&s->nan, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        int b0, below0, b1, below1, total;
        if (pass == 0) {
            any_nan = s->nan != 0;
            ss_pick(s->hist[0], 0, b0, below0, total);
            cnt = total;
            if (k0 < 0) { r0 = (cnt - 1) / 2; r1 = cnt / 2; }
            if (cnt == 0 || r1 >= cnt) return SsPair<T>{(T)__builtin_nan(""), (T)__builtin_nan(""), cnt, any_nan};
        }
        ss_pick(s->hist[0], r0, b0, below0, total);
        ss_pick(s->hist[two ? 1 : 0], r1, b1, below1, total);
        if (b0 != b1) two = true;
        pre0 |= (K)b0 << shift; pre1 |= (K)b1 << shift;
        mask |= (K)255 << shift;
        r0 -= below0; r1 -= below1;
    }
    return SsPair<T>{SsKey<T>::back(pre0), SsKey<T>::back(pre1), cnt, any_nan};
}

// np.median of f(x[0, n)) -- np.nanmedian with `skipnan`: NaN when nothing is counted, or when a key is NaN and counted; the
// mean (a + b) / 2 of the two middles of an even count
template <class T, class F, class X>
static __device__ __forceinline__ T ss_median(const X x, int n, bool skipnan, F f, LDS SsLds *s)
{
    const SsPair<T> p = ss_select2<T, F, X>(x, n, -1, -1, skipnan, f, s);
    if (p.cnt == 0 || (p.nan && !skipnan)) return (T)__builtin_nan("");
    return (p.cnt & 1) ? p.v1 : (p.v0 + p.v1) / (T)2;
}

// median and MAD (the median of |x - median|) of x[0, n), n >= 0
template <class T, class X>
static __device__ __forceinline__ void ss_med_mad(const X x, int n, bool skipnan, LDS SsLds *s, T &med, T &mad)
{
    med = n > 0 ? ss_median<T, SsIdent<T>, X>(x, n, skipnan, SsIdent<T>(), s) : (T)__builtin_nan("");
    // (a NaN median: every deviation is NaN, and so is their median)
    mad = med != med ? med : ss_median<T, SsAbsDev<T>, X>(x, n, skipnan, SsAbsDev<T>{med}, s);
}

// np.add.reduce(x[0, n)) and np.add.reduce((x - mu)^2) in numpy's order
template <class T, class X> static __device__ __forceinline__ T ss_sum(const X x, int n, LDS NpSumLdsT<T> *ws)
{
    return np_sum_wave(n, [&](long k) { return x[k]; }, ws);
}
template <class T, class X> static __device__ __forceinline__ T ss_sum_sqdev(const X x, int n, T mu, LDS NpSumLdsT<T> *ws)
{
    return np_sum_wave(n, [&](long k) { const T d = x[k] - mu; return d * d; }, ws);
}
static __device__ __forceinline__ float ss_sqrt(float v) { return sqrtf(v); }
static __device__ __forceinline__ double ss_sqrt(double v) { return sqrt(v); }

// A segment of the batch: signal[row, start:end] with Python's clipping to the row's length (start, end >= 0).
// (mirrors adp_seg of include/adapted_hip.h)
struct SsSeg { int64_t start, end; int32_t row, pad; };
static_assert(sizeof(SsSeg) == sizeof(adp_seg), "SsSeg mirrors adp_seg");

// the clipped slice of a segment: its first sample (nullptr and 0 for an empty one)
template <class T>
static __device__ __forceinline__ const T *ss_slice(const T *sig, const int32_t *len, int n_reads, int L, const SsSeg &sg, int &n)
{
    n = 0;
    if (sg.row < 0 || sg.row >= n_reads || sg.start < 0 || sg.end <= sg.start) return nullptr;
    const long long S = len[sg.row];
    const long long a = sg.start < S ? sg.start : S, b = sg.end < S ? sg.end : S;
    n = b > a ? (int)(b - a) : 0;
    return sig + (size_t)sg.row * L + a;
}

// ---------------------------------------------------------------- partition statistics (signal_partitions.py:81-96)
// mean, std, median, MAD of each segment as the reference's calc_partition_stats computes them -> stats[seg, 4] (float64
// carrying the value of the working type exactly) and count[seg], the number of samples of the clipped slice.  An empty slice
// gives NaN x 4 (numpy's mean and median of nothing).  One workgroup per segment.
// the four statistics of x[0, n) -> o[0..3], n -> *cnt: the whole workgroup, x through any accessor (ss_select2)
template <class T, class X>
static __device__ __forceinline__ void ss_stats4(const X x, int n, LDS NpSumLdsT<T> *ws, LDS SsLds *sl, double *o, int64_t *cnt)
{
    if (n == 0) {
        if (threadIdx.x == 0) { o[0] = o[1] = o[2] = o[3] = __builtin_nan(""); *cnt = 0; }
        return;
    }
    const T mean = ss_sum<T>(x, n, ws) / (T)n;
    const T sd = ss_sqrt(ss_sum_sqdev<T>(x, n, mean, ws) / (T)n);
    T med, mad;
    ss_med_mad<T>(x, n, false, sl, med, mad);
    if (threadIdx.x == 0) { o[0] = (double)mean; o[1] = (double)sd; o[2] = (double)med; o[3] = (double)mad; *cnt = n; }
}

template <class T>
__global__ void __launch_bounds__(SS_BLOCK) k_seg_stats(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, int L,
                                                  const SsSeg *__restrict__ segs, int n_seg, double *__restrict__ stats,
                                                  int64_t *__restrict__ count)
{
    __shared__ __attribute__((aligned(16))) SsScratch<T> ws_[1];
    LDS NpSumLdsT<T> *ws = (LDS NpSumLdsT<T> *)&ws_[0].sum;
    LDS SsLds *sl = (LDS SsLds *)&ws_[0].sel;
    const int g = blockIdx.x;
    if (g >= n_seg) return;
    int n;
    const T *x = ss_slice(sig, len, n_reads, L, segs[g], n);
    ss_stats4<T>(x, n, ws, sl, stats + (size_t)g * 4, count + g);
}

// ---------------------------------------------------------------- median and MAD of rows (normalize.py:15-22)
// med_mad of row r's x[0, len[r]) -> medmad[r, 2]; with `skipnan` np.nanmedian's.  One workgroup per row.
template <class T>
__global__ void __launch_bounds__(SS_BLOCK) k_row_med_mad(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, long long L,
                                                    int skipnan, double *__restrict__ medmad)
{
    __shared__ __attribute__((aligned(16))) SsLds sl_[1];
    LDS SsLds *sl = (LDS SsLds *)&sl_[0];
    const int r = blockIdx.x;
    if (r >= n_reads) return;
    T med, mad;
    ss_med_mad<T>(sig + (size_t)r * L, (int)len[r], skipnan != 0, sl, med, mad);
    if (threadIdx.x == 0) { medmad[2 * r] = (double)med; medmad[2 * r + 1] = (double)mad; }
}

// ---------------------------------------------------------------- median and MAD of one large population
// The state of one selection over the population, kept on the device between the passes.
struct SsPop {
    unsigned long long pre0, pre1, mask;
    int r0, r1, cnt, two, nan, pad;
};
#define SS_POP_BLOCK 256

// Pass `pass` of the selection over f(x[0, n)): the histograms of the digit of this pass among the keys that share the prefixes
// found so far.  f: x itself, or |x - *center| with `center` given.  A grid of workgroups, each with histograms in LDS that it
// adds to ghist[2][256] at the end; pass 0 also notes a NaN key.
template <class T>
__global__ void __launch_bounds__(SS_POP_BLOCK) k_pop_hist(const T *__restrict__ x, long long n, const double *__restrict__ center, int pass,
                                                          int skipnan, SsPop *__restrict__ st, uint32_t *__restrict__ ghist)
{
    typedef typename SsKey<T>::type K;
    constexpr int NB = (int)sizeof(K);
    __shared__ __attribute__((aligned(16))) uint32_t hist[2][256];
    const int t = threadIdx.x;
    for (int q = t; q < 512; q += SS_POP_BLOCK) (&hist[0][0])[q] = 0;
    __syncthreads();
    const int shift = 8 * (NB - 1 - pass);
    const K pre0 = (K)st->pre0, pre1 = (K)st->pre1, mask = (K)st->mask;
    const bool two = st->two != 0, abs_dev = center != nullptr;
    const T c = abs_dev ? (T)*center : (T)0;
    bool bad = false;
    const long long stride = (long long)gridDim.x * SS_POP_BLOCK;
    const long long n_up = (n + stride - 1) / stride * stride;
    for (long long i = (long long)blockIdx.x * SS_POP_BLOCK + t; i < n_up; i += stride) { // (whole waves take every round)
        const bool act = i < n;
        T v = act ? x[i] : (T)0;
        if (abs_dev) v = ss_abs(v - c);
        const bool isn = v != v;
        bad |= isn;
        const K key = SsKey<T>::of(v);
        const unsigned d = (unsigned)(key >> shift) & 255u;
        const bool in = act && !(skipnan && isn);
        ss_hist_add((LDS uint32_t *)hist[0], in && (key & mask) == pre0, d);
        if (two) ss_hist_add((LDS uint32_t *)hist[1], in && (key & mask) == pre1, d);
    }
    __syncthreads();
    for (int q = t; q < (two ? 512 : 256); q += SS_POP_BLOCK) {
        const uint32_t h = (&hist[0][0])[q];
        if (h) atomicAdd(&ghist[q], h);
    }
    if (pass == 0 && __any(bad) && lane_id() == 0) atomicOr(&st->nan, 1);
}

// After pass `pass`: the bins of the two ranks (pass 0: the ranks themselves, the middles of the keys counted), the state for
// the next pass, ghist cleared; after the last pass the median into out[0] (and, as T's value, what the MAD's keys are taken
// about).  One wave.
template <class T>
__global__ void __launch_bounds__(64) k_pop_pick(int pass, int skipnan, SsPop *__restrict__ st, uint32_t *__restrict__ ghist,
                                                 double *__restrict__ out)
{
    typedef typename SsKey<T>::type K;
    constexpr int NB = (int)sizeof(K);
    __shared__ __attribute__((aligned(16))) SsLds sl_[1];
    LDS SsLds *s = (LDS SsLds *)&sl_[0];
    const int ln = lane_id();
    for (int q = ln; q < 512; q += 64) { (&s->hist[0][0])[q] = ghist[q]; ghist[q] = 0; }
    ws_sync();
    SsPop p = *st;
    if (pass > 0 && p.cnt == 0) return; // (nothing was counted: NaN was written after pass 0)
    const int shift = 8 * (NB - 1 - pass);
    int b0, below0, b1, below1, total;
    if (pass == 0) {
        ss_pick(s->hist[0], 0, b0, below0, total);
        p.cnt = total; p.r0 = (total - 1) / 2; p.r1 = total / 2;
        if (total == 0 || (p.nan && !skipnan)) {
            p.cnt = 0;
            if (ln == 0) { *st = p; *out = __builtin_nan(""); }
            return;
        }
    }
    ss_pick(s->hist[0], p.r0, b0, below0, total);
    ss_pick(s->hist[p.two ? 1 : 0], p.r1, b1, below1, total);
    if (b0 != b1) p.two = 1;
    p.pre0 |= (unsigned long long)b0 << shift; p.pre1 |= (unsigned long long)b1 << shift;
    p.mask |= 255ull << shift;
    p.r0 -= below0; p.r1 -= below1;
    if (ln != 0) return;
    *st = p;
    if (pass == NB - 1) {
        const T a = SsKey<T>::back((K)p.pre0), b = SsKey<T>::back((K)p.pre1);
        *out = (double)((p.cnt & 1) ? b : (a + b) / (T)2);
    }
}

// ---------------------------------------------------------------- clip and scale (normalize.py:25-63)
// out = (clip(x, med - mad * thresh, med + mad * thresh) - med) / mad, or with `clip_only` the clip alone; the bounds are
// computed in float64 and rounded once to T, as numpy does with Python floats; a NaN sample stays NaN.  medmad: [n_rows, 2], or
// [1, 2] for all rows with `whole`.  status[r] = 1 and nothing written where the MAD is 0 (clip_only: never).  Cells behind
// len[r] are not written.  `nbx` workgroups per row.
template <class T>
__global__ void __launch_bounds__(256) k_clip_scale(const T *__restrict__ x, const int32_t *__restrict__ len, long long L,
                                                    const double *__restrict__ medmad, double thresh, int whole, int clip_only,
                                                    int nbx, T *__restrict__ out, int32_t *__restrict__ status)
{
    const int r = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const double med = medmad[whole ? 0 : 2 * r], mad = medmad[whole ? 1 : 2 * r + 1];
    const bool fail = !clip_only && mad == 0.0;
    if (bx == 0 && threadIdx.x == 0 && (!whole || r == 0)) status[whole ? 0 : r] = fail ? 1 : 0;
    if (fail) return;
    const double w = mad * thresh;
    const T lo = (T)(med - w), hi = (T)(med + w), m = (T)med, sc = (T)mad;
    const long long n = len ? (long long)len[r] : L;
    const T *xr = x + (size_t)r * L;
    T *o = out + (size_t)r * L;
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n; i += (long long)nbx * 256) {
        T v = xr[i];
        v = v < lo ? lo : v; // (np.clip: minimum(maximum(x, lo), hi); a NaN passes both comparisons)
        v = v > hi ? hi : v;
        o[i] = clip_only ? v : (v - m) / sc;
    }
}

// ---------------------------------------------------------------- average pooling (downscale.py:4-38)
// out[r, j] = add.reduce(x[r, j * pool : (j + 1) * pool] with zeros behind the row's end) / T(pool), the sum in numpy's order.
// pool <= 128: one leaf of numpy's tree, a lane per output; `nbx` workgroups per row.
template <class T>
__global__ void __launch_bounds__(256) k_pool_mean(const T *__restrict__ x, int n_rows, long long n_cols, int pool, long long n_out,
                                                   int nbx, T *__restrict__ out)
{
    const int r = blockIdx.x / nbx;
    const long long j = (long long)(blockIdx.x % nbx) * 256 + threadIdx.x;
    if (j >= n_out) return;
    const T *xr = x + (size_t)r * n_cols;
    const long long o = j * pool, left = n_cols - o;
    const T sum = np_pw_leaf<T>(0, pool, [&](int k) { return k < left ? xr[o + k] : (T)0; });
    out[(size_t)r * n_out + j] = sum / (T)pool;
}
// pool > 128: a wave per output
template <class T>
__global__ void __launch_bounds__(64) k_pool_mean_wave(const T *__restrict__ x, int n_rows, long long n_cols, int pool, long long n_out,
                                                       T *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) NpSumLdsT<T> ws_[1];
    const long long j = blockIdx.x % n_out;
    const int r = (int)(blockIdx.x / n_out);
    const T *xr = x + (size_t)r * n_cols;
    const long long o = j * pool, left = n_cols - o;
    const T sum = np_sum_wave(pool, [&](long k) { return k < left ? xr[o + k] : (T)0; }, (LDS NpSumLdsT<T> *)&ws_[0]);
    if (lane_id() == 0) out[(size_t)r * n_out + j] = sum / (T)pool;
}

// ---------------------------------------------------------------- the real-range check (real_range.py:34-67)
// in_range (utils.py) of a scalar: float64 comparisons, NaN never passes
static __device__ __forceinline__ bool ss_in_range(double v, const double *r) { return r[0] <= v && v <= r[1]; }

// np.percentile(x, q100) from the two order statistics around its virtual index: the difference in T, the interpolation in
// float64 (numpy's _lerp)
template <class T>
static __device__ __forceinline__ double ss_percentile(const T *x, int n, double q100, LDS SsLds *s, bool &nan)
{
    int lo, hi;
    double g;
    ws_pct_ranks(n, q100, lo, hi, g);
    const SsPair<T> p = ss_select2<T, SsIdent<T>, const T *>(x, n, lo, hi, false, SsIdent<T>(), s);
    nan = p.nan;
    const T a = p.v0, b = p.v1, diff = b - a;
    double r = (double)a + (double)diff * g;
    if (g >= 0.5) r = (double)b - (double)diff * (1.0 - g);
    return r;
}

// info[seg, 2]: the result; the stage reached -- 0 fewer than 2 * mean_window samples (no values), 1 a mean out of range (the two
// means), 2 the local range taken (all three values).  vals[seg, 3]: mean of the first and of the last mean_window samples (T's
// values), np.percentile(tail, 85) - np.percentile(tail, 15) of the last min(max_obs_local_range, n) samples (float64).
template <class T>
__global__ void __launch_bounds__(SS_BLOCK) k_real_range(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, int L,
                                                   const SsSeg *__restrict__ segs, int n_seg, adp_real_range_args a,
                                                   int32_t *__restrict__ info, double *__restrict__ vals)
{
    __shared__ __attribute__((aligned(16))) SsScratch<T> ws_[1];
    LDS NpSumLdsT<T> *ws = (LDS NpSumLdsT<T> *)&ws_[0].sum;
    LDS SsLds *sl = (LDS SsLds *)&ws_[0].sel;
    const int g = blockIdx.x;
    if (g >= n_seg) return;
    int n;
    const T *x = ss_slice(sig, len, n_reads, L, segs[g], n);
    const int w = a.mean_window;
    int32_t *oi = info + (size_t)g * 2;
    double *ov = vals + (size_t)g * 3;
    if ((long long)n < 2ll * w) {
        if (threadIdx.x == 0) { oi[0] = 0; oi[1] = 0; ov[0] = ov[1] = ov[2] = 0.0; }
        return;
    }
    const T m0 = ss_sum<T>(x, w, ws) / (T)w, m1 = ss_sum<T>(x + (n - w), w, ws) / (T)w;
    int ok = 0, stage = 1;
    double lr = 0.0;
    if (ss_in_range((double)m0, a.mean_start_range) && ss_in_range((double)m1, a.mean_end_range)) {
        const int nt = a.max_obs_local_range < n ? a.max_obs_local_range : n;
        const T *tail = x + (n - nt);
        bool nan85, nan15;
        const double p85 = ss_percentile(tail, nt, 85.0, sl, nan85), p15 = ss_percentile(tail, nt, 15.0, sl, nan15);
        lr = (nan85 || nan15) ? __builtin_nan("") : p85 - p15; // (np.percentile of a slice with a NaN is NaN)
        stage = 2;
        ok = ss_in_range(lr, a.local_range);
    }
    if (threadIdx.x == 0) { oi[0] = ok; oi[1] = stage; ov[0] = (double)m0; ov[1] = (double)m1; ov[2] = lr; }
}

// ---------------------------------------------------------------- open pores (anomalies.py:15-35)
// in_range of an array (utils.py): float32 samples against the bounds rounded to float32 (numpy compares a float32 array with
// a Python float in float32), float64 as is; NaN never passes
static __device__ __forceinline__ bool ss_in_arr(float v, double lo, double hi) { return (float)lo <= v && v <= (float)hi; }
static __device__ __forceinline__ bool ss_in_arr(double v, double lo, double hi) { return lo <= v && v <= hi; }

// The positions (from the slice's start) in range whose distance to the PRECEDING position in range is >= min_obs_diff -> the
// first `cap` of them into pos[seg, cap] (the rest of the row: -1) and count[seg, 3]: how many there are (also past cap), how
// many positions are in range, the last of those (-1: none).  One wave per segment: 64 samples per round, the predecessor of a
// lane's position from the ballot of the round, or the last position of the rounds before.
template <class T>
__global__ void __launch_bounds__(64) k_open_pores(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, int L,
                                                   const SsSeg *__restrict__ segs, int n_seg, double lo, double hi, double min_obs_diff,
                                                   int cap, int64_t *__restrict__ pos, int64_t *__restrict__ count)
{
    const int g = blockIdx.x, ln = lane_id();
    if (g >= n_seg) return;
    int n;
    const T *x = ss_slice(sig, len, n_reads, L, segs[g], n);
    int64_t *op = pos + (size_t)g * cap;
    long long kept = 0, inr = 0, last = -1;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + ln;
        const bool in = i < n && ss_in_arr(x[i], lo, hi);
        const unsigned long long b = __ballot(in);
        if (b == 0) continue;
        const unsigned long long below = b & ((1ull << ln) - 1ull);
        const long long prev = below ? (long long)(i0 + 63 - __clzll((long long)below)) : last;
        const bool keep = in && prev >= 0 && (double)(i - prev) >= min_obs_diff;
        const unsigned long long kb = __ballot(keep);
        if (keep) {
            const long long slot = kept + __popcll(kb & ((1ull << ln) - 1ull));
            if (slot < cap) op[slot] = i;
        }
        kept += __popcll(kb);
        inr += __popcll(b);
        last = i0 + 63 - __clzll((long long)b);
    }
    for (long long k = kept + ln; k < cap; k += 64) op[k] = -1;
    if (ln == 0) { count[(size_t)g * 3] = kept; count[(size_t)g * 3 + 1] = inr; count[(size_t)g * 3 + 2] = last; }
}
