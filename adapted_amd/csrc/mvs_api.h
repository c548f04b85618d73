// mvs_api.h -- the reference's MVS poly(A) module (adapted/detect/mvs.py) as batched kernels, one wave per read.
//
//   k_mvs_check    mean_var_shift_polyA_check          mvs.py:45-158   (every branch: windowed_stats, less_signal_ok)
//   k_mvs_at_loc   mean_var_shift_polyA_detect_at_loc  mvs.py:181-338  (less_signal_ok either way)
//   k_mvs_stream   mean_var_shift_polyA_detect         mvs.py:341-426  (the streaming walk)
//
// Each kernel is instantiated for float (the pipeline's calibrated signals) and double (float64 and widened integer input):
// bottleneck runs its recurrences in the input dtype, numpy's medians and sums too.  The float instantiations use the float32
// selections and sums of wave_stats.h; the double ones the 64-bit radix select below (common.h's d2key) and np_sum.h's
// pairwise float64 sum.  k_validate's mvs_check / mvs_detect_at_loc (validate.h) are not touched.
//
// The bottleneck chains are the NaN-aware recurrences of bottleneck/src/move_template.c (a NaN sample is counted out of the
// window; a window with fewer than `window` valid samples yields NaN): on NaN-free input they perform exactly the operations of
// bn_move_mean / bn_move_var.  Lane 0 runs move_var and move_mean side by side, over chunks the wave stages in LDS with coalesced loads
// (MVC_HIST samples of history in front of each chunk serve the sliding steps; a longer window reads its old sample from
// global memory).  k_mvs_stream keeps only the current chunk of both series, in LDS: the values at position i depend on samples
// <= i alone, so the walk never needs the whole series, and its scratch is bounded per wave, not per read.
//
// Compiled in modules.hip with the other module drop-ins, apart from adapted_hip.hip: calls from here into the shared helpers
// of wave_stats.h would otherwise change how the compiler optimises them across the detect path's kernels (k_validate's code
// changed when this header was part of that unit).  In a unit of its own it calls them freely.
#pragma once
#include <type_traits>
#include "common.h"
#include "np_sum.h"
#include "wave_stats.h"

#define MVC_CHUNK 512
#define MVC_HIST 256

// status of a read (adp_mvs_* info[2]): the reference raises
#define MVS_ST_OK 0
#define MVS_ST_INDEX 1 // IndexError: np.percentile of an empty slice (info[3] = -1, info[4] = 0), or moving_mean[2 * offset] past
                       // the series (info[3] = 2 * offset, info[4] = its size)
#define MVS_ST_VALUE 2 // bottleneck's ValueError "Moving window (=w) must between 1 and n, inclusive" (info[3] = w, info[4] = n)

static __device__ __forceinline__ bool in_range_d(double v, double lo, double hi) { return lo <= v && v <= hi; }

template <class T> struct MvsLds {
    T in[MVC_HIST + MVC_CHUNK]; // buf[k] = x[lo + k]
    T mean[MVC_CHUNK], var[MVC_CHUNK];
};

// ---------------------------------------------------------------- bottleneck's NaN-aware chains, one lane each
template <class T> struct BnMean { T asum, inv; int count; };
template <class T> struct BnVar { T amean, assqdm, inv; int count; };

template <class T> static __device__ __forceinline__ T mv_nan() { return (T)__builtin_nan(""); }

// position i of move_mean(x, w): ai = x[i], aold = x[i - w] (read only for i >= w)
template <class T>
static __device__ __forceinline__ T bn_mean_step(BnMean<T> &s, int i, int w, T ai, T aold)
{
    if (i < w) {
        if (ai == ai) { s.asum += ai; s.count++; }
        if (i < w - 1) return mv_nan<T>();
        const T y = s.count >= w ? s.asum / (T)s.count : mv_nan<T>();
        s.inv = (T)(1.0 / (double)s.count);
        return y;
    }
    if (ai == ai) {
        if (aold == aold) s.asum += ai - aold;
        else { s.asum += ai; s.count++; s.inv = (T)(1.0 / (double)s.count); }
    } else if (aold == aold) { s.asum -= aold; s.count--; s.inv = (T)(1.0 / (double)s.count); }
    return s.count >= w ? s.asum * s.inv : mv_nan<T>();
}

template <class T>
static __device__ __forceinline__ T bn_var_step(BnVar<T> &s, int i, int w, T ai, T aold)
{
    if (i < w) {
        if (ai == ai) {
            s.count++;
            const T delta = ai - s.amean;
            s.amean += delta / (T)s.count;
            s.assqdm += delta * (ai - s.amean);
        }
        if (i < w - 1) return mv_nan<T>();
        T y = mv_nan<T>();
        if (s.count >= w) { if (s.assqdm < 0) s.assqdm = 0; y = s.assqdm / (T)s.count; }
        s.inv = (T)(1.0 / (double)s.count);
        return y;
    }
    if (ai == ai) {
        if (aold == aold) {
            const T delta = ai - aold;
            aold -= s.amean; s.amean += delta * s.inv; ai -= s.amean;
            s.assqdm += (ai + aold) * delta;
        } else {
            s.count++; s.inv = (T)(1.0 / (double)s.count);
            const T delta = ai - s.amean;
            s.amean += delta * s.inv;
            s.assqdm += delta * (ai - s.amean);
        }
    } else if (aold == aold) {
        s.count--; s.inv = (T)(1.0 / (double)s.count);
        if (s.count > 0) { const T delta = aold - s.amean; s.amean -= delta * s.inv; s.assqdm -= delta * (aold - s.amean); }
        else { s.amean = 0; s.assqdm = 0; }
    }
    if (s.count >= w) { if (s.assqdm < 0) s.assqdm = 0; return s.assqdm * s.inv; }
    return mv_nan<T>();
}

// Stage x[lo, hi) into LDS (lo = max(0, c0 - MVC_HIST)) and advance both chains over [c0, hi); position i goes to
// out_mean / out_var [i - o0].  All lanes call it; lane 0 runs both chains, step by step side by side (two independent
// dependency chains for the scheduler).  A chunk whose staged samples hold no NaN, past the first window and with both
// windows inside the staged history, takes the sliding steps eight at a time with the LDS reads first: every window is full
// there (count == window), and the steps are those of the NaN-aware recurrence's both-valid branch, operation for operation.
template <class T, class O>
static __device__ void mv_chunk(const T *x, int c0, int hi, int wm, int wv, LDS MvsLds<T> *b, BnMean<T> &sm, BnVar<T> &sv,
                                O out_mean, O out_var, int o0)
{
    const int ln = lane_id();
    const int lo = c0 >= MVC_HIST ? c0 - MVC_HIST : 0;
    ws_sync();
    bool bad = false;
    for (int k = ln; k < hi - lo; k += 64) { const T v = x[lo + k]; b->in[k] = v; bad |= v != v; }
    const bool fast = !__any(bad) && c0 >= (wm > wv ? wm : wv) && wm <= MVC_HIST && wv <= MVC_HIST;
    ws_sync();
    if (ln == 0) {
        int i = c0;
        if (fast) {
            for (; i + 8 <= hi; i += 8) {
                T an[8], om[8], ov[8], rm[8], rv[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { an[j] = b->in[i + j - lo]; om[j] = b->in[i + j - wm - lo]; ov[j] = b->in[i + j - wv - lo]; }
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    sm.asum += an[j] - om[j];
                    rm[j] = sm.asum * sm.inv;
                    T ai = an[j], aold = ov[j];
                    const T delta = ai - aold;
                    aold -= sv.amean; sv.amean += delta * sv.inv; ai -= sv.amean;
                    sv.assqdm += (ai + aold) * delta;
                    if (sv.assqdm < 0) sv.assqdm = 0;
                    rv[j] = sv.assqdm * sv.inv;
                }
#pragma unroll
                for (int j = 0; j < 8; j++) { out_mean[i + j - o0] = rm[j]; out_var[i + j - o0] = rv[j]; }
            }
        }
        for (; i < hi; i++) {
            const T ai = b->in[i - lo];
            const T aom = i < wm ? (T)0 : (i - wm >= lo ? b->in[i - wm - lo] : x[i - wm]);
            const T aov = i < wv ? (T)0 : (i - wv >= lo ? b->in[i - wv - lo] : x[i - wv]);
            out_var[i - o0] = bn_var_step(sv, i, wv, ai, aov);
            out_mean[i - o0] = bn_mean_step(sm, i, wm, ai, aom);
        }
    }
    __threadfence_block();
    ws_sync();
}

// both whole series of x[0, n) into global scratch (positions < window - 1 hold NaN, as bottleneck returns them)
template <class T>
static __device__ void mv_series(const T *x, int n, int wm, int wv, LDS MvsLds<T> *b, T *smean, T *svar)
{
    BnMean<T> sm = {0, 0, 0};
    BnVar<T> sv = {0, 0, 0, 0};
    for (int c0 = 0; c0 < n; c0 += MVC_CHUNK) mv_chunk<T, T *>(x, c0, min(n, c0 + MVC_CHUNK), wm, wv, b, sm, sv, smean, svar, 0);
}

// ---------------------------------------------------------------- numpy's statistics, per dtype
static __device__ __forceinline__ bool mv_any_nan(const float *x, int n)
{
    bool bad = false;
    for (int i = lane_id(); i < n; i += 64) { const float v = x[i]; bad |= v != v; }
    return __any(bad);
}
static __device__ __forceinline__ bool mv_any_nan(const double *x, int n)
{
    bool bad = false;
    for (int i = lane_id(); i < n; i += 64) { const double v = x[i]; bad |= v != v; }
    return __any(bad);
}

// x_(k) of the (non-NaN, with skipnan) entries of x[0, n): MSB-first radix select, 8 bits of the 64-bit key per pass
static __device__ __noinline__ double mv_select_d(const double *x, int n, int k, bool skipnan, LDS WaveScratch *ws)
{
    const int ln = lane_id();
    uint64_t prefix = 0, mask = 0;
    int kk = k;
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        ws_sync();
        for (int q = ln; q < 256; q += 64) ws->hist[q] = 0;
        ws_sync();
        for (int i = ln; i < n; i += 64) {
            const double v = x[i];
            if (skipnan && v != v) continue;
            const uint64_t key = d2key(v);
            if ((key & mask) == prefix) __hip_atomic_fetch_add(&ws->hist[(key >> shift) & 255u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        ws_sync();
        const int c0 = ws->hist[4 * ln], c1 = ws->hist[4 * ln + 1], c2 = ws->hist[4 * ln + 2], c3 = ws->hist[4 * ln + 3];
        const int s = c0 + c1 + c2 + c3;
        const int incl = wave_scan_incl(s), excl = incl - s;
        const unsigned long long mk = __ballot(excl <= kk && kk < incl);
        const int src = __ffsll((long long)mk) - 1;
        int bin = 4 * ln, below = excl;
        if (kk >= below + c0) { below += c0; bin++; if (kk >= below + c1) { below += c1; bin++; if (kk >= below + c2) { below += c2; bin++; } } }
        bin = __shfl(bin, src);
        below = __shfl(below, src);
        prefix |= (uint64_t)bin << shift;
        mask |= (uint64_t)255 << shift;
        kk -= below;
    }
    return key2d(prefix);
}

// np.median(x[0, n)): NaN for an empty slice or one with a NaN
static __device__ float mv_median(const float *x, int n, LDS WaveScratch *ws)
{
    if (n <= 0 || mv_any_nan(x, n)) return __builtin_nanf("");
    return wave_median(x, n, 0, 0.f, ws);
}
static __device__ double mv_median(const double *x, int n, LDS WaveScratch *ws)
{
    if (n <= 0 || mv_any_nan(x, n)) return __builtin_nan("");
    const double vk = mv_select_d(x, n, n / 2, false, ws);
    if (n & 1) return vk;
    return (mv_select_d(x, n, n / 2 - 1, false, ws) + vk) / 2.0;
}

// np.nanmedian(s[0, n))
static __device__ float mv_nanmedian(const float *s, int n, LDS WaveScratch *ws)
{
    int cnt = 0;
    for (int i = lane_id(); i < n; i += 64) cnt += s[i] == s[i];
    cnt = wave_sum(cnt);
    if (cnt <= 0) return __builtin_nanf("");
    float vk, vkm1;
    wave_select2_skipnan(s, n, cnt / 2, 0, 0.f, ws, vk, vkm1);
    return (cnt & 1) ? vk : (vkm1 + vk) / 2.0f;
}
static __device__ double mv_nanmedian(const double *s, int n, LDS WaveScratch *ws)
{
    int cnt = 0;
    for (int i = lane_id(); i < n; i += 64) cnt += s[i] == s[i];
    cnt = wave_sum(cnt);
    if (cnt <= 0) return __builtin_nan("");
    const double vk = mv_select_d(s, n, cnt / 2, true, ws);
    if (cnt & 1) return vk;
    return (mv_select_d(s, n, cnt / 2 - 1, true, ws) + vk) / 2.0;
}

// np.median(x) and np.subtract(*np.percentile(x, (85, 15))) of a non-empty slice (NaN anywhere: both NaN)
static __device__ void mv_med_lrange(const float *x, int n, LDS WaveScratch *ws, float &med, double &lr)
{
    if (mv_any_nan(x, n)) { med = __builtin_nanf(""); lr = __builtin_nan(""); return; }
    wave_median_local_range(x, n, ws, med, lr);
}
static __device__ __forceinline__ double mv_pct_d(const double *x, int n, double q100, LDS WaveScratch *ws)
{
    int lo, hi; double g;
    ws_pct_ranks(n, q100, lo, hi, g);
    const double b = mv_select_d(x, n, hi, false, ws), a = hi == lo ? b : mv_select_d(x, n, lo, false, ws);
    const double diff = b - a;
    double r = a + diff * g;
    if (g >= 0.5) r = b - diff * (1.0 - g);
    return r;
}
static __device__ void mv_med_lrange(const double *x, int n, LDS WaveScratch *ws, double &med, double &lr)
{
    if (mv_any_nan(x, n)) { med = __builtin_nan(""); lr = __builtin_nan(""); return; }
    med = mv_median(x, n, ws);
    lr = mv_pct_d(x, n, 85.0, ws) - mv_pct_d(x, n, 15.0, ws);
}

// np.mean / np.var (ddof 0) of x[0, n): NaN for an empty slice (numpy's 0 / 0)
// (float32: wave_stats.h's)
static __device__ float mv_np_mean(const float *x, int n, LDS WaveScratch *ws) { return wave_np_mean(x, n, ws); }
static __device__ float mv_np_var(const float *x, int n, LDS WaveScratch *ws) { return wave_np_var(x, n, ws, nullptr); }
// (float64: np_sum.h's sum; its LDS state takes the place of the selections' scratch, idle meanwhile)
static_assert(sizeof(NpSumLds) <= sizeof(WaveScratch) && alignof(NpSumLds) <= 16, "np_sum_wave's state must fit the wave scratch it reuses");
static __device__ double mv_np_mean(const double *x, int n, LDS WaveScratch *ws)
{
    return np_sum_wave(n, [&](long k) { return x[k]; }, (LDS NpSumLds *)ws) / (double)n;
}
static __device__ double mv_np_var(const double *x, int n, LDS WaveScratch *ws)
{
    const double mu = mv_np_mean(x, n, ws);
    return np_sum_wave(n, [&](long k) { const double d = x[k] - mu; return d * d; }, (LDS NpSumLds *)ws) / (double)n;
}

// the array form of in_range (utils.py:26) on a series value: float32 against the bounds cast to float32 (numpy 1.x value-based
// casting), float64 as is; NaN never passes
static __device__ __forceinline__ bool mv_in_arr(float v, double lo, double hi) { return (float)lo <= v && v <= (float)hi; }
static __device__ __forceinline__ bool mv_in_arr(double v, double lo, double hi) { return lo <= v && v <= hi; }

// python's x[lo:hi] of an array of size S, 0 <= lo, hi -> (start, length)
static __device__ __forceinline__ void mv_slice(long long lo, long long hi, long long S, long long &st, int &n)
{
    const long long a = lo < S ? lo : S, b = hi < S ? hi : S;
    st = a;
    n = b > a ? (int)(b - a) : 0;
}

static __device__ __forceinline__ void mv_set_err(int32_t *info, int st, int w, int n)
{
    info[2] = st; info[3] = w; info[4] = n;
}

// ---------------------------------------------------------------- mean_var_shift_polyA_check (mvs.py:45-158)
// out: info int32 [n, 8] (0 ok, 1 check_vector bits (bit j = entry j True), 2 status, 3-4 the exception's numbers, 5 past the early outs),
// vals float64 [n, 5] (mean, var, med, local range, median shift).  scratch: [gridDim.x, 2, L] of T.
template <class T>
__global__ void __launch_bounds__(64) k_mvs_check(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, int L,
                                                  const int64_t *__restrict__ a_end, const int64_t *__restrict__ p_end, adp_mvs_args p,
                                                  T *__restrict__ scratch, int32_t *__restrict__ info_out, double *__restrict__ vals_out)
{
    __shared__ __attribute__((aligned(16))) WaveScratch ws_;
    __shared__ __attribute__((aligned(16))) MvsLds<T> b_;
    LDS WaveScratch *ws = (LDS WaveScratch *)&ws_;
    LDS MvsLds<T> *b = (LDS MvsLds<T> *)&b_;
    T *smean = scratch + (size_t)blockIdx.x * 2 * L, *svar = smean + L;
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        int32_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double v[5] = {0, 0, 0, 0, 0};
        const long long S = len[r], ae = a_end[r], pe = p_end[r];
        const T *x0 = sig + (size_t)r * L;
        const bool early = pe == 0 || ae == 0 || pe < ae || pe - ae <= 2 || (!p.less_signal_ok && S < ae + p.median_shift_window);
        if (!early) {
            info[5] = 1; // (past the early outs: the reference's result is no longer its `failed_results`)
            long long st; int n;
            mv_slice(ae, pe, S, st, n);
            const T *x = x0 + st;
            T mean = 0, var = 0;
            bool err = false;
            if (p.windowed_stats) {
                const bool wvar = !(pe - ae <= p.pA_var_window + 2), wmean = !(pe - ae <= p.pA_mean_window + 2);
                if (wvar && n < p.pA_var_window) { mv_set_err(info, MVS_ST_VALUE, p.pA_var_window, n); err = true; }
                else if (wmean && n < p.pA_mean_window) { mv_set_err(info, MVS_ST_VALUE, p.pA_mean_window, n); err = true; }
                else {
                    if (wvar || wmean) mv_series<T>(x, n, p.pA_mean_window, p.pA_var_window, b, smean, svar);
                    var = wvar ? mv_nanmedian(svar, n, ws) : mv_np_var(x, n, ws);
                    mean = wmean ? mv_nanmedian(smean, n, ws) : mv_np_mean(x, n, ws);
                }
            } else {
                mean = mv_np_mean(x, n, ws);
                var = mv_np_var(x, n, ws);
            }
            if (!err && n == 0) { mv_set_err(info, MVS_ST_INDEX, -1, 0); err = true; } // np.percentile of an empty slice
            if (!err) {
                T med; double lr;
                mv_med_lrange(x, n, ws, med, lr);
                long long s1, s2; int n1, n2;
                mv_slice(ae, ae + p.median_shift_window, S, s1, n1);
                const long long l0 = ae - p.median_shift_window > 0 ? ae - p.median_shift_window : 0;
                mv_slice(l0, ae, S, s2, n2);
                const T shift = mv_median(x0 + s1, n1, ws) - mv_median(x0 + s2, n2, ws);
                v[0] = (double)mean; v[1] = (double)var; v[2] = (double)med; v[3] = lr; v[4] = (double)shift;
                int bits = 0;
                if (in_range_d(v[0], p.pA_mean_range[0], p.pA_mean_range[1])) bits |= 1;
                if (in_range_d(v[1], p.pA_var_range[0], p.pA_var_range[1])) bits |= 2;
                if (in_range_d(v[2], p.polyA_med_range[0], p.polyA_med_range[1])) bits |= 4;
                if (in_range_d(v[3], p.polyA_local_range[0], p.polyA_local_range[1])) bits |= 8;
                if (in_range_d(v[4], p.median_shift_range[0], p.median_shift_range[1])) bits |= 16;
                info[1] = bits;
                info[0] = bits == 31;
            }
        }
        if (lane_id() < 8) info_out[(size_t)r * 8 + lane_id()] = info[lane_id()];
        if (lane_id() < 5) vals_out[(size_t)r * 5 + lane_id()] = v[lane_id()];
    }
}

// ---------------------------------------------------------------- mean_var_shift_polyA_detect_at_loc (mvs.py:181-338)
// out: info as k_mvs_check's (bit 0 of info[1] unused), idx int64 [n], vals float64 [n, 5]
template <class T>
__global__ void __launch_bounds__(64) k_mvs_at_loc(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, int L,
                                                   const int64_t *__restrict__ locs, adp_mvs_args p, T *__restrict__ scratch,
                                                   int32_t *__restrict__ info_out, int64_t *__restrict__ idx_out, double *__restrict__ vals_out)
{
    __shared__ __attribute__((aligned(16))) WaveScratch ws_;
    __shared__ __attribute__((aligned(16))) MvsLds<T> b_;
    LDS WaveScratch *ws = (LDS WaveScratch *)&ws_;
    LDS MvsLds<T> *b = (LDS MvsLds<T> *)&b_;
    T *smean = scratch + (size_t)blockIdx.x * 2 * L, *svar = smean + L;
    const int wm = p.pA_mean_window, wv = p.pA_var_window;
    const int offset = wm > wv ? wm : wv;
    const int tailw = p.median_shift_window > p.polyA_window ? p.median_shift_window : p.polyA_window;
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        int32_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double v[5] = {0, 0, 0, 0, 0};
        long long ridx = 0;
        const long long S = len[r], loc = locs[r];
        const T *x0 = sig + (size_t)r * L;
        const bool early = (!p.less_signal_ok && S < loc + p.search_window + tailw) || loc < offset;
        if (!early) {
            long long st; int n;
            mv_slice(loc - offset, loc + p.search_window, S, st, n);
            bool err = false;
            if (n < wm) { mv_set_err(info, MVS_ST_VALUE, wm, n); err = true; }
            else if (n < wv) { mv_set_err(info, MVS_ST_VALUE, wv, n); err = true; }
            int idx = 0;
            T mean = 0, var = 0;
            if (!err) {
                mv_series<T>(x0 + st, n, wm, wv, b, smean, svar);
                idx = -1;
                for (int base = 0; base < n; base += 64) { // np.argmax of the match mask: its first True
                    const int i = base + lane_id();
                    const bool hit = i < n && mv_in_arr(smean[i], p.pA_mean_range[0], p.pA_mean_range[1]) &&
                                     mv_in_arr(svar[i], p.pA_var_range[0], p.pA_var_range[1]);
                    const unsigned long long mk = __ballot(hit);
                    if (mk) { idx = base + __ffsll((long long)mk) - 1; break; }
                }
                if (idx < 0) idx = 0;
                const int at = idx > 0 ? idx : 2 * offset;
                if (at >= n) { mv_set_err(info, MVS_ST_INDEX, at, n); err = true; }
                else { mean = smean[at]; var = svar[at]; }
            }
            if (!err) {
                ridx = idx > 0 ? (long long)idx + loc - offset : 0;
                const long long loc_ = loc > ridx ? loc : ridx;
                long long s1, s2, s3; int n1, n2, n3;
                mv_slice(loc_, loc_ + p.polyA_window, S, s1, n1);
                if (n1 == 0) { mv_set_err(info, MVS_ST_INDEX, -1, 0); err = true; }
                else {
                    T med; double lr;
                    mv_med_lrange(x0 + s1, n1, ws, med, lr);
                    mv_slice(loc_, loc_ + p.median_shift_window, S, s2, n2);
                    mv_slice(0, loc_, S, s3, n3);
                    const T shift = mv_median(x0 + s2, n2, ws) - mv_median(x0 + s3, n3, ws);
                    v[0] = (double)mean; v[1] = (double)var; v[2] = (double)med; v[3] = lr; v[4] = (double)shift;
                    info[0] = idx > 0 && in_range_d(v[2], p.polyA_med_range[0], p.polyA_med_range[1]) &&
                              in_range_d(v[3], p.polyA_local_range[0], p.polyA_local_range[1]) &&
                              in_range_d(v[4], p.median_shift_range[0], p.median_shift_range[1]);
                }
            }
            if (err) ridx = 0;
        }
        if (lane_id() < 8) info_out[(size_t)r * 8 + lane_id()] = info[lane_id()];
        if (lane_id() < 5) vals_out[(size_t)r * 5 + lane_id()] = v[lane_id()];
        if (lane_id() == 0) idx_out[r] = ridx;
    }
}

// ---------------------------------------------------------------- mean_var_shift_polyA_detect (mvs.py:341-426)
// The series of signal[min_obs_adapter:] advance chunk by chunk; each chunk's match mask is balloted from the position the walk
// has reached (`offset`) on.  A match at series index j is the reference's hit idx = min_obs_adapter + j: too close to the end
// (min_obs_post_loc) ends the walk with 0, otherwise the wave evaluates the poly(A) window's median and local range and the
// median shift, accepts (idx) or continues from j + search_increment_step.  No match up to the end: 0.  out: int64 [n].
template <class T>
__global__ void __launch_bounds__(64) k_mvs_stream(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, int L,
                                                   adp_mvs_args p, int64_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) WaveScratch ws_;
    __shared__ __attribute__((aligned(16))) MvsLds<T> b_;
    LDS WaveScratch *ws = (LDS WaveScratch *)&ws_;
    LDS MvsLds<T> *b = (LDS MvsLds<T> *)&b_;
    const int wm = p.s_pA_mean_window, wv = p.s_pA_var_window, mo = p.min_obs_adapter;
    const int offset0 = wm > wv ? wm : wv;
    int need = offset0;
    if (p.min_obs_post_loc > need) need = p.min_obs_post_loc;
    if (p.s_polyA_window > need) need = p.s_polyA_window;
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const long long S = len[r];
        long long res = 0;
        if (S >= (long long)mo + need) {
            const T *x0 = sig + (size_t)r * L;
            const T *x = x0 + mo;
            const int N = (int)(S - mo);
            BnMean<T> sm = {0, 0, 0};
            BnVar<T> sv = {0, 0, 0, 0};
            long long off = offset0; // the reference's `offset`: matches before it are ignored
            bool done = false;
            for (int c0 = 0; c0 < N && !done; c0 += MVC_CHUNK) {
                const int hi = min(N, c0 + MVC_CHUNK);
                if (off >= N) break;
                mv_chunk<T, LDS T *>(x, c0, hi, wm, wv, b, sm, sv, b->mean, b->var, c0);
                while (!done && off < hi) {
                    int j = -1;
                    for (long long base = off > c0 ? off : c0; base < hi; base += 64) {
                        const long long i = base + lane_id();
                        const bool hit = i < hi && mv_in_arr(b->mean[i - c0], p.s_pA_mean_range[0], p.s_pA_mean_range[1]) &&
                                         mv_in_arr(b->var[i - c0], p.s_pA_var_range[0], p.s_pA_var_range[1]);
                        const unsigned long long mk = __ballot(hit);
                        if (mk) { j = (int)(base + __ffsll((long long)mk) - 1); break; }
                    }
                    if (j < 0) break; // nothing more in this chunk
                    const long long idx = (long long)mo + j;
                    if (S - idx < p.min_obs_post_loc) { done = true; break; }
                    long long s1, s2, s3; int n1, n2, n3;
                    mv_slice(idx, idx + p.s_polyA_window, S, s1, n1);
                    mv_slice(idx, idx + p.s_median_shift_window, S, s2, n2);
                    mv_slice(idx - p.s_median_shift_window > 0 ? idx - p.s_median_shift_window : 0, idx, S, s3, n3);
                    T med; double lr;
                    mv_med_lrange(x0 + s1, n1, ws, med, lr);
                    const T shift = mv_median(x0 + s2, n2, ws) - mv_median(x0 + s3, n3, ws);
                    if (in_range_d((double)med, p.s_polyA_med_range[0], p.s_polyA_med_range[1]) &&
                        in_range_d(lr, p.s_polyA_local_range[0], p.s_polyA_local_range[1]) &&
                        in_range_d((double)shift, p.s_median_shift_range[0], p.s_median_shift_range[1])) {
                        res = idx; done = true; break;
                    }
                    off = (long long)j + p.search_increment_step;
                }
            }
        }
        if (lane_id() == 0) out[r] = res;
    }
}

