// startmods_api.h -- the reference's start-peak and adapter-start modules as batched kernels, one wave per read.
//
//   k_startpeak_mod   detect_rna_start_peak             start_peak.py:19-84    (every parameter an argument)
//   k_adapter_start   moving_mean_adapter_start_detect  adapter_start.py:20-54
//
// Each kernel is instantiated for float and double (float64 and widened integer input), as mvs_api.h's are: the pooled means,
// bottleneck's move_mean and numpy's cumsum run in the input dtype.  k_start_peak of validate.h (the detect path's float32
// operator with the engine's configuration) is not touched and not called: this header belongs to modules.hip.
#pragma once
#include "common.h"
#include "np_sum.h"
#include "mvs_api.h"

// ---------------------------------------------------------------- detect_rna_start_peak (start_peak.py:19-84)
// lane l's pooled value j0 + l of efficient_average_pooling(row[0, m), ds) (0 at or behind jend): add.reduce of the ds samples in
// numpy's order -- one leaf of its pairwise tree per lane for ds <= 128, the whole tree by the wave, value after value, for a
// longer block -- over zeros behind the row's end (np.pad), divided by T(ds).  Uniform call.
template <class T>
static __device__ T spm_pooled64(const T *row, int m, int ds, long long j0, long long jend, LDS NpSumLdsT<T> *s)
{
    const int ln = lane_id();
    if (ds <= 128) {
        const long long j = j0 + ln;
        if (j >= jend) return (T)0;
        const long long o = j * ds, left = (long long)m - o;
        return np_pw_leaf<T>(0, ds, [&](int k) { return k < left ? row[o + k] : (T)0; }) / (T)ds;
    }
    T mine = (T)0;
    for (int u = 0; u < 64 && j0 + u < jend; u++) {
        const long long o = (j0 + u) * ds, left = (long long)m - o;
        const T v = np_sum_wave(ds, [&](long k) { return k < left ? row[o + k] : (T)0; }, s) / (T)ds;
        if (u == ln) mine = v;
    }
    return mine;
}

// info int32 [n, 5]: 0 valid (0: the reference's try block raised -- an all-None row), 1 start_peak_idx, 2 next_greater_idx,
// 3 open_pore_idx (-1: None), 4 flagged type (0 None, 1 "open pore in adapter", 2 "potential concatemer adapter-only read");
// POOLED indices.  vals float64 [n, 2]: start_peak_pa, next_greater_pa (T's values).
template <class T>
__global__ void __launch_bounds__(64) k_startpeak_mod(const T *__restrict__ sig, const int32_t *__restrict__ full_len, int n_reads, int m,
                                                      adp_start_peak_args p, int32_t *__restrict__ info_out, double *__restrict__ vals_out)
{
    __shared__ __attribute__((aligned(16))) NpSumLdsT<T> sum_[1];
    LDS NpSumLdsT<T> *s = (LDS NpSumLdsT<T> *)&sum_[0];
    const int ln = lane_id();
    const int ds = p.downscale_factor;
    const long long Lp = ((long long)m + ds - 1) / ds; // the pooled width
    const T thr = (T)p.open_pore_pa;                   // (numpy compares an array with a Python float in the array's type)
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const T *row = sig + (size_t)r * m;
        const long long fl = full_len[r];
        const int end_idx = (int)((fl < m ? fl : m) / ds);
        // the open pore: the first of the first end_idx RAW samples above the level, as a pooled index; 0 counts as none
        int op = 0x7fffffff;
        for (int base = 0; base < end_idx && op == 0x7fffffff; base += 64) {
            const int i = base + ln;
            const unsigned long long mk = __ballot(i < end_idx && row[i] > thr);
            if (mk) op = base + __ffsll((long long)mk) - 1;
        }
        op = op == 0x7fffffff ? 0 : op / ds;
        // max_ and its first index in pooled[offset1 : start_peak_max_idx]; a NaN there is the maximum and equals nothing (index 0)
        const long long a = p.offset1 < Lp ? p.offset1 : Lp, b = p.start_peak_max_idx < Lp ? p.start_peak_max_idx : Lp;
        bool valid = b - a > 0; // (an empty slice: .max() raises)
        T mx = (T)0;
        long long max_idx = 0;
        if (valid) {
            T lm = (T)0;
            long long li = -1;
            bool anynan = false;
            for (long long j0 = a; j0 < b; j0 += 64) {
                const T v = spm_pooled64<T>(row, m, ds, j0, b, s);
                if (j0 + ln < b) {
                    if (v != v) anynan = true;
                    else if (li < 0 || v > lm) { lm = v; li = j0 + ln; }
                }
            }
            anynan = __any(anynan);
            if (anynan) { mx = mv_nan<T>(); max_idx = p.offset1; }
            else {
                // (every lane with an entry holds its own maximum and first index; the others stand back)
                T wm = lm;
                bool have = li >= 0;
                for (int o = 32; o > 0; o >>= 1) {
                    const T ov = __shfl_xor(wm, o);
                    const bool oh = __shfl_xor((int)have, o) != 0;
                    if (oh && (!have || ov > wm)) { wm = ov; have = true; }
                }
                mx = wm;
                const long long first = wave_min((li >= 0 && lm == wm) ? li : (long long)0x7fffffffffffffffLL);
                max_idx = first; // (first - a + offset1 with a == offset1: the slice is not empty)
            }
        }
        // the first pooled value above max_ in pooled[start_peak_max_idx + offset2 : end_idx] (none: the slice's start)
        const long long s0 = (long long)p.start_peak_max_idx + p.offset2;
        const long long e0 = end_idx < Lp ? end_idx : Lp, a2 = s0 < Lp ? s0 : Lp;
        if (valid && e0 - a2 <= 0) valid = false; // (argmax of an empty slice raises)
        long long nxt = 0;
        if (valid) {
            long long hit = -1;
            for (long long base = a2; base < e0 && hit < 0; base += 64) {
                const T v = spm_pooled64<T>(row, m, ds, base, e0, s);
                const unsigned long long mk = __ballot(base + ln < e0 && v > mx);
                if (mk) hit = base + __ffsll((long long)mk) - 1;
            }
            nxt = (hit < 0 ? 0 : hit - a2) + s0;
            if (nxt >= Lp) valid = false; // (IndexError)
        }
        int32_t info[5] = {0, 0, 0, -1, 0};
        double v0 = 0.0, v1 = 0.0;
        if (valid) {
            const T nv = __shfl(spm_pooled64<T>(row, m, ds, nxt, nxt + 1, s), 0);
            info[0] = 1; info[1] = (int32_t)max_idx; info[2] = (int32_t)nxt;
            v0 = (double)mx; v1 = (double)nv;
            if (op > 0) {
                if (fabs((double)nxt - (double)op) <= 2.0 + 0.01 * fabs((double)op)) info[4] = 1; // np.isclose(next, open_pore, atol=2, rtol=0.01)
                else if (max_idx < op && op < nxt) info[4] = 2;
                if (info[4]) info[3] = op;
            }
        }
        if (ln < 5) info_out[(size_t)r * 5 + ln] = info[ln];
        if (ln < 2) vals_out[(size_t)r * 2 + ln] = ln ? v1 : v0;
    }
}

// ---------------------------------------------------------------- moving_mean_adapter_start_detect (adapter_start.py:20-54)
// With N = len - min_obs_adapter, w = window and L = N - w, the reference's arrays are, for i in [0, L):
//   moving_mean_fwd[i] = move_mean(x[N-1::-1], w)[N - 1 - i]      (the mean of x[i, i + w), by the chain that runs DOWN the read)
//   bsum[i] = cumsum(moving_mean_rev)[L - 1 - i]                  (the running sum of those means, in the chain's order)
//   fsum[i] = cumsum(moving_mean_fwd)[i]
//   difference[i] = bsum[i] / (L - i) - fsum[i] / (i + 1)         (float64: T array / int64 array)
// Pass 1 walks x from N - 1 down to 0: lane 0 runs bottleneck's chain and the running sum of its means side by side over
// chunks the wave stages in LDS (ASC_HIST samples behind the chunk's end serve x[p + w]; a longer window reads it from global
// memory), and the wave stores both series to its slot of the workspace.  Pass 2 walks up: lane 0 runs fsum over a staged
// chunk, then every lane forms the differences of its positions.  max(difference) -- NaN when any is -- and the first minimum
// over i >= w decide what `difference[:w] = max; cand = argmin(difference)` gives, without the array:
//   a NaN anywhere: difference[0] is NaN and argmin takes the first NaN -> cand 0;   L <= w or min == max: cand 0 (the first);
//   otherwise the first minimum over i >= w.
#define ASC_CHUNK 512
#define ASC_HIST 256

#define AS_ST_OK 0
#define AS_ST_VALUE 2 // bottleneck's ValueError "Moving window (=w) must between 1 and n, inclusive" (info[1] = w, info[2] = n)

template <class T> struct AsLds {
    T in[ASC_CHUNK + ASC_HIST]; // pass 1: in[k] = x[lo + k]
    T mean[ASC_CHUNK];          // pass 1: moving_mean_fwd of the chunk; pass 2: the same, then fsum
    T sum[ASC_CHUNK];           // bsum of the chunk
};

// The detector for ONE read, by one wave (a uniform call): x[i], i in [0, N + min_obs_adapter), through any accessor that gives T
// -- a pointer, or a Row of common.h (adapter_front.h: the slice of a resident row, float32 or raw int16) --, N = len -
// min_obs_adapter.  wmean / wsum: the wave's slot of the workspace, N - w elements each.  What comes back is what k_adapter_start
// writes: info (status, the exception's window and slice size, accepted), res (adapter_start), cand, dc (difference[cand]).
struct AsOut {
    int32_t status, window, size, accepted;
    long long res, cand;
    double dc;
    // info[k] (a chain of selects: an array indexed by the lane would live in scratch memory)
    __device__ __forceinline__ int32_t info(int k) const { return k == 0 ? status : k == 1 ? window : k == 2 ? size : accepted; }
};
template <class T, class X>
static __device__ __forceinline__ AsOut as_detect(const X x, int N, const adp_adapter_start_args &p, T *wmean, T *wsum, LDS AsLds<T> *b)
{
    const int ln = lane_id();
    const int w = p.window, half = p.window / 2, Ls = N - w;
    const T level = (T)p.min_pA_current; // (numpy compares an array with a Python float in the array's type)
    AsOut o = {AS_ST_OK, 0, 0, 0, 0, -1, 0.0};
    long long cand = -1;
    double dc = 0.0;
    if (N < w) { o.status = AS_ST_VALUE; o.window = w; o.size = N > 0 ? N : 0; }
    else if (Ls > 0) {
        // ---- pass 1: p = N - 1 ... 0 is step k = N - 1 - p of move_mean(reversed x); steps k >= w are outputs, at i = p
        BnMean<T> sm = {0, 0, 0};
        T bs = (T)-0.0; // (-0 + y == y for every y: the first sum is the first mean itself, as cumsum's is)
        for (int hi = N; hi > 0;) {
            const int lo = ((hi - 1) / ASC_CHUNK) * ASC_CHUNK;
            const int e = hi + ASC_HIST < N ? hi + ASC_HIST : N;
            ws_sync();
            bool bad = false;
            for (int k = ln; k < e - lo; k += 64) { const T v = x[lo + k]; b->in[k] = v; bad |= v != v; }
            // no NaN in the chunk's windows, all of them full and sliding (hi <= Ls), every old sample staged
            const bool fast = !__any(bad) && hi <= Ls && w <= ASC_HIST;
            ws_sync();
            if (ln == 0) {
                int q = hi - 1;
                if (fast) {
                    for (; q - 7 >= lo; q -= 8) {
                        T an[8], om[8], rm[8], rs[8];
#pragma unroll
                        for (int j = 0; j < 8; j++) { an[j] = b->in[q - j - lo]; om[j] = b->in[q - j + w - lo]; }
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            sm.asum += an[j] - om[j];
                            rm[j] = sm.asum * sm.inv;
                            bs += rm[j];
                            rs[j] = bs;
                        }
#pragma unroll
                        for (int j = 0; j < 8; j++) { b->mean[q - j - lo] = rm[j]; b->sum[q - j - lo] = rs[j]; }
                    }
                }
                for (; q >= lo; q--) {
                    const int k = N - 1 - q;
                    const T aold = k < w ? (T)0 : (q + w < e ? b->in[q + w - lo] : x[q + w]);
                    const T y = bn_mean_step(sm, k, w, b->in[q - lo], aold);
                    if (k >= w) { bs += y; b->mean[q - lo] = y; b->sum[q - lo] = bs; }
                }
            }
            ws_sync();
            const int top = hi < Ls ? hi : Ls;
            for (int k = lo + ln; k < top; k += 64) { wmean[k] = b->mean[k - lo]; wsum[k] = b->sum[k - lo]; }
            hi = lo;
        }
        __threadfence_block();
        ws_sync();
        // ---- pass 2: fsum, the differences, their maximum and the first minimum over i >= w
        T fs = (T)-0.0;
        double lmax = 0.0, lmin = 0.0;
        int imin = -1;
        bool hmax = false, anynan = false;
        for (int c0 = 0; c0 < Ls; c0 += ASC_CHUNK) {
            const int c1 = c0 + ASC_CHUNK < Ls ? c0 + ASC_CHUNK : Ls, nc = c1 - c0;
            ws_sync();
            for (int k = ln; k < nc; k += 64) { b->mean[k] = wmean[c0 + k]; b->sum[k] = wsum[c0 + k]; }
            ws_sync();
            if (ln == 0) {
                int q = 0;
                for (; q + 8 <= nc; q += 8) {
                    T v[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) v[j] = b->mean[q + j];
#pragma unroll
                    for (int j = 0; j < 8; j++) { fs += v[j]; v[j] = fs; }
#pragma unroll
                    for (int j = 0; j < 8; j++) b->mean[q + j] = v[j];
                }
                for (; q < nc; q++) { fs += b->mean[q]; b->mean[q] = fs; }
            }
            ws_sync();
            for (int k = ln; k < nc; k += 64) {
                const int i = c0 + k;
                const double d = (double)b->sum[k] / (double)(Ls - i) - (double)b->mean[k] / (double)(i + 1);
                if (d != d) anynan = true;
                else {
                    if (!hmax || d > lmax) { lmax = d; hmax = true; }
                    if (i >= w && (imin < 0 || d < lmin)) { lmin = d; imin = i; }
                }
            }
        }
        anynan = __any(anynan);
        // the wave's maximum, and its minimum with the first index that holds it (lanes without an entry stand back)
        double M = lmax, m2 = lmin;
        bool hM = hmax, hm = imin >= 0;
        for (int o = 32; o > 0; o >>= 1) {
            const double oM = __shfl_xor(M, o), om = __shfl_xor(m2, o);
            const bool ohM = __shfl_xor((int)hM, o) != 0, ohm = __shfl_xor((int)hm, o) != 0;
            if (ohM && (!hM || oM > M)) { M = oM; hM = true; }
            if (ohm && (!hm || om < m2)) { m2 = om; hm = true; }
        }
        const int i2 = wave_min((imin >= 0 && lmin == m2) ? imin : 0x7fffffff);
        if (anynan) { cand = 0; dc = __builtin_nan(""); }
        else if (hm && m2 < M) { cand = i2; dc = m2; }
        else { cand = 0; dc = M; }
        // ---- the accept: the shift, and a mean above the level within half a window of the candidate
        if (dc < -p.min_shift) {
            const int s0 = cand - half > 0 ? (int)cand - half : 0, s1 = cand + half < Ls ? (int)cand + half : Ls;
            bool above = false;
            for (int k = s0 + ln; k < s1; k += 64) above |= wmean[k] > level;
            if (__any(above)) { o.accepted = 1; o.res = cand + half; }
        }
    }
    o.cand = cand; o.dc = dc;
    return o;
}

// info int32 [n, 4]: status, the exception's window and slice size, accepted.  out int64 [n]: adapter_start.  cand int64 [n]:
// argmin (-1: difference is empty, or the exception).  diff float64 [n]: difference[cand].  ws: [gridDim.x, 2, L] of T.
template <class T>
__global__ void __launch_bounds__(64) k_adapter_start(const T *__restrict__ sig, const int32_t *__restrict__ len, int n_reads, int L,
                                                      adp_adapter_start_args p, T *ws, int32_t *__restrict__ info_out,
                                                      int64_t *__restrict__ out, int64_t *__restrict__ cand_out, double *__restrict__ diff_out)
{
    __shared__ __attribute__((aligned(16))) AsLds<T> b_;
    LDS AsLds<T> *b = (LDS AsLds<T> *)&b_;
    const int ln = lane_id();
    T *wmean = ws + (size_t)blockIdx.x * 2 * L, *wsum = wmean + L;
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const AsOut o = as_detect<T>(sig + (size_t)r * L, len[r] - p.min_obs_adapter, p, wmean, wsum, b);
        if (ln < 4) info_out[(size_t)r * 4 + ln] = o.info(ln);
        if (ln == 0) { out[r] = o.res; cand_out[r] = o.cand; diff_out[r] = o.dc; }
    }
}
