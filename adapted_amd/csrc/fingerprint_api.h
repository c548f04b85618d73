// fingerprint_api.h -- adapter event fingerprints and their comparison by dynamic time warping (an extension, as events_api.h is:
// the reference's README sends its users to a sister tool that tells barcoded adapters apart by the levels of the adapter's
// events).  Compiled in modules.hip only.  Everything is float64 in a fixed order of operations, so that a numpy restatement is
// the exact oracle (tests/fingerprint_oracle.py).  Three kernels:
//
//   k_ev_levels   behind k_ev_scores and k_ev_bounds in a batch of slots, one wave per slot: the slot's boundaries (wl[0, nk), in
//                 index order) and its scores are still there.  With more than E - 1 boundaries the E - 1 greatest in the order
//                 (score, index) stay: an MSB-first radix selection of the (E - 1)-th greatest score on the scores' bit patterns
//                 (scores are >= 0: the pattern orders them), the histogram in LDS as ev_select's; then the strictly greater and,
//                 of the equal ones, the latest.  The level of an event is np.mean of its widened samples: np_sum.h's order, a lane
//                 per event of at most 128 samples (one leaf of numpy's tree), the whole wave on a longer one.  np.median of the
//                 levels and of their absolute deviations by counting ranks in LDS (at most 512 values: exact, no sort).
//   k_dtw         one wave per (query, template) pair: dtw_wave.h's wavefront and nothing else, with C = ceil(Et / 64) template
//                 columns per lane.  The query is staged once in LDS.
//   k_dtw_best    the least and the second least distance of every query, a thread per query.
#pragma once
#include "common.h"
#include "dtw_wave.h"
#include "events_api.h"
#include "np_sum.h"

#define FP_EMAX 512         // the most events of a fingerprint, and the longest query / template of the DTW
#define DTW_SCRATCH_MIB 512 // the default byte budget of a call's distance matrix: batches of queries (modules.hip)
#define DTW_NT_MAX 4096

// the key of rank `rank` (0-based, ascending) among the 64-bit keys key(0), ..., key(m - 1): ev_select with eight passes.
// Uniform call of a one-wave workgroup; every lane gets the key.
template <class F>
static __device__ uint64_t fp_select64(int m, int rank, F key, LDS uint32_t *hist)
{
    const int ln = lane_id();
    uint64_t pre = 0, mask = 0;
    int r = rank;
    for (int pass = 7; pass >= 0; pass--) {
        const int shift = 8 * pass;
        __syncthreads();
        for (int q = ln; q < 256; q += 64) hist[q] = 0;
        __syncthreads();
        for (int base = 0; base < m; base += 64) {
            const int k = base + ln;
            const bool act = k < m;
            const uint64_t v = act ? key(k) : 0ull;
            ss_hist_add(hist, act && (v & mask) == pre, (unsigned)(v >> shift) & 255u);
        }
        __syncthreads();
        int bin, below, total;
        ss_pick(hist, r, bin, below, total);
        pre |= (uint64_t)bin << shift;
        mask |= 255ull << shift;
        r -= below;
    }
    return pre;
}

// np.median of v[0, c), 1 <= c <= FP_EMAX, in LDS: NaN when a value is NaN, else the value of rank c / 2, or the mean of the two
// middle ones.  The rank of v[i]: the values below it plus the equal ones before it.  Uniform call of a one-wave workgroup.
static __device__ double fp_median(const LDS double *v, int c, LDS double *mid)
{
    const int ln = lane_id();
    const int r0 = (c - 1) / 2, r1 = c / 2;
    bool bad = false;
    __syncthreads();
    for (int base = 0; base < c; base += 64) {
        const int i = base + ln;
        if (i < c) {
            const double x = v[i];
            if (x != x) bad = true;
            else {
                int rank = 0;
                for (int j = 0; j < c; j++) {
                    const double y = v[j];
                    rank += (y < x || (y == x && j < i)) ? 1 : 0;
                }
                if (rank == r0) mid[0] = x;
                if (rank == r1) mid[1] = x;
            }
        }
    }
    const bool any_bad = __any(bad);
    __syncthreads();
    if (any_bad) return __builtin_nan("");
    const double a = mid[0], b = mid[1];
    return (c & 1) ? b : (a + b) / 2.0;
}

// grid = slots, block = 64.  info [n_seg, 2]: what k_ev_bounds wrote (the number of boundaries, the status).  count / fpstatus
// [n_seg], lengths / levels / fp [n_seg, E], norm [n_seg, 2].  Src: the samples' source (events_api.h).
template <class Src>
__global__ void __launch_bounds__(64) k_ev_levels(const Src src, const EvSeg *__restrict__ segs, int g0,
                                                const double *__restrict__ score, size_t stride, const uint32_t *__restrict__ wl_all,
                                                int half, const int64_t *__restrict__ info, int E, int32_t *__restrict__ count_out,
                                                int32_t *__restrict__ fpstatus, int32_t *__restrict__ lengths, double *__restrict__ levels,
                                                double *__restrict__ fp, double *__restrict__ norm)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist_[256];
    __shared__ __attribute__((aligned(16))) double lev_[FP_EMAX];
    __shared__ __attribute__((aligned(16))) double dev_[FP_EMAX];
    __shared__ __attribute__((aligned(16))) int32_t edge_[FP_EMAX + 4];
    __shared__ __attribute__((aligned(16))) double mid_[2];
    __shared__ __attribute__((aligned(16))) NpSumLds sum_[1];
    LDS uint32_t *hist = (LDS uint32_t *)hist_;
    LDS double *lev = (LDS double *)lev_, *dev = (LDS double *)dev_, *mid = (LDS double *)mid_;
    LDS int32_t *edge = (LDS int32_t *)edge_;
    LDS NpSumLds *sum = (LDS NpSumLds *)&sum_[0];
    const int s = blockIdx.x, g = g0 + s, ln = lane_id();
    const unsigned long long lower = (1ull << ln) - 1ull;
    const int n = segs[g].n;
    const int nk = (int)info[(size_t)g * 2];
    const int status = (int)info[(size_t)g * 2 + 1];
    const uint32_t *wl = wl_all + (size_t)s * half;
    const double *sc = score + (size_t)s * stride;
    int32_t *ol = lengths + (size_t)g * E;
    double *ov = levels + (size_t)g * E, *of = fp + (size_t)g * E;
    const double nan = __builtin_nan("");
    int count = 0, fst = status;
    double med = nan, mad = nan;
    bool ok = false;
    if (status == 0) {
        // the edges of the events: 0, the boundaries that stay, n
        int kept = 0;
        if (nk > E - 1) {
            const int K = E - 1;
            auto key = [&](int k) { return (uint64_t)__double_as_longlong(sc[wl[k]]); };
            const uint64_t thr = fp_select64(nk, nk - K, key, hist);
            int ngt = 0, neq = 0;
            for (int base = 0; base < nk; base += 64) {
                const int k = base + ln;
                const bool act = k < nk;
                const uint64_t v = act ? key(k) : 0ull;
                ngt += __popcll(__ballot(act && v > thr));
                neq += __popcll(__ballot(act && v == thr));
            }
            const int skip = neq - (K - ngt); // of the equal ones the earliest `skip` go
            int seen = 0;
            for (int base = 0; base < nk; base += 64) {
                const int k = base + ln;
                const bool act = k < nk;
                const uint64_t v = act ? key(k) : 0ull;
                const bool eq = act && v == thr;
                const unsigned long long me = __ballot(eq);
                const bool keep = act && (v > thr || (eq && seen + __popcll(me & lower) >= skip));
                const unsigned long long mk = __ballot(keep);
                if (keep) edge[1 + kept + __popcll(mk & lower)] = (int32_t)wl[k];
                seen += __popcll(me);
                kept += __popcll(mk);
            }
        } else {
            for (int k = ln; k < nk; k += 64) edge[1 + k] = (int32_t)wl[k];
            kept = nk;
        }
        if (ln == 0) { edge[0] = 0; edge[kept + 1] = n; }
        count = kept + 1;
        __syncthreads();
        // the levels: a lane per event of one leaf, then the wave on every longer one
        const auto x = src.seg(g, segs[g].off);
        for (int base = 0; base < count; base += 64) {
            const int e = base + ln;
            if (e < count) {
                const int a = edge[e], len = edge[e + 1] - a;
                if (len <= 128) lev[e] = (0.0 + np_pw_leaf<double>(a, len, [&](int k) { return x[k]; })) / (double)len;
            }
        }
        __syncthreads();
        for (int e = 0; e < count; e++) {
            const int a = edge[e], len = edge[e + 1] - a;
            if (len > 128) {
                const double t = np_sum_wave(len, [&](long k) { return x[a + k]; }, sum);
                if (ln == 0) lev[e] = t / (double)len;
            }
        }
        med = fp_median(lev, count, mid);
        for (int e = ln; e < count; e += 64) dev[e] = __builtin_fabs(lev[e] - med);
        mad = fp_median(dev, count, mid);
        ok = mad != 0.0 && __builtin_isfinite(med) && __builtin_isfinite(mad);
        fst = ok ? 0 : 4;
    }
    for (int e = ln; e < E; e += 64) {
        const bool in = e < count;
        ol[e] = in ? edge[e + 1] - edge[e] : 0;
        ov[e] = in ? lev[e] : nan;
        of[e] = (in && ok) ? (lev[e] - med) / mad : nan;
    }
    if (ln == 0) {
        count_out[g] = count;
        fpstatus[g] = fst;
        norm[(size_t)g * 2] = med;
        norm[(size_t)g * 2 + 1] = mad;
    }
}

// grid = pairs of the batch (query p0 + pair / nt, template pair % nt), block = 64.  q [.., Eq], qc [..]; t [nt, Et], tc [nt] (checked
// by the caller: 1 <= tc <= Et, finite values); dist [queries of the batch, nt].  C * 64 >= Et.
template <int C>
__global__ void __launch_bounds__(64) k_dtw(const double *__restrict__ q, const int32_t *__restrict__ qc, int p0, int Eq,
                                          const double *__restrict__ t, const int32_t *__restrict__ tc, int nt, int Et, int band,
                                          double *__restrict__ dist)
{
    __shared__ __attribute__((aligned(16))) double qa_[FP_EMAX];
    LDS double *qa = (LDS double *)qa_;
    const int ln = lane_id();
    const int pl = (int)(blockIdx.x / (unsigned)nt), k = (int)(blockIdx.x % (unsigned)nt), p = p0 + pl;
    const int n = qc[p], m = tc[k];
    double *o = dist + (size_t)pl * nt + k;
    const double inf = __builtin_inf();
    const bool bad = __any(dtw_stage(q + (size_t)p * Eq, n, Eq, qa, ln, 64));
    __syncthreads();
    if (bad) {
        if (ln == 0) *o = __builtin_nan("");
        return;
    }
    const int R = dtw_radius(band, n, m);
    double c[C], P[C]; // this lane's template values and D[row before][its columns]
#pragma unroll
    for (int jj = 0; jj < C; jj++) {
        const int j0 = ln * C + jj;
        c[jj] = j0 < m ? t[(size_t)k * Et + j0] : 0.0;
        P[jj] = inf;
    }
    double plold = inf; // D[two rows before the next][its last column]
    const int steps = n + (m - 1) / C;
    for (int s = 1; s <= steps; s++) dtw_step<C>(s, ln, n, R, qa, c, P, plold);
    const double res = dtw_corner<C>(P, m);
    if (ln == dtw_corner_lane<C>(m)) *o = res;
}

// block = 64, a thread per query of the batch.  best [.., 2]: the template of the least distance (the lowest index on ties) and of
// the second least, -1 where there is none; bestd [.., 2]: their distances, NaN where -1.  A NaN row: a query that was refused.
__global__ void __launch_bounds__(64) k_dtw_best(const double *__restrict__ dist, int nqb, int nt, int32_t *__restrict__ best,
                                               double *__restrict__ bestd)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= nqb) return;
    const double *row = dist + (size_t)p * nt;
    const double nan = __builtin_nan("");
    int i1 = -1, i2 = -1;
    double d1 = nan, d2 = nan;
    if (row[0] == row[0]) {
        for (int k = 0; k < nt; k++) {
            const double d = row[k];
            if (i1 < 0 || d < d1) { i2 = i1; d2 = d1; i1 = k; d1 = d; }
            else if (i2 < 0 || d < d2) { i2 = k; d2 = d; }
        }
    }
    best[(size_t)p * 2] = i1;
    best[(size_t)p * 2 + 1] = i2;
    bestd[(size_t)p * 2] = d1;
    bestd[(size_t)p * 2 + 1] = i2 < 0 ? nan : d2;
}
