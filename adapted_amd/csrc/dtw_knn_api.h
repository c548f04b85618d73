// dtw_knn_api.h -- the k nearest labelled fingerprints of every query under DTW, without the distance matrix (an extension, as
// dtw_cluster_api.h is, whose pair kernel this one continues).  Compiled in modules.hip only.  The distance of a pair is k_dtw's to
// the bit (dtw_wave.h: the one wavefront of both, lane l owns C = ceil(Er / 64) reference columns in registers, the query staged once
// in LDS); what is new is that a pair is ABANDONED as soon as a lower bound of its distance is strictly greater than a distance that
// is known to be >= the query's final k-th least -- which no result can see (include/adapted_hip_knn.h).  No data passes between
// workgroups inside a launch, no float atomics, nothing depends on scheduling.  Two kernels:
//
//   k_dtw_knn      one workgroup of KNN_WAVES waves per (query, segment of references).  The query is staged and checked once.  Wave w
//                  walks the references j0 + w, j0 + w + KNN_WAVES, ... of its segment and keeps the k least (dist, idx) of the pairs
//                  it finished, sorted, in registers: lane t holds entry t.  With k entries its k-th distance goes to the wave's LDS
//                  slot.  A slot is the k-th least of a subset of the candidates, so it is >= the final k-th least; the threshold of a
//                  test is the least of the slots as they are read at that moment -- a slot only ever falls, so a stale read is only
//                  looser (a slot is one aligned double, written and read as one 64-bit LDS access).  At the end wave 0 selects the k least of the waves' lists: the segment's list.
//   k_knn_merge    one wave per query: the k least (dist, idx) of its segments' lists, and the sums of their counters.
#pragma once
#include "fingerprint_api.h"

// (KNN_KMAX, the most neighbours, and KNN_NR_MAX, the most references: include/adapted_hip_knn.h)
#define KNN_WAVES 4         // waves of a workgroup of k_dtw_knn
#define KNN_SEG_MIN 256      // the default segment: at least this many references, ...
#define KNN_TARGET_WGS 8192  // ... and as many segments per query as make this many workgroups (modules.hip)
#define KNN_CHECK_PERIOD 8   // the abandon test runs at the steps s that are multiples of it (a power of two; measured: DESIGN.md)

// is (d1, i1) before (d2, i2)?  Distance first, then the lower index.  +inf is an ordinary distance; NaN does not occur.
static __device__ __forceinline__ bool knn_before(double d1, int i1, double d2, int i2) { return d1 < d2 || (d1 == d2 && i1 < i2); }

// One wave: the k least in the order (dist, idx) of the entries e < total with idx_of(e) >= 0 -- all of different idx --, ascending,
// to od / oi [k]; -1 and NaN where there are fewer.  Round t takes the least entry behind the one of round t - 1: no sort, no
// storage, and every lane ends with the same answer (the butterfly's operation is a minimum of a total order).
template <class FD, class FI> static __device__ void knn_select(int total, int k, FD dist_of, FI idx_of, double *od, int32_t *oi)
{
    const int ln = lane_id();
    double last_d = 0.0;
    int last_i = -1;
    for (int t = 0; t < k; t++) {
        double bd = 0.0;
        int bi = -1;
        if (t == 0 || last_i >= 0) {
            for (int e = ln; e < total; e += 64) {
                const int i = idx_of(e);
                const double d = dist_of(e);
                if (i < 0 || (t > 0 && !knn_before(last_d, last_i, d, i))) continue;
                if (bi < 0 || knn_before(d, i, bd, bi)) { bd = d; bi = i; }
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const double d2 = __shfl_xor(bd, s);
                const int i2 = __shfl_xor(bi, s);
                if (i2 >= 0 && (bi < 0 || knn_before(d2, i2, bd, bi))) { bd = d2; bi = i2; }
            }
        }
        if (ln == 0) { oi[t] = bi; od[t] = bi < 0 ? __builtin_nan("") : bd; }
        last_d = bd;
        last_i = bi;
    }
}

// the least of this lane's cells of P that lie in real columns (column ln * C + jj + 1 <= m); +inf where it has none
template <int C> static __device__ __forceinline__ double knn_lane_min(const double (&P)[C], int ln, int m)
{
    double v = __builtin_inf();
#pragma unroll
    for (int jj = 0; jj < C; jj++) if (ln * C + jj < m) v = fmin(v, P[jj]);
    return v;
}

// grid = queries of the batch (query p0 + block / nseg) * nseg, block = 64 * KNN_WAVES.  q [.., Eq], qc [..]; r [nr, Er], rc [nr]
// (checked by the caller: 1 <= rc <= Er, finite values); excl [..] or null: the reference that does not count.  seg_dist / seg_idx
// [queries of the batch, nseg, k], seg_work [.., nseg, 3] (pairs finished, pairs abandoned, DP steps).  C * 64 >= Er; pmask =
// the period of the abandon test - 1; prune == 0: every pair runs to the end.
template <int C>
__global__ void __launch_bounds__(64 * KNN_WAVES) k_dtw_knn(const double *__restrict__ q, const int32_t *__restrict__ qc, int p0, int Eq,
                                                          const double *__restrict__ r, const int32_t *__restrict__ rc, int nr, int Er, int band,
                                                          int k, int seg_refs, int nseg, int pmask, int prune, const int32_t *__restrict__ excl,
                                                          double *__restrict__ seg_dist, int32_t *__restrict__ seg_idx,
                                                          long long *__restrict__ seg_work)
{
    __shared__ __attribute__((aligned(16))) double qa_[FP_EMAX];
    __shared__ __attribute__((aligned(16))) double slot_[KNN_WAVES];
    __shared__ __attribute__((aligned(16))) double ld_[KNN_WAVES * KNN_KMAX];
    __shared__ __attribute__((aligned(16))) int32_t li_[KNN_WAVES * KNN_KMAX];
    __shared__ __attribute__((aligned(16))) long long wk_[KNN_WAVES * 3];
    __shared__ __attribute__((aligned(16))) int32_t bad_[KNN_WAVES];
    LDS double *qa = (LDS double *)qa_;
    volatile LDS double *slot = (volatile LDS double *)slot_;
    LDS double *ld = (LDS double *)ld_;
    LDS int32_t *li = (LDS int32_t *)li_;
    LDS long long *wk = (LDS long long *)wk_;
    LDS int32_t *badw = (LDS int32_t *)bad_;
    const int ln = lane_id(), w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = (int)(blockIdx.x / (unsigned)nseg), seg = (int)(blockIdx.x % (unsigned)nseg), p = p0 + pl;
    const int n = qc[p];
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const size_t at = (size_t)pl * nseg + seg;
    double *od = seg_dist + at * k;
    int32_t *oi = seg_idx + at * k;
    long long *ow = seg_work + at * 3;
    bool bad = __any(dtw_stage(q + (size_t)p * Eq, n, Eq, qa, (int)threadIdx.x, 64 * KNN_WAVES));
    if (ln == 0) badw[w] = bad ? 1 : 0;
    if (threadIdx.x < KNN_WAVES) slot[threadIdx.x] = inf;
    __syncthreads();
    bad = false;
#pragma unroll
    for (int v = 0; v < KNN_WAVES; v++) bad |= badw[v] != 0;
    if (bad) { // an unusable query: empty lists, no work
        if (w == 0) {
            if (ln < k) { oi[ln] = -1; od[ln] = nan; }
            if (ln < 3) ow[ln] = 0;
        }
        return;
    }
    const int ex = excl ? excl[p] : -1;
    const int j0 = seg * seg_refs, j1 = j0 + seg_refs < nr ? j0 + seg_refs : nr;
    // this wave's list: lane t holds entry t of cnt (t < k), ascending in (dist, idx)
    double myd = inf;
    int myi = -1, cnt = 0;
    long long n_fin = 0, n_ab = 0, n_steps = 0;
    for (int j = j0 + w; j < j1; j += KNN_WAVES) {
        if (j == ex) continue;
        const int m = rc[j];
        double c[C], P[C]; // this lane's reference values and D[row before][its columns]
#pragma unroll
        for (int jj = 0; jj < C; jj++) {
            const int c0 = ln * C + jj;
            c[jj] = c0 < m ? r[(size_t)j * Er + c0] : 0.0;
            P[jj] = inf;
        }
        const int last = dtw_corner_lane<C>(m);
        bool gone = false;
        if (prune && (n > 1 || m > 1)) {
            // THE ENDPOINT BOUND.  Every warping path starts in cell (1, 1) and ends in (n, m), two cells unless n == m == 1, both
            // inside every band (R >= |n - m|).  D[1][1] = fl(d1 * d1 + 0.0) = fl(d1 * d1).  Along the chain of arg-min
            // predecessors from (n, m) back to (1, 1) the values never decrease in floating point -- D[cell] = fl(cost + D[pred])
            // with cost >= 0, and fl(x + c) >= x for c >= 0 (rounding is monotone and x is representable) --, so the predecessor
            // of (n, m) has a value >= fl(d1 * d1), and by the monotonicity of a rounded sum in its operand
            // D[n][m] = fl(fl(dn * dn) + D[pred]) >= fl(fl(dn * dn) + fl(d1 * d1)): the value computed here, in these operations
            // (D is dtw_step's, dtw_wave.h: fl(fl(d * d) + the least predecessor), nothing contracted).
            double cl = 0.0;
#pragma unroll
            for (int jj = 0; jj < C; jj++) if (jj == (m - 1) % C) cl = c[jj];
            const double d1 = qa[0] - __shfl(c[0], 0), dn = qa[n - 1] - __shfl(cl, last);
            const double e = dn * dn + d1 * d1;
            double thr = slot[0];
#pragma unroll
            for (int v = 1; v < KNN_WAVES; v++) thr = fmin(thr, slot[v]);
            gone = e > thr;
        }
        int ran = 0; // the steps made
        if (!gone) {
            const int R = dtw_radius(band, n, m);
            double plold = inf; // D[two rows before the next][its last column]
            const int steps = n + (m - 1) / C;
            // dtw_wave.h's step under a local name (its two sites calling it directly cost a register: profiles/dtw_wave_isa.txt)
            auto step = [&](int s) __attribute__((always_inline)) { dtw_step<C>(s, ln, n, R, qa, c, P, plold); };
            // plain steps up to the next multiple b of the period, then step b with the abandon test around it
            int s = 1;
            for (;;) {
                const int b = prune ? ((s + pmask) & ~pmask) : steps + 1;
                const int stop = b <= steps ? b : steps + 1;
                for (; s < stop; s++) step(s);
                if (b > steps) break;
                // THE FRONTIER BOUND.  Call the TIME of cell (i, j) i + (j - 1) / C: the step at which lane (j - 1) / C computes
                // it (dtw_step, dtw_wave.h: this bound relies on its layout of P and on its +inf outside the band).  A path
                // starts at time 1, in (1, 1), ends at time `steps`, in (n, m), and one warping step -- (i + 1, j),
                // (i, j + 1) or (i + 1, j + 1) -- raises the time by 0, 1 or 2.  So for every 1 <= b <= steps every path holds a
                // cell of time b or b - 1, and so does the chain of arg-min predecessors of (n, m), along which the values never
                // decrease in floating point (above): the least D over the cells of the times b - 1 and b is <= D[n][m].  ONE
                // time alone is no bound -- a diagonal step jumps over it.  Before step b a lane with row i - 1 in [1, n] holds
                // its cells of time b - 1 in P, behind it a lane with row i in [1, n] its cells of time b; a lane with
                // i == n + 1 has its cells of time b - 1 in both.  The other lanes, and the padding columns > m, lie on no path and
                // are left out; cells outside the band are +inf as in the recurrence.  `pm > thr` for every lane that counts:
                // the bound is strictly greater than the threshold.
                double pm = knn_lane_min<C>(P, ln, m);
                step(b);
                s = b + 1;
                pm = fmin(pm, knn_lane_min<C>(P, ln, m));
                double thr = slot[0];
#pragma unroll
                for (int v = 1; v < KNN_WAVES; v++) thr = fmin(thr, slot[v]);
                const int i = b - ln;
                if (!__any(i >= 1 && i <= n + 1 && !(pm > thr))) { gone = true; break; }
            }
            ran = s - 1;
        }
        n_steps += ran;
        if (gone) { n_ab++; continue; }
        n_fin++;
        const double D = __shfl(dtw_corner<C>(P, m), last);
        // into the list: behind the entries that are before (D, j)
        const bool have = ln < cnt;
        const int pos = __popcll(__ballot(have && knn_before(myd, myi, D, j)));
        if (pos < k) {
            const double upd = __shfl_up(myd, 1);
            const int upi = __shfl_up(myi, 1);
            if (ln == pos) { myd = D; myi = j; }
            else if (ln > pos) { myd = upd; myi = upi; }
            if (cnt < k) cnt++;
            if (cnt == k) {
                const double kth = __shfl(myd, k - 1);
                if (ln == 0) slot[w] = kth;
            }
        }
    }
    if (ln < KNN_KMAX) { ld[w * KNN_KMAX + ln] = myd; li[w * KNN_KMAX + ln] = ln < cnt ? myi : -1; }
    if (ln == 0) { wk[w * 3] = n_fin; wk[w * 3 + 1] = n_ab; wk[w * 3 + 2] = n_steps; }
    __syncthreads();
    if (w == 0) {
        knn_select(KNN_WAVES * KNN_KMAX, k, [&](int e) { return ld[e]; }, [&](int e) { return (int)li[e]; }, od, oi);
        if (ln < 3) {
            long long t = 0;
#pragma unroll
            for (int v = 0; v < KNN_WAVES; v++) t += wk[v * 3 + ln];
            ow[ln] = t;
        }
    }
}

// grid = queries of the batch, block = 64: idx / dist [k] of query p0 + block from its nseg lists; work [3] (may be null) their sums
__global__ void __launch_bounds__(64) k_knn_merge(const double *__restrict__ seg_dist, const int32_t *__restrict__ seg_idx,
                                                const long long *__restrict__ seg_work, int nseg, int k, int p0,
                                                int32_t *__restrict__ idx, double *__restrict__ dist, long long *__restrict__ work)
{
    const int pl = blockIdx.x, ln = lane_id();
    const double *sd = seg_dist + (size_t)pl * nseg * k;
    const int32_t *si = seg_idx + (size_t)pl * nseg * k;
    knn_select(nseg * k, k, [&](int e) { return sd[e]; }, [&](int e) { return (int)si[e]; }, dist + (size_t)(p0 + pl) * k,
               idx + (size_t)(p0 + pl) * k);
    if (work && ln < 3) {
        long long t = 0;
        for (int s = 0; s < nseg; s++) t += seg_work[((size_t)pl * nseg + s) * 3 + ln];
        work[(size_t)(p0 + pl) * 3 + ln] = t;
    }
}
