// dtw_cluster_api.h -- clustering fingerprints without labels: the all-pairs DTW matrix, PAM's BUILD, alternating k-medoids and
// the silhouette, all on a matrix that stays on the device (an extension, as fingerprint_api.h is, whose k_dtw the pair kernel
// continues).  Compiled in modules.hip only.  Everything is float64 in a fixed order of operations, so that a numpy restatement is
// the exact oracle (tests/dtw_cluster_oracle.py).  No float atomics: nothing depends on scheduling.  The kernels:
//
//   k_dtw_pairs    one wave per row i and a strip of CL_STRIP partners j.  Row i is staged once in LDS and checked once; per partner
//                  dtw_wave.h's wavefront, which is k_dtw's (C = ceil(E / 64) of the partner's columns per lane), so a pair has k_dtw's
//                  bits, and -- the recurrence being symmetric in its operands to the bit -- the bits of either order.  mirror: the
//                  partners of row i are (i + d) % n for d = 1 .. (n - 1) / 2 (and d = n / 2 for i < n / 2 with an even n): every
//                  unordered pair once, the same number of pairs for every row (no long and short rows), and both entries written.
//                  Without mirror (a band of rows for a host matrix over the byte budget): every other row, one entry written.
//   k_cl_check     a matrix entry that is NaN, negative or infinite raises a flag (a plain store of 1: every writer writes the same).
//   k_cl_rowsum    one wave per row: the sum of a row's terms in THE order of the header (cl_fold: 64 lane partials over the columns
//                  j = l (mod 64) in ascending j, then p[l] += p[l + s] for s = 32 .. 1).  The terms: D[i][j], or BUILD's
//                  max(dmin[j] - D[i][j], 0.0).
//   k_cl_pick      one workgroup: the least (row sums) or the greatest (gains, of the rows that are no medoid yet) value, the lowest
//                  index on ties; the row becomes medoid c and dmin takes its row in.
//   k_cl_assign    a thread per row: the slot of the nearest medoid (its own for a medoid), and that distance.
//   k_cl_sums      one wave per row: sums[i][c] over the members j of every cluster c, a lane adding into its private column of
//                  an LDS table [CL_KC clusters of the chunk][64]; lane c then folds cluster c.  Serves the update, and the silhouette.
//   k_cl_total     one wave: the cost, the rows' distances to their medoids added in THE order (over the row index).
//   k_cl_update    one workgroup per cluster: the member of the least sums[i][c], the lowest index on ties.
//   k_cl_sil       a thread per row: the silhouette from sums and sizes.
#pragma once
#include "fingerprint_api.h"

#define CL_NMAX 16384 // the most rows of a distance matrix
#define CL_KMAX 4096  // the most clusters
#define CL_STRIP 16   // partners of one workgroup of k_dtw_pairs
#define CL_KC 32      // clusters of one pass of k_cl_sums over a row
#define CL_PAD 65     // doubles per cluster in its table (64 and one: lane c's fold walks its row without bank conflicts)

// THE fold of the header: lane l holds partial l; -> lane 0 holds the sum (the other lanes: no meaning)
static __device__ __forceinline__ double cl_fold(double p)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p += __shfl_down(p, s);
    return p;
}

// grid = rows of the call (row r0 + block / nchunks) * nchunks, block = 64.  q [n, E], qc [n].  out [rows of the call, n] (mirror:
// r0 == 0 and all n rows).  C * 64 >= E.
template <int C>
__global__ void __launch_bounds__(64) k_dtw_pairs(const double *__restrict__ q, const int32_t *__restrict__ qc, int n, int E, int band,
                                                int r0, int nchunks, int mirror, double *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) double qa_[FP_EMAX];
    LDS double *qa = (LDS double *)qa_;
    const int ln = lane_id();
    const int il = (int)(blockIdx.x / (unsigned)nchunks), chunk = (int)(blockIdx.x % (unsigned)nchunks), i = r0 + il;
    const int na = qc[i];
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const bool bad_i = __any(dtw_stage(q + (size_t)i * E, na, E, qa, ln, 64));
    __syncthreads();
    double *orow = out + (size_t)il * n;
    if (chunk == 0 && ln == 0) orow[i] = bad_i ? nan : 0.0;
    const int partners = mirror ? (n - 1) / 2 + ((n % 2 == 0 && i < n / 2) ? 1 : 0) : n - 1;
    const int d0 = 1 + chunk * CL_STRIP;
    const int d1 = d0 + CL_STRIP - 1 < partners ? d0 + CL_STRIP - 1 : partners;
    for (int dd = d0; dd <= d1; dd++) {
        int j = i + dd;
        if (j >= n) j -= n;
        const int m = qc[j];
        bool bad = bad_i || m < 1 || m > E;
        double c[C], P[C]; // this lane's columns of the partner and D[row before][its columns]
#pragma unroll
        for (int jj = 0; jj < C; jj++) {
            const int j0 = ln * C + jj;
            c[jj] = (!bad && j0 < m) ? q[(size_t)j * E + j0] : 0.0;
            bad |= !__builtin_isfinite(c[jj]);
            P[jj] = inf;
        }
        bad = __any(bad);
        double res = nan;
        int last = 0;
        if (!bad) {
            const int R = dtw_radius(band, na, m);
            double plold = inf; // D[two rows before the next][its last column]
            const int steps = na + (m - 1) / C;
            for (int s = 1; s <= steps; s++) dtw_step<C>(s, ln, na, R, qa, c, P, plold);
            res = dtw_corner<C>(P, m);
            last = dtw_corner_lane<C>(m);
        }
        if (ln == last) {
            orow[j] = res;
            if (mirror) out[(size_t)j * n + i] = res;
        }
    }
}

// block = 256, any grid: flag[0] = 1 where an entry of d [count] is NaN, negative or infinite
__global__ void __launch_bounds__(256) k_cl_check(const double *__restrict__ d, size_t count, int32_t *__restrict__ flag)
{
    bool bad = false;
    for (size_t at = (size_t)blockIdx.x * 256 + threadIdx.x; at < count; at += (size_t)gridDim.x * 256) {
        const double v = d[at];
        bad |= !(v >= 0.0 && v < __builtin_inf());
    }
    if (bad) flag[0] = 1;
}

// grid = n, block = 64.  GAIN: out[i] = the sum over j of max(dmin[j] - D[i][j], 0.0), else of D[i][j]: THE order
template <bool GAIN>
__global__ void __launch_bounds__(64) k_cl_rowsum(const double *__restrict__ D, int n, const double *__restrict__ dmin, double *__restrict__ out)
{
    const int i = blockIdx.x, ln = lane_id();
    const double *row = D + (size_t)i * n;
    double p = 0.0;
    for (int j = ln; j < n; j += 64) {
        double t = row[j];
        if (GAIN) { t = dmin[j] - t; t = t > 0.0 ? t : 0.0; }
        p += t;
    }
    p = cl_fold(p);
    if (ln == 0) out[i] = p;
}

// is (v1, i1) before (v2, i2)?  MAX: the greater value first, else the less; the lower index on equal values; an index < 0: no entry
template <bool MAX> static __device__ __forceinline__ bool cl_before(double v1, int i1, double v2, int i2)
{
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    if (v1 != v2) return MAX ? v1 > v2 : v1 < v2;
    return i1 < i2;
}

// the first of the entries (v, i) of a workgroup of 256 threads, for all its threads (sv / si: 256 entries of LDS each)
template <bool MAX> static __device__ int cl_first(double v, int i, LDS double *sv, LDS int32_t *si, double *vout)
{
    const int t = threadIdx.x;
    __syncthreads();
    sv[t] = v;
    si[t] = i;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s && cl_before<MAX>(sv[t + s], si[t + s], sv[t], si[t])) { sv[t] = sv[t + s]; si[t] = si[t + s]; }
        __syncthreads();
    }
    *vout = sv[0];
    return si[0];
}

// grid = 1, block = 256.  c == 0: the row of the least vals (the row sums); else the row that is no medoid with the greatest vals
// (the gains); the lowest index on ties.  It becomes medoids[c] with gain[c] = its value; dmin[j] = D[it][j] (c == 0), else the
// lesser of dmin[j] and D[it][j].
__global__ void __launch_bounds__(256) k_cl_pick(const double *__restrict__ D, int n, int c, const double *__restrict__ vals,
                                               int32_t *__restrict__ ismed, int32_t *__restrict__ medoids, double *__restrict__ gain,
                                               double *__restrict__ dmin)
{
    __shared__ __attribute__((aligned(16))) double sv_[256];
    __shared__ __attribute__((aligned(16))) int32_t si_[256];
    LDS double *sv = (LDS double *)sv_;
    LDS int32_t *si = (LDS int32_t *)si_;
    const int t = threadIdx.x;
    double bv = 0.0, v;
    int bi = -1, pick;
    if (c == 0) {
        for (int i = t; i < n; i += 256) if (cl_before<false>(vals[i], i, bv, bi)) { bv = vals[i]; bi = i; }
        pick = cl_first<false>(bv, bi, sv, si, &v);
    } else {
        for (int i = t; i < n; i += 256) if (!ismed[i] && cl_before<true>(vals[i], i, bv, bi)) { bv = vals[i]; bi = i; }
        pick = cl_first<true>(bv, bi, sv, si, &v);
    }
    if (pick < 0) return; // (kmax <= n: there is a row left)
    const double *row = D + (size_t)pick * n;
    for (int j = t; j < n; j += 256) {
        const double d = row[j];
        dmin[j] = (c == 0 || d < dmin[j]) ? d : dmin[j];
    }
    if (t == 0) { ismed[pick] = 1; medoids[c] = pick; gain[c] = v; }
}

// block = 64, a thread per row: assign[i] = the slot whose medoid is i, else the slot of the least D[i][med[c]] (the lowest on
// ties); dnear[i] = D[i][med[assign[i]]]
__global__ void __launch_bounds__(64) k_cl_assign(const double *__restrict__ D, int n, const int32_t *__restrict__ med, int k,
                                                int32_t *__restrict__ assign, double *__restrict__ dnear)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double *row = D + (size_t)i * n;
    int best = -1;
    double bd = 0.0;
    for (int c = 0; c < k; c++) {
        const int m = med[c];
        const double d = row[m];
        if (m == i) { best = c; bd = d; break; }
        if (best < 0 || d < bd) { best = c; bd = d; }
    }
    assign[i] = best;
    dnear[i] = bd;
}

// grid = n, block = 64: sums[i][c] = the sum over the members j of c (assign[j] == c) of D[i][j], THE order, for every c < k
__global__ void __launch_bounds__(64) k_cl_sums(const double *__restrict__ D, int n, const int32_t *__restrict__ assign, int k,
                                              double *__restrict__ sums)
{
    __shared__ __attribute__((aligned(16))) double tab_[CL_KC * CL_PAD];
    LDS double *tab = (LDS double *)tab_;
    const int i = blockIdx.x, ln = lane_id();
    const double *row = D + (size_t)i * n;
    for (int c0 = 0; c0 < k; c0 += CL_KC) {
        __syncthreads();
        for (int c = 0; c < CL_KC; c++) tab[c * CL_PAD + ln] = 0.0;
        for (int j = ln; j < n; j += 64) { // (lane l alone touches column l of the table: no barrier inside)
            const int c = assign[j] - c0;
            if (c >= 0 && c < CL_KC) tab[c * CL_PAD + ln] += row[j];
        }
        __syncthreads();
        if (ln < CL_KC && c0 + ln < k) {
            LDS double *p = tab + ln * CL_PAD;
            for (int s = 32; s >= 1; s >>= 1)
                for (int l = 0; l < s; l++) p[l] += p[l + s];
            sums[(size_t)i * k + c0 + ln] = p[0];
        }
    }
}

// grid = 1, block = 64: out[0] = the sum of v [n], THE order (over the index)
__global__ void __launch_bounds__(64) k_cl_total(const double *__restrict__ v, int n, double *__restrict__ out)
{
    const int ln = lane_id();
    double p = 0.0;
    for (int j = ln; j < n; j += 64) p += v[j];
    p = cl_fold(p);
    if (ln == 0) out[0] = p;
}

// grid = k, block = 256: med_new[c] = the member i of c with the least sums[i][c], the lowest index on ties (a cluster holds its
// medoid: it is never empty); changed[0] = 1 where that is not med[c]
__global__ void __launch_bounds__(256) k_cl_update(const double *__restrict__ sums, int n, int k, const int32_t *__restrict__ assign,
                                                 const int32_t *__restrict__ med, int32_t *__restrict__ med_new, int32_t *__restrict__ changed)
{
    __shared__ __attribute__((aligned(16))) double sv_[256];
    __shared__ __attribute__((aligned(16))) int32_t si_[256];
    LDS double *sv = (LDS double *)sv_;
    LDS int32_t *si = (LDS int32_t *)si_;
    const int c = blockIdx.x, t = threadIdx.x;
    double bv = 0.0, v;
    int bi = -1;
    for (int i = t; i < n; i += 256) {
        if (assign[i] != c) continue;
        const double s = sums[(size_t)i * k + c];
        if (cl_before<false>(s, i, bv, bi)) { bv = s; bi = i; }
    }
    const int pick = cl_first<false>(bv, bi, sv, si, &v);
    if (t == 0) {
        const int m = pick < 0 ? med[c] : pick;
        med_new[c] = m;
        if (m != med[c]) changed[0] = 1;
    }
}

// block = 64, a thread per row: a = sums[i][own] / (size[own] - 1), b = the least sums[i][c] / size[c] over the other clusters,
// sil = (b - a) / max(a, b); 0.0 for a cluster of one, for max(a, b) == 0 and for k == 1
__global__ void __launch_bounds__(64) k_cl_sil(const double *__restrict__ sums, int n, int k, const int32_t *__restrict__ assign,
                                             const int32_t *__restrict__ size, double *__restrict__ sil)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int own = assign[i];
    double s = 0.0;
    if (k > 1 && size[own] > 1) {
        const double a = sums[(size_t)i * k + own] / (double)(size[own] - 1);
        double b = 0.0;
        bool have = false;
        for (int c = 0; c < k; c++) {
            if (c == own) continue;
            const double m = sums[(size_t)i * k + c] / (double)size[c];
            if (!have || m < b) { b = m; have = true; }
        }
        const double mx = a > b ? a : b;
        s = mx == 0.0 ? 0.0 : (b - a) / mx;
    }
    sil[i] = s;
}
