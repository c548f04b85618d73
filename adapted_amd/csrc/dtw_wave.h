// dtw_wave.h -- THE wavefront of the DTW kernels: k_dtw (fingerprint_api.h), k_dtw_pairs (dtw_cluster_api.h), k_dtw_knn
// (dtw_knn_api.h) and k_dtw_align (dtw_align_api.h) state none of it themselves, so one pair gets one distance from all four, in
// every bit (tests/test_gpu_dtw_one_distance.py).  Three things lean on that: the cluster oracle takes the matrix of k_dtw_pairs to
// be symmetric, the two lower bounds of k_dtw_knn speak of the value "computed here, in these operations", and the templates code
// compares k_dtw_align's distances with k_dtw's.  The order of the operations below is the contract (float64, no contraction).
//
// One wave per pair of a row x[0, n) -- staged in LDS -- and a row y[0, m).  Lane l owns the C columns l * C + 1 .. l * C + C of y
// (C * 64 >= m) in registers: c their values, P the cells D[row before][its columns], plold D[two rows before the next][its last
// column].  At step s lane l works on row s - l; its left neighbour's last column of this row and of the row before arrive through a
// lane shift.  A cell's value does not depend on the order of the visits, so the anti-diagonal order gives what the row order
// gives.  Cell (n, m) is done after n + (m - 1) / C steps.  Free functions on the caller's own plain locals: a struct around c, P
// and plold cost registers in most instances.  Loading c (0.0 beyond m) and setting P to +inf stays with the kernels:
// k_dtw_pairs threads its partner's check through that loop, and a shared load cost k_dtw_knn registers.
#pragma once
#include "common.h"

// a row into LDS with its check: x[0, n) -> qa by the threads tid, tid + stride, ...  -> this thread's flag: the row is unusable
// (n outside [1, E], or a value it copied is not finite).  The caller combines the flags and sets the barrier.
static __device__ __forceinline__ bool dtw_stage(const double *__restrict__ x, int n, int E, LDS double *qa, int tid, int stride)
{
    bool bad = n < 1 || n > E;
    if (!bad) {
        for (int i = tid; i < n; i += stride) {
            const double v = x[i];
            qa[i] = v;
            bad |= !__builtin_isfinite(v);
        }
    }
    return bad;
}

// the band radius: none without a band, else at least |n - m|, so that cell (n, m) lies inside
static __device__ __forceinline__ int dtw_radius(int band, int n, int m)
{
    int R = 1 << 30;
    if (band > 0) { const int dm = n > m ? n - m : m - n; R = band > dm ? band : dm; }
    return R;
}

struct DtwNoCodes { __device__ __forceinline__ void operator()(int, unsigned) const {} };

// step s: lane ln computes row i = s - ln of its columns.  Uniform call of the wave (the lane shifts).  CODES: emit(i, code) inside
// the active branch, code holding at bits 2 * jj the predecessor cell jj took -- 0 diagonal, 1 up, 2 left: the least value, the
// diagonal first on equal values, then up --, from the values before the cell is overwritten.
template <int C, bool CODES = false, class F = DtwNoCodes>
static __device__ __forceinline__ void dtw_step(int s, int ln, int n, int R, const LDS double *qa, const double (&c)[C], double (&P)[C],
                                                double &plold, F &&emit = F())
{
    const double inf = __builtin_inf();
    const int i = s - ln;
    const double left_in = __shfl_up(P[C - 1], 1), diag_in = __shfl_up(plold, 1);
    if (i >= 1 && i <= n) {
        const double a = qa[i - 1];
        double left = ln == 0 ? inf : left_in;
        double diag = ln == 0 ? (i == 1 ? 0.0 : inf) : diag_in;
        plold = P[C - 1];
        unsigned code = 0;
#pragma unroll
        for (int jj = 0; jj < C; jj++) {
            const int dj = i - (ln * C + jj + 1);
            const double up = P[jj];
            const double d = a - c[jj];
            if constexpr (CODES) code |= ((diag <= up && diag <= left) ? 0u : (up <= left ? 1u : 2u)) << (2 * jj);
            double v = d * d + fmin(fmin(up, left), diag);
            if (dj > R || dj < -R) v = inf; // (|dj| > R; -R stated so, it is hoisted whatever the caller knows of R)
            diag = up;
            left = v;
            P[jj] = v;
        }
        if constexpr (CODES) emit(i, code);
    }
}

// the lane that owns column m
template <int C> static __device__ __forceinline__ int dtw_corner_lane(int m) { return (m - 1) / C; }

// this lane's value of column m: D[n][m] in lane dtw_corner_lane<C>(m) behind the last step
template <int C> static __device__ __forceinline__ double dtw_corner(const double (&P)[C], int m)
{
    double res = __builtin_inf();
#pragma unroll
    for (int jj = 0; jj < C; jj++) if (jj == (m - 1) % C) res = P[jj];
    return res;
}
