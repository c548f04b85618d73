// dtw_align_api.h -- the warping path of a DTW alignment and one iteration of DTW barycentre averaging (DBA), for building barcode
// templates (an extension, as fingerprint_api.h is, whose k_dtw this continues).  Compiled in modules.hip only.  Everything is
// float64 in a fixed order of operations, so that a numpy restatement is the exact oracle (tests/dtw_align_oracle.py).  Three kernels:
//
//   k_dtw_align   one wave per query and ITS template (which[p]).  The forward pass is dtw_wave.h's wavefront, which is k_dtw's
//                 (C = ceil(Et / 64) template columns per lane), so the distance has k_dtw's bits.  With its switch on, every
//                 cell also leaves the 2-bit code of the predecessor it took (0 diagonal, 1 up, 2 left: the least value, the
//                 diagonal first on equal values, then up): the C codes of a lane's cells of one row are one unit (a byte; 16 bits
//                 with C = 8), W = ceil(longest template of the call / C) units per row, Eq rows.  The units live in LDS where
//                 Eq * W units fit DA_LDS_CODES bytes (G = false), else in a slice of the call's scratch (G = true).  Lane 0 then
//                 walks back from (n, m) to (1, 1) -- at most n + m - 2 dependent reads -- and leaves the first and the last query
//                 index of every template position in LDS; the lanes sum the query over these runs, a position each, in ascending
//                 order.
//   k_dba_reduce  behind k_dtw_align in a batch of queries, a thread per (template, position): walks the template's members of the
//                 batch in ascending query order (a list made on the host: `which` is a host array) and adds their sums, run
//                 lengths and -- position 0 -- distances onto accumulators that live across the batches, so that every sum is made
//                 in one order whatever the batch size is.
//   k_dba_finish  the new templates from the accumulators.
#pragma once
#include "fingerprint_api.h"

#define DA_LDS_CODES 49152 // the most bytes of direction codes a workgroup keeps in LDS (beside 8 KiB of static arrays)

template <int C> struct DaUnit { using type = uint8_t; };
template <> struct DaUnit<8> { using type = uint16_t; };

// grid = queries of the batch (query p0 + block), block = 64, dynamic LDS = G ? 0 : Eq * W units.  q [.., Eq], qc [..], which [..]
// (-1: skipped; else a template, checked by the caller); t [nt, Et], tc [nt] (checked by the caller: 1 <= tc <= Et, finite values);
// W * C >= every tc, W <= 64; gcodes [queries of the batch, Eq * W] units (G).  dist / status [all queries]; lo / hi / sum
// [queries of the batch, Et].
template <int C, bool G>
__global__ void __launch_bounds__(64) k_dtw_align(const double *__restrict__ q, const int32_t *__restrict__ qc,
                                                const int32_t *__restrict__ which, int p0, int Eq, const double *__restrict__ t,
                                                const int32_t *__restrict__ tc, int Et, int band, int W, unsigned char *gcodes,
                                                double *__restrict__ dist, int32_t *__restrict__ status, int32_t *__restrict__ lo_out,
                                                int32_t *__restrict__ hi_out, double *__restrict__ sum_out)
{
    using U = typename DaUnit<C>::type;
    __shared__ __attribute__((aligned(16))) double qa_[FP_EMAX];
    __shared__ __attribute__((aligned(16))) int32_t lo_[FP_EMAX];
    __shared__ __attribute__((aligned(16))) int32_t hi_[FP_EMAX];
    extern __shared__ __attribute__((aligned(16))) unsigned char da_codes_[];
    LDS double *qa = (LDS double *)qa_;
    LDS int32_t *lo = (LDS int32_t *)lo_, *hi = (LDS int32_t *)hi_;
    LDS U *lcodes = (LDS U *)da_codes_;
    const int ln = lane_id();
    const int pl = (int)blockIdx.x, p = p0 + pl;
    U *gc = (U *)gcodes + (G ? (size_t)pl * Eq * W : (size_t)0);
    const int k = which[p], n = qc[p];
    int32_t *ol = lo_out + (size_t)pl * Et, *oh = hi_out + (size_t)pl * Et;
    double *os = sum_out + (size_t)pl * Et;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    int st = 0;
    if (k < 0) st = 3;
    else if (__any(dtw_stage(q + (size_t)p * Eq, n, Eq, qa, ln, 64))) st = 1;
    __syncthreads();
    double res = nan;
    int m = 0;
    if (st == 0) {
        m = tc[k];
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
        for (int s = 1; s <= steps; s++) {
            dtw_step<C, true>(s, ln, n, R, qa, c, P, plold, [&](int i, unsigned code) {
                if (ln < W) { // (i - 1 < n <= Eq: inside the Eq * W units)
                    if (G) gc[(size_t)(i - 1) * W + ln] = (U)code;
                    else lcodes[(i - 1) * W + ln] = (U)code;
                }
            });
        }
        res = __shfl(dtw_corner<C>(P, m), dtw_corner_lane<C>(m));
        if (!__builtin_isfinite(res)) st = 2;
    }
    __syncthreads(); // (the codes, of other lanes: LDS, or global memory inside the workgroup)
    if (st == 0) {
        if (ln == 0) {
            int i = n, j = m;
            hi[m - 1] = n - 1;
            while (i > 1 || j > 1) {
                unsigned dir;
                if (i == 1) dir = 2u;
                else if (j == 1) dir = 1u;
                else {
                    const int jc = j - 1;
                    const unsigned u = G ? (unsigned)gc[(size_t)(i - 1) * W + jc / C] : (unsigned)lcodes[(i - 1) * W + jc / C];
                    dir = (u >> (2 * (jc % C))) & 3u;
                }
                if (dir != 1u) { lo[j - 1] = i - 1; j--; }
                if (dir != 2u) i--;
                if (dir != 1u) hi[j - 1] = i - 1;
            }
            lo[0] = 0;
        }
        __syncthreads();
    }
    for (int j = ln; j < Et; j += 64) {
        int l = -1, r = -1;
        double sum = nan;
        if (st == 0 && j < m) {
            l = lo[j];
            r = hi[j];
            sum = qa[l];
            for (int i = l + 1; i <= r; i++) sum += qa[i];
        }
        ol[j] = l;
        oh[j] = r;
        os[j] = sum;
    }
    if (ln == 0) {
        dist[p] = res;
        status[p] = st;
    }
}

// block = 64, a thread per (template k, position j) of nt * Et.  list [offs[k], offs[k + 1]): the queries whose template is k, in
// ascending order (of all queries of the call); the batch is the queries [p0, p0 + nb).  T / N [nt, Et], members / inertia [nt]:
// zero before the first batch.
__global__ void __launch_bounds__(64) k_dba_reduce(const int32_t *__restrict__ offs, const int32_t *__restrict__ list, int p0, int nb,
                                                 int nt, int Et, const int32_t *__restrict__ tc, const int32_t *__restrict__ status,
                                                 const double *__restrict__ dist, const int32_t *__restrict__ lo,
                                                 const int32_t *__restrict__ hi, const double *__restrict__ sum, double *__restrict__ T,
                                                 long long *__restrict__ N, int32_t *__restrict__ members, double *__restrict__ inertia)
{
    const size_t idx = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (size_t)nt * Et) return;
    const int k = (int)(idx / (unsigned)Et), j = (int)(idx % (unsigned)Et);
    if (j >= tc[k]) return;
    const int end = offs[k + 1];
    int a = offs[k], b = end; // the first member at or behind p0
    while (a < b) {
        const int mid = a + (b - a) / 2;
        if (list[mid] < p0) a = mid + 1;
        else b = mid;
    }
    double acc = T[idx], in = j == 0 ? inertia[k] : 0.0;
    long long cnt = N[idx];
    int mem = 0;
    for (; a < end; a++) {
        const int p = list[a];
        if (p >= p0 + nb) break;
        if (status[p] != 0) continue;
        const size_t at = (size_t)(p - p0) * Et + j;
        acc += sum[at];
        cnt += hi[at] - lo[at] + 1;
        if (j == 0) { in += dist[p]; mem++; }
    }
    T[idx] = acc;
    N[idx] = cnt;
    if (j == 0) { inertia[k] = in; members[k] += mem; }
}

// block = 64, a thread per (template, position): T / N inside the count of a template with members, its old value without, NaN
// at and beyond the count
__global__ void __launch_bounds__(64) k_dba_finish(const double *__restrict__ t, const int32_t *__restrict__ tc, int nt, int Et,
                                                 const double *__restrict__ T, const long long *__restrict__ N,
                                                 const int32_t *__restrict__ members, double *__restrict__ t_new)
{
    const size_t idx = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (size_t)nt * Et) return;
    const int k = (int)(idx / (unsigned)Et), j = (int)(idx % (unsigned)Et);
    double v = __builtin_nan("");
    if (j < tc[k]) v = members[k] > 0 ? T[idx] / (double)N[idx] : t[idx];
    t_new[idx] = v;
}
