// llr_detect_api.h -- the rest of the reference's native module (adapted/detect/_c_llr.pyx): `_best_split` (:40-64) and the
// unnormalised best-split segmenters `c_llr_detect_adapter` (:239-287) / `c_llr_detect_adapter_polya` (:290-365), batched per read.
//
// A detect call is a short chain of launches on the handle's stream:
//   k_trace_cumsum<T>    np.cumsum(raw), np.cumsum(raw * raw): the sequential chains of trace_api.h (float32 rows are widened
//                        first: exact, so the sums are those of x.astype(float64))
//   k_cd_plan            the segments of the next level, from the splits found so far (level 0: [0, len - 1); level 1: the head
//                        [0, x_first) and tail [x_first, len - 1) of the first split)
//   k_split_part         one chunk of CD_CHUNK split points of one segment per workgroup -> the chunk's best (gain, index)
//   k_split_reduce       the chunks of a segment, in order -> the segment's (x, gain) into its slot of the per-read state
//   k_cd_medians         the four segment medians over the whole read (exact: radix select on order-preserving 64-bit keys),
//                        the reference's decision (:262-287 / :313-351) and, with poly(A), the segment of the 4th split
//   k_split_part/_reduce the poly(A) split, then k_cd_finish writes the rows.
// No gain array is written: a split point's gain lives in registers until its chunk's winner is known.
//
// The winner rule is the reference's loop: best starts at 0.0, a gain must be STRICTLY greater, so NaN and gains <= 0 never win
// and the first index of the maximum does; nothing wins -> (x = -1, gain 0.0).  A chunk keeps the first of its maxima (each
// lane walks its points in increasing order, the lanes and waves are combined with the lower index winning ties) and the
// chunks are combined in the same way.
#pragma once
#include "common.h"
#include "log_cr.h"
#include "trace_api.h"

constexpr int CD_BLOCK = 256;          // k_split_part: lanes per workgroup
constexpr int CD_PER = 16;             // split points per lane
constexpr int CD_CHUNK = CD_BLOCK * CD_PER;
constexpr int CD_MED_BLOCK = 512;      // k_cd_medians: one workgroup per read

// one split search: points i in [lo, hi) of the segment [start, end) of read `row`; the result goes to state slot `slot`
// (row < 0: no search, the slot gets (-1, 0.0))
struct CdSeg { int32_t row, start, end, lo, hi, slot; };

// (a, xa) <- the better of (a, xa) and (b, xb): the larger gain, the lower index on a tie; an empty candidate is (0.0, -1) and a
// real one has a gain > 0, so the two never tie
static __device__ __forceinline__ void cd_better(double &a, int &xa, double b, int xb)
{
    if (b > a || (b == a && xb >= 0 && (xa < 0 || xb < xa))) { a = b; xa = xb; }
}

static __device__ __forceinline__ void cd_wave_best(double &g, int &x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double og = __shfl_xor(g, o, 64);
        const int ox = __shfl_xor(x, o, 64);
        cd_better(g, x, og, ox);
    }
}

// grid = (n_seg, n_chunks), block = CD_BLOCK.  part_g / part_x [n_seg][n_chunks].
__global__ void __launch_bounds__(CD_BLOCK) k_split_part(const double *__restrict__ c, const double *__restrict__ c2, int L,
                                                         const CdSeg *__restrict__ segs, int n_chunks, double *__restrict__ part_g,
                                                         int32_t *__restrict__ part_x)
{
    __shared__ __attribute__((aligned(16))) double lt_[3 * LOGCR_N];
    __shared__ __attribute__((aligned(16))) double wg[CD_BLOCK / 64];
    __shared__ __attribute__((aligned(16))) int wx[CD_BLOCK / 64];
    const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const CdSeg sg = segs[s];
    const long p0 = (long)sg.lo + (long)b * CD_CHUNK;
    const size_t po = (size_t)s * n_chunks + b;
    if (sg.row < 0 || p0 >= sg.hi) { // (uniform in the workgroup)
        if (t == 0) { part_g[po] = 0.0; part_x[po] = -1; }
        return;
    }
    for (int i = t; i < 3 * LOGCR_N; i += CD_BLOCK) lt_[i] = g_logcr_table[i];
    __syncthreads();
    const LDS double *lt = (const LDS double *)lt_;
    auto flog = [&](double v) { return log_cr_impl(v, lt, [](double u) { return log(u); }); };
    const double *cr = c + (size_t)sg.row * L, *c2r = c2 + (size_t)sg.row * L;
    const long start = sg.start, end = sg.end;
    const double vs = (double)(end - start) * flog(llr_var_c(cr, c2r, start, end));
    const long p1 = min((long)sg.hi, p0 + CD_CHUNK);
    double best = 0.0;
    int bx = -1;
    for (long i = p0 + t; i < p1; i += CD_BLOCK) {
        const double g = llr_gain_at(cr, c2r, start, end, i, vs, flog);
        if (g > best) { best = g; bx = (int)i; }
    }
    cd_wave_best(best, bx);
    if ((t & 63) == 0) { wg[t >> 6] = best; wx[t >> 6] = bx; }
    __syncthreads();
    if (t == 0) {
        double g = wg[0];
        int x = wx[0];
        for (int w = 1; w < CD_BLOCK / 64; w++) cd_better(g, x, wg[w], wx[w]);
        part_g[po] = g; part_x[po] = x;
    }
}

// grid = n_seg, block = 64: the chunks of a segment -> st_x / st_g [slot]
__global__ void __launch_bounds__(64) k_split_reduce(const CdSeg *__restrict__ segs, int n_chunks, const double *__restrict__ part_g,
                                                     const int32_t *__restrict__ part_x, int32_t *__restrict__ st_x, double *__restrict__ st_g)
{
    const int s = blockIdx.x, ln = threadIdx.x;
    double g = 0.0;
    int x = -1;
    for (int k = ln; k < n_chunks; k += 64) cd_better(g, x, part_g[(size_t)s * n_chunks + k], part_x[(size_t)s * n_chunks + k]);
    cd_wave_best(g, x);
    if (ln == 0) { st_x[segs[s].slot] = x; st_g[segs[s].slot] = g; }
}

struct CdArgs { int min_obs_adapter, border_trim, min_obs_polya, polya; };

// per-read state, slot r * 4 + k: k = 0 the first split, 1 the head, 2 the tail, 3 the poly(A) split
// res [n][4]: adapter_start, adapter_end, polya_end, the length of the reference's tuple (2 or 3)

// level 0: [0, len - 1) with (min_obs_adapter + border_trim, border_trim) -- segs[r];  level 1: the head [0, x_first) with
// (border_trim, min_obs_adapter) -- segs[2r] -- and the tail [x_first, len - 1) with (min_obs_adapter, border_trim) -- segs[2r + 1];
// none when x_first = -1 (the reference's result is (0, 0) then, whatever those two searches give).  A thread per read.
static __device__ CdSeg cd_seg(int row, long start, long end, long oh, long ot, int slot)
{
    long lo = start + oh, hi = end - ot;
    if (lo > end) lo = end;
    if (hi < lo) hi = lo; // (an empty range: the loop does not run)
    return CdSeg{row, (int32_t)start, (int32_t)end, (int32_t)lo, (int32_t)hi, slot};
}

__global__ void k_cd_plan(int level, const int32_t *__restrict__ len, int n_reads, CdArgs a, const int32_t *__restrict__ st_x,
                          CdSeg *__restrict__ segs)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const long length = (long)len[r] - 1, mo = a.min_obs_adapter, bt = a.border_trim;
    if (level == 0) {
        segs[r] = cd_seg(r, 0, length, mo + bt, bt, r * 4);
    } else {
        const long xf = st_x[r * 4];
        if (xf < 0) {
            segs[2 * r] = CdSeg{-1, 0, 0, 0, 0, r * 4 + 1};
            segs[2 * r + 1] = CdSeg{-1, 0, 0, 0, 0, r * 4 + 2};
        } else {
            segs[2 * r] = cd_seg(r, 0, xf, bt, mo, r * 4 + 1);
            segs[2 * r + 1] = cd_seg(r, xf, length, mo, bt, r * 4 + 2);
        }
    }
}

// The medians of raw[:x_head], raw[x_head:x_first], raw[x_first:x_tail], raw[x_tail:] (after the reference's fallbacks
// x_head = 1 / x_tail = x_first + 1) with numpy's rules -- a NaN anywhere in the segment or an empty segment gives NaN, an even
// count the mean (a + b) / 2.0 of the two middle values -- then the decision.  One workgroup per read.
//
// Selection: radix select on 64-bit keys, 8 bits per pass, 8 passes -- a bounded number, whatever the values: a bucket that
// holds every sample (a constant run, values on a coarse grid) only means the next pass looks at the same samples again.  The
// order statistics wanted (the lower and, for an even count, upper middle of each segment: up to 8) are followed together: every
// pass reads the read once, and a sample is counted in the histogram of each statistic of its segment whose key prefix it shares.
// Segments are tested one by one, so they may overlap or be empty.
template <class T>
__global__ void __launch_bounds__(CD_MED_BLOCK) k_cd_medians(const T *__restrict__ raw, const int32_t *__restrict__ len, int L, CdArgs a,
                                                            const int32_t *__restrict__ st_x, const double *__restrict__ st_g,
                                                            int32_t *__restrict__ res, double *__restrict__ med_out, CdSeg *__restrict__ psegs)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[8][256];
    __shared__ __attribute__((aligned(16))) uint64_t pre[8];
    __shared__ __attribute__((aligned(16))) long rank[8];
    __shared__ __attribute__((aligned(16))) int nan_in[4];
    const int r = blockIdx.x, t = threadIdx.x;
    const long n = len[r], length = n - 1;
    const long xf = st_x[r * 4];
    if (xf < 0) { // (uniform) the reference returns (0, 0) before any median, from both functions
        if (t == 0) {
            res[r * 4] = 0; res[r * 4 + 1] = 0; res[r * 4 + 2] = 0; res[r * 4 + 3] = 2;
            for (int k = 0; k < 4; k++) med_out[r * 4 + k] = 0.0;
            if (a.polya) psegs[r] = CdSeg{-1, 0, 0, 0, 0, r * 4 + 3};
        }
        return;
    }
    long xh = st_x[r * 4 + 1], xt = st_x[r * 4 + 2];
    if (xh == -1) xh = 1;
    if (xt == -1) xt = xf + 1;
    const long b[5] = {0, xh, xf, xt, n};
    long cnt[4];
    for (int s = 0; s < 4; s++) cnt[s] = b[s + 1] > b[s] ? b[s + 1] - b[s] : 0;
    if (t < 8) { pre[t] = 0; rank[t] = (t & 1) ? cnt[t >> 1] / 2 : (cnt[t >> 1] - 1) / 2; }
    if (t < 4) nan_in[t] = 0;
    const T *x = raw + (size_t)r * L;
    // (a statistic is followed when its segment is non-empty; the upper middle only for an even count)
    unsigned live = 0;
    for (int s = 0; s < 4; s++) {
        if (cnt[s] > 0) live |= 1u << (2 * s);
        if (cnt[s] > 0 && (cnt[s] & 1) == 0) live |= 2u << (2 * s);
    }
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        const uint64_t hm = pass == 0 ? 0 : ~0ULL << (shift + 8);
        for (int i = t; i < 8 * 256; i += CD_MED_BLOCK) (&hist[0][0])[i] = 0;
        __syncthreads();
        uint64_t pk[8];
#pragma unroll
        for (int k = 0; k < 8; k++) pk[k] = pre[k];
        for (long i = t; i < n; i += CD_MED_BLOCK) {
            const double v = (double)x[i];
            const uint64_t key = d2key(v);
            const bool isn = v != v;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                if (i < b[s] || i >= b[s + 1]) continue;
                if (isn) { if (pass == 0) nan_in[s] = 1; continue; }
                const unsigned d = (unsigned)(key >> shift) & 255u;
                if ((live >> (2 * s)) & 1u && ((key ^ pk[2 * s]) & hm) == 0) atomicAdd(&hist[2 * s][d], 1u);
                if ((live >> (2 * s + 1)) & 1u && ((key ^ pk[2 * s + 1]) & hm) == 0) atomicAdd(&hist[2 * s + 1][d], 1u);
            }
        }
        __syncthreads();
        if (t < 8 && ((live >> t) & 1u)) {
            long k = rank[t], below = 0;
            int d = 0;
            for (; d < 255; d++) {
                const long h = hist[t][d];
                if (below + h > k) break;
                below += h;
            }
            rank[t] = k - below;
            pre[t] |= (uint64_t)d << shift;
        }
        __syncthreads();
    }
    if (t != 0) return;
    double m[4];
    for (int s = 0; s < 4; s++) {
        if (cnt[s] == 0 || nan_in[s]) m[s] = __builtin_nan("");
        else if (cnt[s] & 1) m[s] = key2d(pre[2 * s]);
        else m[s] = (key2d(pre[2 * s]) + key2d(pre[2 * s + 1])) / 2.0;
        med_out[r * 4 + s] = m[s];
    }
    // np.diff(medians)[1] > 0; medians[0] >= medians.mean() (numpy's sum of four from 0.0, in order, then / 4)
    const double mean = ((((0.0 + m[0]) + m[1]) + m[2]) + m[3]) / 4.0;
    const double gh = st_g[r * 4 + 1], gt = st_g[r * 4 + 2];
    long as = 0, ae = 0;
    if (m[2] - m[1] > 0) { as = m[0] >= mean ? xh : 0; ae = xf; }
    else if (gt > gh) { as = xf; ae = xt; }
    res[r * 4] = (int32_t)as; res[r * 4 + 1] = (int32_t)ae; res[r * 4 + 2] = 0; res[r * 4 + 3] = a.polya ? 3 : 2;
    if (a.polya) {
        // the poly(A) end: a split of [adapter_end, len - 1) with (min_obs_polya, border_trim), unless no adapter was found
        if (ae == 0) psegs[r] = CdSeg{-1, 0, 0, 0, 0, r * 4 + 3};
        else psegs[r] = cd_seg(r, ae, length, a.min_obs_polya, a.border_trim, r * 4 + 3);
    }
}

// the poly(A) split into the rows: -1 (nothing found) -> 0.  A thread per read.
__global__ void k_cd_finish(int n_reads, const int32_t *__restrict__ st_x, int32_t *__restrict__ res)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads || res[r * 4 + 3] != 3 || res[r * 4 + 1] == 0) return;
    const int p = st_x[r * 4 + 3];
    res[r * 4 + 2] = p < 0 ? 0 : p;
}
