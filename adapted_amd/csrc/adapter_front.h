// adapter_front.h -- the adapter's front boundary as a post-pass over the rows of a finished detect call (an extension: the
// reference ships moving_mean_adapter_start_detect, adapter_start.py:20-54, and never calls it).  For every row with success == 1
// and an adapter end, with a0 = the row's adapter_start (0 if absent) and ae = its adapter_end, the detector of startmods_api.h
// (as_detect: the arithmetic of k_adapter_start, float32) runs on x = pA[r, a0:ae] of the resident matrix -- float32 rows, or raw
// int16 rows calibrated in registers (common.h: SigI16, NaN at and beyond min(full_len, m)).  With s its result, a read is
// ACCEPTED when s > 0 and ae - (a0 + s) >= min_adapter_len; its row then gets adapter_start = a0 + s, adapter_len and the four
// partition statistics of pA[r, a0 + s:ae] (sigstats_api.h's ss_stats4: numpy's float32 results, as every partition statistic of
// a row) and bit 3 of reserved_.  Nothing else of any row changes, and validation is not repeated.  Compiled in modules.hip only.
//
//   k_adapter_front<Sig>    one wave per read: the detector, the side outputs, the read's segment (start < 0: not accepted)
//   k_seg_stats_sig<Sig>    one workgroup per read: the statistics of an accepted read's segment
//   k_adapter_front_patch   a thread per read: the five columns, adapter_start and the bit into the accepted reads' rows
#pragma once
#include "common.h"
#include "startmods_api.h"
#include "sigstats_api.h"

#define AF_ST_SKIPPED (-1) // info[0] of a read that was not looked at: a failing row, no adapter end, or bounds outside the row

// ws: [gridDim.x, 2, m] floats.  info int32 [n, 4]: status (AF_ST_SKIPPED, AS_ST_OK, AS_ST_VALUE), the exception's window and slice
// size, 1 when the row is to be patched.  shift int64 [n]: s.  cand int64 [n], diff float64 [n]: as k_adapter_start's.
// segs [n]: (r, a0 + s, ae) of an accepted read, start = end = -1 of every other.
template <class Sig>
__global__ void __launch_bounds__(64) k_adapter_front(Sig sig, int n_reads, int m, const adp_row *__restrict__ rows,
                                                      adp_adapter_front_args p, float *ws, int32_t *__restrict__ info_out,
                                                      int64_t *__restrict__ shift_out, int64_t *__restrict__ cand_out,
                                                      double *__restrict__ diff_out, SsSeg *__restrict__ segs)
{
    __shared__ __attribute__((aligned(16))) AsLds<float> b_;
    LDS AsLds<float> *b = (LDS AsLds<float> *)&b_;
    const int ln = lane_id();
    float *wmean = ws + (size_t)blockIdx.x * 2 * m, *wsum = wmean + m;
    const adp_adapter_start_args ap = {p.min_shift, p.min_pA_current, p.window, p.min_obs_adapter};
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const adp_row *row = rows + r;
        AsOut o = {AF_ST_SKIPPED, 0, 0, 0, 0, -1, 0.0};
        SsSeg sg = {-1, -1, r, 0};
        const unsigned long long pres = row->present;
        if (row->success == 1 && (pres >> ADP_C_ADAPTER_END & 1)) { // (the same row in every lane: a uniform branch)
            const long long a0 = (pres >> ADP_C_ADAPTER_START & 1) ? (long long)row->col[ADP_C_ADAPTER_START] : 0;
            const long long ae = (long long)row->col[ADP_C_ADAPTER_END];
            if (a0 >= 0 && a0 <= ae && ae <= m) { // (the slice lies inside the row: nothing outside it is read)
                o = as_detect<float>(sig.row(r, m) + a0, (int)(ae - a0) - p.min_obs_adapter, ap, wmean, wsum, b);
                const bool take = o.res > 0 && ae - (a0 + o.res) >= p.min_adapter_len;
                o.accepted = take ? 1 : 0;
                if (take) { sg.start = a0 + o.res; sg.end = ae; }
            }
        }
        if (ln < 4) info_out[(size_t)r * 4 + ln] = o.info(ln);
        if (ln == 0) { shift_out[r] = o.res; cand_out[r] = o.cand; diff_out[r] = o.dc; segs[r] = sg; }
    }
}

// k_seg_stats (sigstats_api.h) for the rows of a resident matrix of either kind: stats[g, 4] and count[g] of signal[row, start:end]
// clipped to the row's width m (NaN x 4 and 0 for an empty segment: start < 0 or end <= start).  One workgroup per segment.
template <class Sig>
__global__ void __launch_bounds__(SS_BLOCK) k_seg_stats_sig(Sig sig, int n_reads, int m, const SsSeg *__restrict__ segs, int n_seg,
                                                            double *__restrict__ stats, int64_t *__restrict__ count)
{
    __shared__ __attribute__((aligned(16))) SsScratch<float> ws_[1];
    LDS NpSumLdsT<float> *ws = (LDS NpSumLdsT<float> *)&ws_[0].sum;
    LDS SsLds *sl = (LDS SsLds *)&ws_[0].sel;
    const int g = blockIdx.x;
    if (g >= n_seg) return;
    const SsSeg sg = segs[g];
    long long a = 0;
    int n = 0;
    if (sg.row >= 0 && sg.row < n_reads && sg.start >= 0 && sg.end > sg.start) {
        a = sg.start < m ? sg.start : m;
        n = (int)((sg.end < m ? sg.end : m) - a);
    }
    ss_stats4<float>(sig.row(n > 0 ? sg.row : 0, m) + a, n, ws, sl, stats + (size_t)g * 4, count + g);
}

__global__ void __launch_bounds__(256) k_adapter_front_patch(adp_row *__restrict__ rows, int n_reads, const SsSeg *__restrict__ segs,
                                                             const double *__restrict__ stats)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads) return;
    const SsSeg sg = segs[r];
    if (sg.start < 0) return;
    adp_row *row = rows + r;
    row->col[ADP_C_ADAPTER_START] = (double)sg.start;
    row->col[ADP_C_ADAPTER_LEN] = (double)(sg.end - sg.start);
    for (int k = 0; k < 4; k++) row->col[ADP_C_ADAPTER_MEAN + k] = stats[(size_t)r * 4 + k];
    row->present |= 1ull << ADP_C_ADAPTER_START | 31ull << ADP_C_ADAPTER_LEN;
    row->reserved_ |= ADP_ROW_ADAPTER_FRONT;
}
