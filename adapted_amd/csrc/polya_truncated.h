// polya_truncated.h -- the device side of ADP_FLAG_TRUNCATED: behind everything else a detect call does, every read whose signal
// goes on past the preloaded window (full_len > m) is looked at once more -- does its poly(A) run into the window's end?
//
//   T1  the last W = cfg.median_shift_window observed samples look like poly(A): the first four entries (mean, var, med, range)
//       of the check vector of mean_var_shift_polyA_check(signal[:obs_end], obs_end - W, obs_end, less_signal_ok = True)
//       (adapted/detect/mvs.py:45-158), the mean range being the configured one or pA_mean_adapter_med_scale_range x the ROW's
//       adapter_med.  One wave per read, the W samples and both moving series in LDS.
//   T2  the reads that passed T1 are validated again with the boundaries (primary adapter end, obs_end), k = 1 and
//       Boundaries.polya_truncated = True (launch_validate over the rows where they lie, SigIdx): "everything observed behind the
//       adapter is poly(A)" is decided by the reference's own gates.
//   merge: a T2 row that passes replaces the read's row (adp_row.reserved_ bit 1); what the first row knew about the primary's
//       poly(A) end, its candidates and the start peak is carried over.
//
// New here:
//   k_pt_t1      eligibility and T1 of every read; marks every row of the call (reserved_ bit 2)
//   k_pt_select  the reads that passed T1, ascending, their count (the host reads it with the call's arena counter and launches
//                nothing more when it is 0), and the call's counts of eligible / passed reads
//   k_pt_gather  per-subset arrays of T2: full_len, (adapter end, obs_end), polya_end_topk given
//   k_pt_preq    Boundaries.polya_truncated for a validation: the RNA partition of every read is all None
//   k_pt_merge   passing T2 rows to their reads' positions in the call's row buffer
#pragma once
#include <cstddef>

#include "common.h"
#include "wave_stats.h"
#include "validate.h"

#define PT_WMAX 4096        // longest median_shift_window T1 holds in LDS (three arrays of W floats beside the wave's scratch)
// k_pt_t1's verdict per read
#define PT_INELIGIBLE 0
#define PT_T1_FAILED 1
#define PT_T1_PASSED 2

// np.median of a NaN-free float32 array in LDS
static __device__ __forceinline__ float pt_median_lds(const LDS float *x, int n, LDS WaveScratch *ws)
{
    float vk, vkm1;
    wave_select2_lds(x, n, n / 2, 0, 0.f, ws, vk, vkm1);
    return (n & 1) ? vk : (vkm1 + vk) / 2.0f;
}

// grid = reads of the call, one wave each; dynamic LDS: 3 * W floats.  The host guarantees 1 <= pA_*_window, both windows + 2 < W
// (the reference takes the windowed statistics then) and W <= PT_WMAX.
__global__ void __launch_bounds__(64) k_pt_t1(const float *__restrict__ sigs, const int32_t *__restrict__ full_len, int n_reads, int m, adp_cfg cfg,
                                              adp_row *__restrict__ rows, int8_t *__restrict__ verdict)
{
    extern __shared__ __attribute__((aligned(16))) float pt_lds_[];
    __shared__ __attribute__((aligned(16))) WaveScratch ws_;
    LDS WaveScratch *ws = (LDS WaveScratch *)&ws_;
    const int r = blockIdx.x, ln = lane_id();
    if (r >= n_reads) return;
    adp_row *row = rows + r;
    const int W = cfg.median_shift_window;
    const long long fl = full_len[r];
    const unsigned long long present = row->present;
    const int fc = row->fail_code;
    const long long ae = (long long)row->col[ADP_C_PRIMARY_ADAPTER_END];
    const double amed = row->col[ADP_C_ADAPTER_MED];
    if (ln == 0) { row->reserved_ |= ADP_ROW_TRUNC_LOOKED; verdict[r] = PT_INELIGIBLE; }
    // (a row of a dropped minibatch is all zero: nothing present)
    if (!(fl > m) || ADP_F_IS_EXCEPTION(fc) || !(present >> ADP_C_PRIMARY_ADAPTER_END & 1) || ae <= 0 || !(present >> ADP_C_ADAPTER_MED & 1) ||
        ae + W > (long long)m)
        return;
    double pr0 = cfg.pA_mean_range[0], pr1 = cfg.pA_mean_range[1];
    if (range_empty(cfg.pA_mean_range)) {
        if (range_empty(cfg.pA_mean_adapter_med_scale_range)) return; // ("pA_mean_range is not specified": such a call's rows are exceptions)
        pr0 = cfg.pA_mean_adapter_med_scale_range[0] * amed;
        pr1 = cfg.pA_mean_adapter_med_scale_range[1] * amed;
    }
    LDS float *sx = (LDS float *)pt_lds_, *svar = sx + W, *smean = svar + W;
    const GLB float *x = (const GLB float *)sigs + (size_t)r * m + (m - W);
    for (int i = ln; i < W; i += 64) sx[i] = x[i];
    __syncthreads();
    // np.median and np.percentile(85) - np.percentile(15) of the window: three ranks of one selection (NaN in the window: all NaN)
    float med; double lrange;
    wave_median_local_range((const LDS float *)sx, W, ws, med, lrange);
    bool ok = in_range_d((double)med, cfg.polyA_med_range[0], cfg.polyA_med_range[1]) &&
              in_range_d(lrange, cfg.polyA_local_range[0], cfg.polyA_local_range[1]);
    if (ok) { // (the window is NaN-free from here on) bottleneck's two recurrences, then their medians
        const int wv = cfg.pA_var_window, wm = cfg.pA_mean_window;
        // ONE call for lanes 0 (variance) and 1 (mean): every step's two LDS reads are issued for both lanes together, so the two
        // chains share their round trips (two calls under `ln == 0` / `ln == 1` would run one chain after the other)
        if (ln < 2) bn_move_slim<const LDS float *, LDS float *>((const LDS float *)sx, W, ln == 0 ? wv : wm, (float *)(ln == 0 ? svar : smean), ln == 0);
        __syncthreads();
        const float fvar = pt_median_lds(svar, W - wv + 1, ws);
        const float fmean = pt_median_lds(smean, W - wm + 1, ws);
        ok = in_range_d((double)fmean, pr0, pr1) && in_range_d((double)fvar, cfg.pA_var_range[0], cfg.pA_var_range[1]);
    }
    if (ln == 0) verdict[r] = ok ? PT_T1_PASSED : PT_T1_FAILED;
}

// One workgroup walks the verdicts SEL_THREADS at a time (sel_step, common.h): ascending read order.
// counts (adp_debug_fetch what = 12; zeroed by the host): [0] eligible reads -- every wave adds its own, [1] reads that passed T1
__global__ void __launch_bounds__(SEL_THREADS) k_pt_select(const int8_t *__restrict__ verdict, int n, int32_t *__restrict__ sel,
                                                           unsigned int *__restrict__ count_out, unsigned int *__restrict__ counts)
{
    int total = 0, eligible = 0;
    for (int r0 = 0; r0 < n; r0 += SEL_THREADS) {
        const int r = r0 + threadIdx.x;
        const int v = r < n ? verdict[r] : PT_INELIGIBLE;
        eligible += __popcll(__ballot(v != PT_INELIGIBLE));
        sel_step(v == PT_T1_PASSED, r, sel, total);
    }
    if (lane_id() == 0 && eligible) atomicAdd(counts, (unsigned int)eligible);
    if (threadIdx.x == 0) { *count_out = (unsigned int)total; counts[1] = (unsigned int)total; }
}

__global__ void __launch_bounds__(256) k_pt_gather(const int32_t *__restrict__ sel, int n_sel, int m, const int32_t *__restrict__ full_len,
                                                   const adp_row *__restrict__ rows, int32_t *__restrict__ len_sub, int64_t *__restrict__ bounds2,
                                                   int8_t *__restrict__ topk_sub)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_sel) return;
    const int r = sel[j];
    const int32_t fl = full_len[r];
    len_sub[j] = fl;
    bounds2[2 * j] = (int64_t)rows[r].col[ADP_C_PRIMARY_ADAPTER_END];
    bounds2[2 * j + 1] = fl < m ? fl : m;
    topk_sub[j] = 0;
}

// between k_validate and k_partition_stats of a validation with Boundaries.polya_truncated (PartReq.p_none bit 1)
__global__ void __launch_bounds__(256) k_pt_preq(PartReq *__restrict__ preq, int n)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n && preq[r].valid) preq[r].p_none |= 2;
}

// one wave per selected read.  Carried over from the first row: the primary's poly(A) end, polya_candidates, the five start-peak
// columns (each with its present bit), start_peak_type and reserved_ bit 0.  counts[2]: rows replaced
__global__ void __launch_bounds__(64) k_pt_merge(const int32_t *__restrict__ sel, int n_sel, const adp_row *__restrict__ rows2, adp_row *__restrict__ rows,
                                                 unsigned int *__restrict__ counts)
{
    const int j = blockIdx.x, ln = lane_id();
    if (j >= n_sel) return;
    if (rows2[j].success != 1) return;
    adp_row *dst_row = rows + sel[j];
    constexpr int NW = (int)(sizeof(adp_row) / 4), COL = (int)(offsetof(adp_row, col) / 4);
    constexpr int W_PPE = COL + 2 * ADP_C_PRIMARY_POLYA_END, W_SP0 = COL + 2 * ADP_C_SP_IDX, W_SP1 = COL + 2 * (ADP_C_SP_OPEN_PORE_IDX + 1);
    constexpr int W_PRESENT = (int)(offsetof(adp_row, present) / 4), W_SPT = (int)(offsetof(adp_row, start_peak_type) / 4);
    constexpr int W_NCAND = (int)(offsetof(adp_row, n_cand) / 4), W_CAND = (int)(offsetof(adp_row, cand) / 4);
    constexpr int W_RES = (int)(offsetof(adp_row, reserved_) / 4);
    constexpr unsigned long long KEEP = (1ull << ADP_C_PRIMARY_POLYA_END) | (31ull << ADP_C_SP_IDX);
    static_assert(ADP_C_SP_OPEN_PORE_IDX == ADP_C_SP_IDX + 4, "the start-peak columns are consecutive");
    const unsigned long long present = (rows2[j].present & ~KEEP) | (dst_row->present & KEEP);
    const int32_t reserved = (dst_row->reserved_ & ADP_ROW_FROM_SECOND_LLR) | ADP_ROW_POLYA_TRUNCATED | ADP_ROW_TRUNC_LOOKED;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows2 + j);
    uint32_t *dst = reinterpret_cast<uint32_t *>(dst_row);
    for (int i = ln; i < NW; i += 64) {
        const bool keep = (i >= W_PPE && i < W_PPE + 2) || (i >= W_SP0 && i < W_SP1) || i == W_SPT || i == W_NCAND ||
                          (i >= W_CAND && i < W_CAND + 2 * ADP_MAX_CAND) || i == W_PRESENT || i == W_PRESENT + 1 || i == W_RES;
        if (!keep) dst[i] = src[i];
    }
    if (ln == 0) { dst_row->present = present; dst_row->reserved_ = reserved; atomicAdd(counts + 2, 1u); }
}
