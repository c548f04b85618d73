// adapter_front_revalidate.h -- the device side of adp_adapter_front_revalidate(_i16): the reads the front detector accepted
// (k_adapter_front, adapter_front.h) are validated again with Boundaries.adapter_start = the trimmed start, by the pattern of
// polya_truncated.h's T2 and cnn_second_opinion.h: select, gather, launch_validate over the rows where they lie (SigIdx /
// SigIdxI16, k_validate<SIG, true>), merge.  A re-validated row that passes replaces the read's row; one that fails leaves the
// read's row as it was -- the trim is then rejected.
//
//   k_afr_select   the accepted reads in two groups, each ascending, with their counts: [0] rows without ADP_ROW_POLYA_TRUNCATED,
//                  [1] rows with it; reval = (-1, 0) for every read of the call
//   k_afr_gather   per-subset arrays of a group's validation: full_len, the bounds the first validation took, read back from the
//                  row (the primary adapter end and cand[0 .. n_cand), zero padded to ADP_MAX_CAND; n_cand == -1: the list is None,
//                  the primary's poly(A) end alone), polya_end_topk given or None, starts = a0 + s.  The truncated group is
//                  validated as T2 validated it: (primary adapter end, the row's polya_end), k = 1
//   k_afr_merge    passing rows to their reads' positions, and every selected read's verdict into reval
//   k_afr_info     info[r][3] = 1 only where the row was replaced
#pragma once
#include <cstddef>

#include "common.h"
#include "validate.h"

// info: k_adapter_front's [n, 4] (column 3: accepted)
__global__ void __launch_bounds__(SEL_THREADS) k_afr_select(const int32_t *__restrict__ info, const adp_row *__restrict__ rows, int n,
                                                            int32_t *__restrict__ sel_a, int32_t *__restrict__ sel_b,
                                                            unsigned int *__restrict__ counts, int32_t *__restrict__ reval)
{
    int total_a = 0, total_b = 0;
    for (int r0 = 0; r0 < n; r0 += SEL_THREADS) {
        const int r = r0 + threadIdx.x;
        const bool acc = r < n && info[(size_t)r * 4 + 3] == 1;
        const bool trunc = acc && (rows[r].reserved_ & ADP_ROW_POLYA_TRUNCATED) != 0;
        if (r < n) { reval[2 * (size_t)r] = -1; reval[2 * (size_t)r + 1] = 0; }
        sel_step(acc && !trunc, r, sel_a, total_a);
        sel_step(trunc, r, sel_b, total_b);
    }
    if (threadIdx.x == 0) { counts[0] = (unsigned int)total_a; counts[1] = (unsigned int)total_b; }
}

// bounds [n_sel, 1 + kmax]: kmax = ADP_MAX_CAND, or 1 for the truncated group
__global__ void __launch_bounds__(256) k_afr_gather(const int32_t *__restrict__ sel, int n_sel, int kmax, int truncated,
                                                    const int32_t *__restrict__ full_len, const adp_row *__restrict__ rows,
                                                    const int64_t *__restrict__ shift, int32_t *__restrict__ len_sub,
                                                    int64_t *__restrict__ bounds, int8_t *__restrict__ topk_sub, int64_t *__restrict__ starts)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_sel) return;
    const int r = sel[j];
    const adp_row *row = rows + r;
    len_sub[j] = full_len[r];
    int64_t *bd = bounds + (size_t)j * (1 + kmax);
    bd[0] = (int64_t)row->col[ADP_C_PRIMARY_ADAPTER_END];
    const int nc = row->n_cand;
    int8_t none = 0;
    if (truncated) bd[1] = (int64_t)row->col[ADP_C_POLYA_END];
    else if (nc < 0) {
        none = 1;
        bd[1] = (row->present >> ADP_C_PRIMARY_POLYA_END & 1) ? (int64_t)row->col[ADP_C_PRIMARY_POLYA_END] : 0;
        for (int c = 1; c < kmax; c++) bd[1 + c] = 0;
    } else
        for (int c = 0; c < kmax; c++) bd[1 + c] = (c < nc && c < ADP_MAX_CAND) ? row->cand[c] : 0;
    topk_sub[j] = none;
    const int64_t a0 = (row->present >> ADP_C_ADAPTER_START & 1) ? (int64_t)row->col[ADP_C_ADAPTER_START] : 0;
    starts[j] = a0 + shift[r];
}

// one wave per selected read.  Carried over from the read's row, as k_pt_merge carries them: the primary's poly(A) end,
// polya_candidates, the five start-peak columns (each with its present bit), start_peak_type and reserved_ bits 0-2; bits 3 and 4 set
__global__ void __launch_bounds__(64) k_afr_merge(const int32_t *__restrict__ sel, int n_sel, const adp_row *__restrict__ rows2,
                                                  adp_row *__restrict__ rows, int32_t *__restrict__ reval)
{
    const int j = blockIdx.x, ln = lane_id();
    if (j >= n_sel) return;
    const int r = sel[j];
    const int ok = rows2[j].success == 1;
    if (ln == 0) { reval[2 * (size_t)r] = ok; reval[2 * (size_t)r + 1] = ok ? 0 : rows2[j].fail_code; }
    if (!ok) return;
    adp_row *dst_row = rows + r;
    constexpr int NW = (int)(sizeof(adp_row) / 4), COL = (int)(offsetof(adp_row, col) / 4);
    constexpr int W_PPE = COL + 2 * ADP_C_PRIMARY_POLYA_END, W_SP0 = COL + 2 * ADP_C_SP_IDX, W_SP1 = COL + 2 * (ADP_C_SP_OPEN_PORE_IDX + 1);
    constexpr int W_PRESENT = (int)(offsetof(adp_row, present) / 4), W_SPT = (int)(offsetof(adp_row, start_peak_type) / 4);
    constexpr int W_NCAND = (int)(offsetof(adp_row, n_cand) / 4), W_CAND = (int)(offsetof(adp_row, cand) / 4);
    constexpr int W_RES = (int)(offsetof(adp_row, reserved_) / 4);
    constexpr unsigned long long KEEP = (1ull << ADP_C_PRIMARY_POLYA_END) | (31ull << ADP_C_SP_IDX);
    static_assert(ADP_C_SP_OPEN_PORE_IDX == ADP_C_SP_IDX + 4, "the start-peak columns are consecutive");
    const unsigned long long present = (rows2[j].present & ~KEEP) | (dst_row->present & KEEP);
    const int32_t reserved = (dst_row->reserved_ & (ADP_ROW_FROM_SECOND_LLR | ADP_ROW_POLYA_TRUNCATED | ADP_ROW_TRUNC_LOOKED)) |
                             ADP_ROW_ADAPTER_FRONT | ADP_ROW_REVALIDATED;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows2 + j);
    uint32_t *dst = reinterpret_cast<uint32_t *>(dst_row);
    for (int i = ln; i < NW; i += 64) {
        const bool keep = (i >= W_PPE && i < W_PPE + 2) || (i >= W_SP0 && i < W_SP1) || i == W_SPT || i == W_NCAND ||
                          (i >= W_CAND && i < W_CAND + 2 * ADP_MAX_CAND) || i == W_PRESENT || i == W_PRESENT + 1 || i == W_RES;
        if (!keep) dst[i] = src[i];
    }
    if (ln == 0) { dst_row->present = present; dst_row->reserved_ = reserved; }
}

__global__ void __launch_bounds__(256) k_afr_info(int32_t *__restrict__ info, const int32_t *__restrict__ reval, int n)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) info[(size_t)r * 4 + 3] = reval[2 * (size_t)r] == 1 ? 1 : 0;
}
