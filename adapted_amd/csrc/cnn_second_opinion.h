// cnn_second_opinion.h -- the device side of ADP_CNN_SECOND_LLR: reads whose row failed on the CNN path (first pass, plus the short-
// read fallback where it ran) get the row combined_detect_llr2 returns for them on the same minibatch, if that row passes.
//
// The LLR primary is the LLR path's own (launch_n1 ... k_polya_peak, k_llr_bounds) over ALL reads of the call, so that the N1
// scalars and the status of every minibatch are those of the whole minibatch; the validation runs over the failed reads only,
// on the rows where they lie (SigIdx, common.h).  New here:
//   k_cnn_so_select   the reads with success == 0 (exception rows included), ascending, and their count -- the host reads it
//                     with the call's arena counter and launches nothing more when it is 0
//   k_cnn_so_gather   per-subset arrays of the validation: full_len, the LLR bounds and polya_end_topk's None-ness of every
//                     selected read; a read of a dropped minibatch (status != ADP_MB_OK) gets (0, 0): it leaves the validation at
//                     its first test and writes nothing to the open-pore arena
//   k_cnn_so_merge    rows that passed to their reads' positions in the call's row buffer, marked (adp_row.reserved_ bit 0), and
//                     the call's counts
#pragma once
#include <cstddef>

#include "common.h"

// One workgroup walks the reads SEL_THREADS at a time (sel_step, common.h): ascending read order.
__global__ void __launch_bounds__(SEL_THREADS) k_cnn_so_select(const adp_row *__restrict__ rows, int n, int32_t *__restrict__ sel,
                                                               unsigned int *__restrict__ count_out)
{
    int total = 0;
    for (int r0 = 0; r0 < n; r0 += SEL_THREADS) {
        const int r = r0 + threadIdx.x;
        sel_step(r < n && rows[r].success == 0, r, sel, total);
    }
    if (threadIdx.x == 0) *count_out = (unsigned int)total;
}

// bounds_all int64 [n, 2] / topk_all [n]: what k_llr_bounds left for every read of the call; mbs: the minibatches' N1 state
__global__ void __launch_bounds__(256) k_cnn_so_gather(const int32_t *__restrict__ sel, int n_sel, int mbsize, const MbState *__restrict__ mbs,
                                                       const int32_t *__restrict__ full_len, const int64_t *__restrict__ bounds_all,
                                                       const int8_t *__restrict__ topk_all, int32_t *__restrict__ len_sub,
                                                       int64_t *__restrict__ bounds2, int8_t *__restrict__ topk_sub)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_sel) return;
    const int r = sel[j];
    const bool ok = mbs[r / mbsize].status == ADP_MB_OK;
    len_sub[j] = full_len[r];
    bounds2[2 * j] = ok ? bounds_all[2 * (size_t)r] : 0;
    bounds2[2 * j + 1] = ok ? bounds_all[2 * (size_t)r + 1] : 0;
    topk_sub[j] = ok ? topk_all[r] : (int8_t)0;
}

// one wave per selected read.  counts (adp_debug_fetch what = 11): [0] rows replaced, [1] rows re-validated and still failing,
// [2] minibatches that hold a selected read and gave no second opinion (sel is ascending: the first selected read of a minibatch
// counts it)
__global__ void __launch_bounds__(64) k_cnn_so_merge(const int32_t *__restrict__ sel, int n_sel, int mbsize, const MbState *__restrict__ mbs,
                                                     const adp_row *__restrict__ rows2, adp_row *__restrict__ rows, unsigned int *__restrict__ counts)
{
    const int j = blockIdx.x, ln = lane_id();
    if (j >= n_sel) return;
    const int r = sel[j], mb = r / mbsize;
    if (mbs[mb].status != ADP_MB_OK) {
        if (ln == 0 && (j == 0 || sel[j - 1] / mbsize != mb)) atomicAdd(counts + 2, 1u);
        return;
    }
    if (rows2[j].success != 1) { if (ln == 0) atomicAdd(counts + 1, 1u); return; }
    constexpr int W = (int)(sizeof(adp_row) / 4), SRC = (int)(offsetof(adp_row, reserved_) / 4);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows2 + j);
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows + r);
    for (int i = ln; i < W; i += 64) dst[i] = i == SRC ? (src[i] | 1u) : src[i];
    if (ln == 0) atomicAdd(counts, 1u);
}
