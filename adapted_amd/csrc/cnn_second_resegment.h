// cnn_second_resegment.h -- the device side of ADP_CNN_SECOND_RESEGMENT (include/adapted_hip_second_resegment.h): behind the LLR second
// opinion of an adp_detect_cnn(_i16) call, every selected read whose SECOND row failed behind a first change point is segmented once
// more from that row's "poly(A) end" -- the re-segmentation of llr_resegment.h with "the first row" read as the second opinion's.
//
// The second opinion (cnn_second_opinion.h) leaves, for the n_so reads so_sel lists, the rows of its own validation in rows2[j] (j the
// position in the subset) and merges those that passed into the call's rows.  The rows that failed are what this phase reads; the
// eligibility test is rs_eligible, on rows2[j] and the status of the read's minibatch.  The trace phase and the validation between
// the gather and the merge are the LLR re-segmentation's (reseg_trace_validate, adapted_hip.hip).  New here:
//   k_csr_select  over the second opinion's subset, ascending (sel_step): the eligible reads' positions in the subset and their indices
//                 into the call's reads, their count where the host reads it with the call's arena counter -- it launches nothing more
//                 when that is 0 -- and counts[0]
//   k_csr_gather  per-subset arrays from rows2[j]: full_len, starts = a1, bounds = (p1, .), the pass-2 start c, the read's minibatch state
//   k_csr_merge   passing rows to their reads' positions in the call's row buffer, whole (nothing of the CNN path's row stays: the
//                 start-peak overlay follows on the host's side), with reserved_ = ADP_ROW_FROM_SECOND_LLR | ADP_ROW_RESEGMENTED |
//                 the second opinion's fail_code << ADP_ROW_FIRST_FAIL_SHIFT; counts[2]: rows replaced
// counts (adp_debug_fetch what = 26; zeroed by the host): [0] eligible reads, [1] reads with p2 > 0 (k_rs_bounds), [2] rows replaced
#pragma once
#include <cstddef>

#include "common.h"
#include "llr_resegment.h"

// One workgroup walks the subset SEL_THREADS positions at a time (sel_step, common.h): both lists come out in ascending order.
// so_sel [n_so]: the second opinion's reads; rows2 [n_so]: its rows; mbs: the minibatch states of its LLR run over the whole call
__global__ void __launch_bounds__(SEL_THREADS) k_csr_select(const int32_t *__restrict__ so_sel, int n_so, int mbsize, const MbState *__restrict__ mbs,
                                                            const adp_row *__restrict__ rows2, int32_t *__restrict__ sel_j, int32_t *__restrict__ sel_r,
                                                            unsigned int *__restrict__ count_out, unsigned int *__restrict__ counts)
{
    int total_j = 0, total_r = 0;
    for (int j0 = 0; j0 < n_so; j0 += SEL_THREADS) {
        const int j = j0 + threadIdx.x;
        const int r = j < n_so ? so_sel[j] : 0;
        const bool take = j < n_so && rs_eligible(rows2 + j, mbs[r / mbsize].status);
        sel_step(take, j, sel_j, total_j);
        sel_step(take, r, sel_r, total_r);
    }
    if (threadIdx.x == 0) { *count_out = (unsigned int)total_r; counts[0] = (unsigned int)total_r; }
}

__global__ void __launch_bounds__(256) k_csr_gather(const int32_t *__restrict__ sel_j, const int32_t *__restrict__ sel_r, int n_sel, int mbsize,
                                                    const MbState *__restrict__ mbs, const int32_t *__restrict__ full_len,
                                                    const adp_row *__restrict__ rows2, int ds, int off, int32_t *__restrict__ len_sub,
                                                    int64_t *__restrict__ starts, int64_t *__restrict__ bounds2, int8_t *__restrict__ topk_sub,
                                                    int32_t *__restrict__ start_sub, MbState *__restrict__ mbs_sub)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sel) return;
    const int r = sel_r[i];
    rs_gather_read(i, rows2 + sel_j[i], full_len[r], mbs[r / mbsize], ds, off, len_sub, starts, bounds2, topk_sub, start_sub, mbs_sub);
}

// one wave per selected read.  rows3 [n_sel]: the rows of the second segmentation's validation; rows2: the second opinion's (the code
// of the failure this row follows); rows: the call's.  A read without p2 was validated as the read without a poly(A) end it is: its
// row fails and the CNN path's stays where it is.
__global__ void __launch_bounds__(64) k_csr_merge(const int32_t *__restrict__ sel_j, const int32_t *__restrict__ sel_r, int n_sel,
                                                  const adp_row *__restrict__ rows3, const adp_row *__restrict__ rows2, adp_row *__restrict__ rows,
                                                  unsigned int *__restrict__ counts)
{
    const int i = blockIdx.x, ln = lane_id();
    if (i >= n_sel) return;
    if (rows3[i].success != 1) return;
    constexpr int NW = (int)(sizeof(adp_row) / 4), W_RES = (int)(offsetof(adp_row, reserved_) / 4);
    const uint32_t reserved = (uint32_t)(ADP_ROW_FROM_SECOND_LLR | ADP_ROW_RESEGMENTED |
                                         ((rows2[sel_j[i]].fail_code << ADP_ROW_FIRST_FAIL_SHIFT) & ADP_ROW_FIRST_FAIL_MASK));
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows3 + i);
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows + sel_r[i]);
    for (int w = ln; w < NW; w += 64) dst[w] = w == W_RES ? reserved : src[w];
    if (ln == 0) atomicAdd(counts + 2, 1u);
}
