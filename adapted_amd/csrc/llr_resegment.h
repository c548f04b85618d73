// llr_resegment.h -- the device side of ADP_LLR_RESEGMENT (include/adapted_hip_resegment.h): behind the first validation of an
// adp_detect_llr call, every read the LLR primary failed behind a first change point is segmented once more from its "poly(A) end".
//
// THE RULE (with ds = cfg.downscale_factor, off = cfg.min_obs_adapter, a1 / p1 = the row's primary adapter / poly(A) end):
//   eligible   the read's minibatch is ADP_MB_OK; the row has success == 0, is no exception row, holds a1 > 0 and holds p1 > a1
//   segment    c = (p1 - off) / ds (exact); the trace of calc_adapter_trace(s_, offset_head = 1, offset_tail = 1, trace_start = c)
//              on the read's pooled signal s_, normalised with its OWN minibatch's median and MAD, and on s_'s sequential float64
//              cumulative sums; p = detect_full_polya_trace_peak_with_spike(trace); p2 = p > 0 ? p * ds + off : 0
//   validate   p2 == 0: nothing more.  Else validate_boundaries with Boundaries(adapter_start = a1, adapter_end = p1, polya_end = p2,
//              polya_end_topk = [p2]) -- launch_validate_t<true> over the rows where they lie (SigIdx), as afr_group calls it
//   merge      a validation with success == 1 replaces the read's row; the five start-peak columns (with their present bits) and
//              start_peak_type stay the first row's; reserved_ = ADP_ROW_RESEGMENTED | first fail_code << ADP_ROW_FIRST_FAIL_SHIFT
//              (bits 6-9).  A validation that fails leaves the first row byte for byte.  One level only.
//
// The trace phase of the selected reads is computed AGAIN, over the subset, by the first pass's own kernels in the first pass's
// instantiations -- k_norm_pool<SigIdx> (numpy's 8-accumulator pooling), k_cumsum / k_cumsum_gather (the sequential float64 sums),
// k_gains<2> + k_polya_peak, windowed with their whole-trace redo -- so the bits are the first pass's whatever became of its
// workspace: a grouped call (ADP_GROUPS, ADP_LANES) recycles a group's, and the rows must not depend on the grouping.  Those
// kernels find a read's normalisation at mbs[r / mbsize]; the subset runs them with mbsize = 1 over a gathered array that holds, for
// every selected read, a copy of its own minibatch's MbState (k_rs_gather: the per-read indirection into the call's states).
//
// New here:
//   k_rs_select  the eligible reads, ascending (sel_step), their count where the host reads it with the call's arena counter -- it
//                launches nothing more when that is 0 -- and counts[0]
//   k_rs_gather  per-subset arrays: full_len, starts = a1, bounds = (p1, .), the pass-2 start c, the read's minibatch state
//   k_rs_bounds  p2 from the second segmentation's poly(A) index into the bounds; counts[1]: reads with p2 > 0
//   k_rs_merge   passing rows to their reads' positions in the call's row buffer; counts[2]: rows replaced
// counts (adp_debug_fetch what = 25; zeroed by the host): [0] eligible reads, [1] reads with p2 > 0, [2] rows replaced
#pragma once
#include <cstddef>

#include "common.h"
#include "validate.h"

static __device__ __forceinline__ bool rs_eligible(const adp_row *row, int mb_status)
{
    const unsigned long long present = row->present;
    const int fc = row->fail_code;
    // (a row of a dropped minibatch is all zero: nothing present; the status says so first)
    if (mb_status != ADP_MB_OK || row->success != 0 || ADP_F_IS_EXCEPTION(fc)) return false;
    if (!(present >> ADP_C_PRIMARY_ADAPTER_END & 1) || !(present >> ADP_C_PRIMARY_POLYA_END & 1)) return false;
    const long long a1 = (long long)row->col[ADP_C_PRIMARY_ADAPTER_END], p1 = (long long)row->col[ADP_C_PRIMARY_POLYA_END];
    return a1 > 0 && p1 > a1;
}

// One workgroup walks the rows SEL_THREADS at a time (sel_step, common.h): ascending read order.  mbs: the CALL's minibatch states
__global__ void __launch_bounds__(SEL_THREADS) k_rs_select(const adp_row *__restrict__ rows, int n, int mbsize, const MbState *__restrict__ mbs,
                                                           int32_t *__restrict__ sel, unsigned int *__restrict__ count_out,
                                                           unsigned int *__restrict__ counts)
{
    int total = 0;
    for (int r0 = 0; r0 < n; r0 += SEL_THREADS) {
        const int r = r0 + threadIdx.x;
        sel_step(r < n && rs_eligible(rows + r, mbs[r / mbsize].status), r, sel, total);
    }
    if (threadIdx.x == 0) { *count_out = (unsigned int)total; counts[0] = (unsigned int)total; }
}

// What the second segmentation of one selected read starts from, position j of the subset's arrays.  row: the failing row that holds
// a1 and p1 (k_rs_gather: the call's row of the read; k_csr_gather, cnn_second_resegment.h: the second opinion's); mb: the state of the
// read's own minibatch.  bounds2 [n_sel, 2]: (p1, 0 until k_rs_bounds); start_sub: pass 2's trace_start in pooled points; mbs_sub
// [n_sel]: for kernels that take mbs[r / 1]
static __device__ __forceinline__ void rs_gather_read(int j, const adp_row *row, int32_t len, const MbState &mb, int ds, int off,
                                                      int32_t *__restrict__ len_sub, int64_t *__restrict__ starts, int64_t *__restrict__ bounds2,
                                                      int8_t *__restrict__ topk_sub, int32_t *__restrict__ start_sub, MbState *__restrict__ mbs_sub)
{
    const int64_t a1 = (int64_t)row->col[ADP_C_PRIMARY_ADAPTER_END], p1 = (int64_t)row->col[ADP_C_PRIMARY_POLYA_END];
    len_sub[j] = len;
    starts[j] = a1;
    bounds2[2 * j] = p1;
    bounds2[2 * j + 1] = 0;
    topk_sub[j] = 1;
    start_sub[j] = (int32_t)((p1 - off) / ds);
    mbs_sub[j] = mb;
}

__global__ void __launch_bounds__(256) k_rs_gather(const int32_t *__restrict__ sel, int n_sel, int mbsize, const MbState *__restrict__ mbs,
                                                   const int32_t *__restrict__ full_len, const adp_row *__restrict__ rows, int ds, int off,
                                                   int32_t *__restrict__ len_sub, int64_t *__restrict__ starts, int64_t *__restrict__ bounds2,
                                                   int8_t *__restrict__ topk_sub, int32_t *__restrict__ start_sub, MbState *__restrict__ mbs_sub)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_sel) return;
    const int r = sel[j];
    rs_gather_read(j, rows + r, full_len[r], mbs[r / mbsize], ds, off, len_sub, starts, bounds2, topk_sub, start_sub, mbs_sub);
}

// as k_llr_bounds makes a poly(A) end from a pooled index (validate.h): p > 0 -> p * ds + off, and polya_end_topk is given then
__global__ void __launch_bounds__(256) k_rs_bounds(const int32_t *__restrict__ polya_idx, int n_sel, int ds, int off, int64_t *__restrict__ bounds2,
                                                   int8_t *__restrict__ topk_sub, unsigned int *__restrict__ counts)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int p = j < n_sel ? polya_idx[j] : 0;
    if (j < n_sel) {
        bounds2[2 * j + 1] = p > 0 ? (int64_t)p * ds + off : 0;
        topk_sub[j] = p > 0 ? 0 : 1;
    }
    const int found = __popcll(__ballot(p > 0));
    if (lane_id() == 0 && found) atomicAdd(counts + 1, (unsigned int)found);
}

// one wave per selected read.  A read without p2 was validated as the read without a poly(A) end it is: its row fails and stays
// where it is.  Carried over from the first row: the five start-peak columns (each with its present bit) and start_peak_type
__global__ void __launch_bounds__(64) k_rs_merge(const int32_t *__restrict__ sel, int n_sel, const adp_row *__restrict__ rows2, adp_row *__restrict__ rows,
                                                 unsigned int *__restrict__ counts)
{
    const int j = blockIdx.x, ln = lane_id();
    if (j >= n_sel) return;
    if (rows2[j].success != 1) return;
    adp_row *dst_row = rows + sel[j];
    constexpr int NW = (int)(sizeof(adp_row) / 4), COL = (int)(offsetof(adp_row, col) / 4);
    constexpr int W_SP0 = COL + 2 * ADP_C_SP_IDX, W_SP1 = COL + 2 * (ADP_C_SP_OPEN_PORE_IDX + 1);
    constexpr int W_PRESENT = (int)(offsetof(adp_row, present) / 4), W_SPT = (int)(offsetof(adp_row, start_peak_type) / 4);
    constexpr int W_RES = (int)(offsetof(adp_row, reserved_) / 4);
    constexpr unsigned long long KEEP = 31ull << ADP_C_SP_IDX;
    static_assert(ADP_C_SP_OPEN_PORE_IDX == ADP_C_SP_IDX + 4, "the start-peak columns are consecutive");
    static_assert(ADP_F_NO_ADAPTER_MVS <= 15 && (ADP_ROW_FIRST_FAIL_MASK >> ADP_ROW_FIRST_FAIL_SHIFT) == 15, "a fail code fits its four bits");
    const unsigned long long present = (rows2[j].present & ~KEEP) | (dst_row->present & KEEP);
    const int32_t reserved = ADP_ROW_RESEGMENTED | ((dst_row->fail_code << ADP_ROW_FIRST_FAIL_SHIFT) & ADP_ROW_FIRST_FAIL_MASK);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rows2 + j);
    uint32_t *dst = reinterpret_cast<uint32_t *>(dst_row);
    for (int i = ln; i < NW; i += 64) {
        const bool keep = (i >= W_SP0 && i < W_SP1) || i == W_SPT || i == W_PRESENT || i == W_PRESENT + 1 || i == W_RES;
        if (!keep) dst[i] = src[i];
    }
    if (ln == 0) { dst_row->present = present; dst_row->reserved_ = reserved; atomicAdd(counts + 2, 1u); }
}
