// cnn_fallback.h -- the device side of combined_detect_cnn's short-read fallback (the reference's "hail mary",
// adapted/detect/combined.py:251-301) inside adp_detect_cnn (ADP_CNN_FALLBACK).
//
// The first pass (prepare -> conv stack -> predict -> validate) leaves one row and one prediction per read.  Then
//   k_cnn_fb_select   which reads take the fallback (combined.py:251-257), their indices compacted in ascending order, and the
//                     count -- the host reads it with the call's arena counter and launches nothing more when it is 0
//   k_cnn_fb_gather   per-subset arrays of the chain: full_len and the range [cnn_adapter_end, cnn_polya_end) of every selected
//                     read; later the bounds (adapter_end, new polya_end) of the re-validation
//   (the chain of adp_llr_refine_polya and the validation kernels read the selected rows IN PLACE through SigIdx, common.h:
//    nothing here is sized by the window m)
//   k_cnn_fb_merge    exception rows and re-validated rows to their reads' positions in the call's row buffer
#pragma once
#include "common.h"

// One workgroup walks the reads SEL_THREADS at a time (sel_step, common.h): the list comes out in ascending read order.
// bounds: int64 [n, bstride], adapter end and first poly(A) candidate in front.  limit = 2 * max_obs_adapter.
__global__ void __launch_bounds__(SEL_THREADS) k_cnn_fb_select(const adp_row *__restrict__ rows, const int64_t *__restrict__ bounds, int bstride,
                                                               const int32_t *__restrict__ full_len, int n, long long limit,
                                                               int32_t *__restrict__ sel, unsigned int *__restrict__ count_out)
{
    int total = 0;
    for (int r0 = 0; r0 < n; r0 += SEL_THREADS) {
        const int r = r0 + threadIdx.x;
        bool take = false;
        if (r < n) {
            const int fc = rows[r].fail_code;
            const long long ae = bounds[(size_t)r * bstride], pe = bounds[(size_t)r * bstride + 1];
            take = rows[r].success == 0 && !ADP_F_IS_EXCEPTION(fc) && ae > 0 && pe > 0 && pe - ae > 1000 && (long long)full_len[r] < limit;
        }
        sel_step(take, r, sel, total);
    }
    if (threadIdx.x == 0) *count_out = (unsigned int)total;
}

// phase 0 (before the chain): len_sub[j] = full_len[sel[j]], ranges[j] = (adapter end, poly(A) end) of the first pass.
// phase 1 (behind it): bounds2[j] = (adapter end, new poly(A) end) where the chain found one, (0, 0) otherwise -- such a read
// leaves the validation at its first test, writes nothing to the open-pore arena, and its row is not merged.
__global__ void __launch_bounds__(256) k_cnn_fb_gather(const int32_t *__restrict__ sel, int n_sel, int phase, const int64_t *__restrict__ bounds, int bstride,
                                                       const int32_t *__restrict__ full_len, int32_t *__restrict__ len_sub, int64_t *__restrict__ ranges,
                                                       const int64_t *__restrict__ new_pe, const int32_t *__restrict__ status, int64_t *__restrict__ bounds2)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_sel) return;
    if (phase == 0) {
        const int r = sel[j];
        len_sub[j] = full_len[r];
        ranges[2 * j] = bounds[(size_t)r * bstride];
        ranges[2 * j + 1] = bounds[(size_t)r * bstride + 1];
    } else {
        const bool redo = status[j] == 0 && new_pe[j] > 0;
        bounds2[2 * j] = redo ? ranges[2 * j] : 0;
        bounds2[2 * j + 1] = redo ? new_pe[j] : 0;
    }
}

// one wave per selected read.  counts: [0] exception rows made, [1] rows re-validated (adp_debug_fetch what = 10)
__global__ void __launch_bounds__(64) k_cnn_fb_merge(const int32_t *__restrict__ sel, int n_sel, const int64_t *__restrict__ new_pe,
                                                     const int32_t *__restrict__ status, const adp_row *__restrict__ rows2,
                                                     adp_row *__restrict__ rows, unsigned int *__restrict__ counts)
{
    const int j = blockIdx.x, ln = lane_id();
    if (j >= n_sel) return;
    const int st = status[j];
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows + sel[j]);
    constexpr int W = (int)(sizeof(adp_row) / 4);
    if (st != 0) { // the reference raised inside its per-read try block: the all-None row
        adp_row *row = rows + sel[j];
        for (int i = ln; i < W; i += 64) dst[i] = 0;
        __syncthreads();
        if (ln == 0) { row->n_cand = -1; row->n_open_pores = -1; row->open_pores_more = -1; row->fail_code = st; atomicAdd(counts, 1u); }
    } else if (new_pe[j] > 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(rows2 + j);
        for (int i = ln; i < W; i += 64) dst[i] = src[i];
        if (ln == 0) atomicAdd(counts + 1, 1u);
    }
}
