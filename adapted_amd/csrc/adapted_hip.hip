// adapted_hip.hip -- libadapted_hip.so: C ABI (include/adapted_hip.h) over the gfx950 kernels.
// The detect path's translation unit: its kernels live in the headers next to this file.  The reference-module drop-ins
// (adp_c_llr_*, adp_llr_*, adp_mvs_*) are compiled apart, in modules.hip; handle.h is what the two share.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "adapted_hip.h"
#include "handle.h"
#include "common.h"
__device__ unsigned long long g_dbg[ADP_NDBG] = {0};
// k_partition_stats' tallies (slots 0-4 of what = 8), spread over ADP_NTALLY cache lines by workgroup: every workgroup adding to ONE
// address serialises device-wide -- 2 x 96 000 same-address atomics were 7.7 ms of the kernel's 13 at the default window
__device__ unsigned long long g_bs_tally[ADP_NTALLY][8] = {{0}};
#include "llr_stream.h"
#include "n1_select.h"
#include "n1_fused.h"
#include "peaks.h"
#include "synth.h"
#include "validate.h"
#include "cand_stats2.h"
#include "series_pipe.h"
#include "cnn_topk.h"
#include "cnn_conv.h"
#include "cnn_conv_split.h"
#include "cnn_fallback.h"
#include "cnn_second_opinion.h"
#include "polya_truncated.h"
#include "adapter_front_revalidate.h"
#include "llr_resegment.h"
#include "cnn_second_resegment.h"
#include "wave_stats.h"

thread_local std::string g_err;

static int env_int(const char *name, int dflt);

static int geom(adp_handle *h)
{
    const adp_cfg &c = h->cfg;
    if (c.downscale_factor < 1 || c.downscale_factor > 32 || c.sp_downscale_factor < 1 || c.sp_downscale_factor > 64) {
        g_err = "downscale_factor must be in [1, 32]"; return ADP_ERR_UNSUPPORTED;
    }
    if (c.mvs_detect_overwrite && c.mvs_detect_check) {
        // mvs.py:264-266 reads the series at 2 * offset when nothing is found: an IndexError in the reference otherwise
        const int off = c.pA_mean_window > c.pA_var_window ? c.pA_mean_window : c.pA_var_window;
        if (c.search_window <= off || c.search_window < 1) { g_err = "mvs_detect_overwrite needs search_window > max(pA_mean_window, pA_var_window)"; return ADP_ERR_UNSUPPORTED; }
    }
    if (c.polya_cand_k > ADP_MAX_CAND - 1) { g_err = "polya_cand_k too large"; return ADP_ERR_UNSUPPORTED; }
    if (h->m > BS_MAXCHUNK * 8192) { g_err = "preload longer than 1 Mi samples: k_partition_stats keeps one chunk sum per 8192 samples in LDS"; return ADP_ERR_UNSUPPORTED; }
    if ((c.max_obs_trace - c.min_obs_adapter) / c.downscale_factor > 400000) { g_err = "max_obs_trace too large for the LDS state of k_polya_peak"; return ADP_ERR_UNSUPPORTED; }
    h->T = c.max_obs_trace < h->m ? c.max_obs_trace : h->m;
    h->off = c.min_obs_adapter;
    h->ds = c.downscale_factor;
    h->oh1 = 5; h->pos_off = h->off;
    if (h->layout == ADP_LAYOUT_SINGLE_READ) { // combined_detect_llr: no min_obs_adapter slice, a longer head offset instead,
        h->off = 0;                             // and min_obs_adapter still added to the positions (combined.py:66-68, 93-95)
        h->oh1 = 5 + c.min_obs_adapter / c.downscale_factor;
        h->pos_off = c.min_obs_adapter;
    }
    int Lseg = h->T - h->off;
    h->L = Lseg > 0 ? (Lseg + h->ds - 1) / h->ds : 0;
    h->Lp = ((h->L + 63) / 64) * 64;
    if (h->Lp == 0) h->Lp = 64;
    h->nck = h->Lp / CK;
    h->nsum = h->Lp / SUMBLK;
    return 0;
}

// Workspace for a call over `reads` reads (grow-only; allocated by the call that needs it, not by adp_create: a grouped LLR
// call keeps its big buffers in the lanes, sized for one group).  llr: the pooled signal / trace / peak-list buffers too.
static int alloc_all(adp_handle *h, int reads, bool llr)
{
    const size_t R = (size_t)(reads < 1 ? 1 : reads), Lp = (size_t)h->Lp;
    int bad = 0;
    if (llr) {
    bad |= h->down.ensure(R * Lp * 4);
    bad |= h->gstat.ensure(R * 24);
    bad |= h->ck.ensure(R * h->nck * sizeof(double2));
    bad |= h->tail.ensure(R * sizeof(double2));
    bad |= h->trace.ensure(R * Lp * 8);
    bad |= h->bmax.ensure(R * h->nsum * 8);
    bad |= h->bmin.ensure(R * h->nsum * 8);
    bad |= h->t1.ensure(R * sizeof(int2));
    }
    bad |= h->nvalid.ensure(R * 4);
    bad |= h->adapter_idx.ensure(R * 4);
    bad |= h->polya_idx.ensure(R * 4);
    bad |= h->bounds.ensure(R * (1 + ADP_MAX_CAND) * 8);
    bad |= h->topk_none.ensure(R);
    bad |= h->rows.ensure(R * sizeof(adp_row));
    bad |= h->preq.ensure(R * sizeof(PartReq));
    bad |= h->series.ensure(R * 2 * MVS_CAP * 4);
    bad |= h->have_series.ensure(R);
    bad |= h->sp.ensure(R * sizeof(SpOut));
    bad |= h->any_none.ensure(64);
    h->vstride = ((h->m + 63) / 64) * 64;
    // k_validate: 6 waves per SIMD = 6144 resident waves; each slot owns two series of up to m floats (moving mean and
    // variance of slices k_mvs_series did not prepare): the slot count is bounded so that this scratch stays below 10 GB
    {
        size_t cap = (size_t)10000000000ull / ((size_t)8 * h->vstride);
        if (cap < 256) cap = 256;
        size_t want = R < 1024 * VAL_WPE ? R : 1024 * VAL_WPE;
        h->vslots = (int)(want < cap ? want : cap);
    }
    bad |= h->vscratch.ensure((size_t)h->vslots * 2 * h->vstride * 4);
    h->pslots = (int)(R < 8192 ? R : 8192);
    if (llr) {
    bad |= h->pk.ensure(R * (Lp / 2 + 1) * 4);   // per-read peak lists (k_gains -> k_polya_peak)
    if (env_int("ADP_PK_VALUES", 1)) bad |= h->pkv.ensure(R * (Lp / 2 + 1) * 8);  // ... and the maxima's heights (twice the list's size: only when they are used)
    bad |= h->npk.ensure(R * 4);
    bad |= h->wend.ensure(R * 4);          // how far pass 2 computed each read's trace (k_gains<2> -> k_polya_peak)
    bad |= h->redo.ensure((R + 1) * 4);    // the windowed pass 2's redo list: count, then reads
    bad |= h->mk.ensure((size_t)h->pslots * (Lp / 2 + 1) * 4);
    }
    ALLOCCHK(bad);
    return 0;
}

// grid = (ceil(m / 1024), n); block = 256.  Read r's samples lie at packed[offs[r] .. offs[r] + min(full_len, m)).
template <class SRC>
__global__ void __launch_bounds__(256) k_expand_ragged(const SRC *__restrict__ packed, const int64_t *__restrict__ offs,
                                                        const int32_t *__restrict__ full_len, const float *__restrict__ scale,
                                                        const float *__restrict__ offset, int m, float *__restrict__ out)
{
    const int r = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= m) return;
    const int len = full_len[r] < m ? (full_len[r] > 0 ? full_len[r] : 0) : m;
    const SRC *src = packed + offs[r] + i0;
    float *dst = out + (size_t)r * m + i0;
    const float nanv = __builtin_nanf("");
    float sc = 1.f, of = 0.f;
    if (scale) { sc = scale[r]; of = offset[r]; }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (i0 + j >= m) break;
        float v = nanv;
        if (i0 + j < len) v = scale ? sc * ((float)src[j] + of) : (float)src[j];
        dst[j] = v;
    }
}

// the same for raw samples that STAY raw (adp_detect_llr_i16 reads them): int16 [n, m], zeros behind each read
__global__ void __launch_bounds__(256) k_expand_ragged_raw(const int16_t *__restrict__ packed, const int64_t *__restrict__ offs,
                                                           const int32_t *__restrict__ full_len, int m, int16_t *__restrict__ out)
{
    const int r = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= m) return;
    const int len = full_len[r] < m ? (full_len[r] > 0 ? full_len[r] : 0) : m;
    const int16_t *src = packed + offs[r] + i0;
    int16_t *dst = out + (size_t)r * m + i0;
#pragma unroll
    for (int j = 0; j < 4; j++) if (i0 + j < m) dst[j] = (i0 + j < len) ? src[j] : (int16_t)0;
}

extern "C" {

int adp_abi_version(void) { return ADP_ABI_VERSION; }
int adp_sizeof_cfg(void) { return (int)sizeof(adp_cfg); }
int adp_sizeof_row(void) { return (int)sizeof(adp_row); }
int adp_sizeof_peak_args(void) { return (int)sizeof(adp_peak_args); }
int adp_sizeof_spike_args(void) { return (int)sizeof(adp_spike_args); }
int adp_sizeof_mvs_args(void) { return (int)sizeof(adp_mvs_args); }
const char *adp_last_error(void) { return g_err.c_str(); }

int adp_device_count(void)
{
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    return n;
}

int adp_create(int device, const adp_cfg *cfg, int max_reads, int m, adp_handle **out)
{
    if (!cfg || !out || max_reads < 1 || m < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(device));
    adp_handle *h = new adp_handle();
    h->device = device;
    h->cfg = *cfg;
    h->max_reads = max_reads;
    h->m = m;
    int rc = geom(h);
    if (rc) { delete h; return rc; }
    if (hipStreamCreate(&h->stream) != hipSuccess || hipStreamCreate(&h->stream2) != hipSuccess ||
        hipStreamCreate(&h->stream3) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) { delete h; g_err = "hipStreamCreate failed"; return ADP_ERR_HIP; }
    if (hipEventCreateWithFlags(&h->ev_start, hipEventDisableTiming) != hipSuccess) { adp_destroy(h); g_err = "hipEventCreate failed"; return ADP_ERR_HIP; }
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) h->n_cu = pr.multiProcessorCount; }
    { const char *cv = getenv("ADP_CNN_CONV"); if (cv && !strcmp(cv, "f32")) h->cnn_mode = 0; } // the exact-float32 conv stack (cnn_conv.h)
    *out = h;
    return ADP_OK;
}

int adp_destroy(adp_handle *h)
{
    if (!h) return ADP_OK;
    (void)hipSetDevice(h->device);
    for (int i = 0; i < ADP_MAX_LANES; i++) if (h->lane[i]) { adp_destroy(h->lane[i]); h->lane[i] = nullptr; }
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : h->ev_sync) (void)hipEventDestroy(e);
    if (h->ev_start) (void)hipEventDestroy(h->ev_start);
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
    if (h->stream3) { (void)hipStreamSynchronize(h->stream3); (void)hipStreamDestroy(h->stream3); }
    for (int i = 0; i < 16; i++) if (h->ev_copy[i]) (void)hipEventDestroy(h->ev_copy[i]);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h; // (the DevBufs free their memory)
    return ADP_OK;
}

int adp_set_config(adp_handle *h, const adp_cfg *cfg)
{
    if (!h || !cfg) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cfg = *cfg;
    int rc = geom(h);
    if (rc) return rc;
    for (int i = 0; i < ADP_MAX_LANES; i++) if (h->lane[i]) { h->lane[i]->cfg = *cfg; (void)geom(h->lane[i]); }
    return ADP_OK;
}

void *adp_stream(adp_handle *h) { return h ? (void *)h->stream : nullptr; }

int adp_synchronize(adp_handle *h)
{
    if (!h) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_set_profiling(adp_handle *h, int on)
{
    if (!h) return ADP_ERR_INVALID;
    h->profiling = on != 0;
    return ADP_OK;
}

} // extern "C"

// ---- profiling helpers -------------------------------------------------------------
hipEvent_t next_event(adp_handle *h)
{
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        h->ev_pool.push_back(e);
    }
    return h->ev_pool[h->ev_used++];
}

// what a call reports through adp_kernel_times starts empty (a handle's or a lane's; the repeats of a call drop it too)
static void drop_profile(adp_handle *h) { h->prof.clear(); h->ev_used = 0; }
static void reset_profile(adp_handle *h) { drop_profile(h); h->last_grouped = false; }
// a call that works on the device: the handle's device current, reset_profile
int begin_call(adp_handle *h) { HIPCHK(hipSetDevice(h->device)); reset_profile(h); return ADP_OK; }

// ---- input staging -----------------------------------------------------------------
static int stage_inputs(adp_handle *h, const float *signals, const int32_t *full_len, int n, int m, int flags,
                        const float **dsig, const int32_t **dlen)
{
    if (flags & ADP_IN_DEVICE) { *dsig = signals; *dlen = full_len; return 0; }
    if (h->sig_stage.ensure((size_t)n * m * 4) || h->len_stage.ensure((size_t)n * 4)) { g_err = "staging allocation failed"; return ADP_ERR_HIP; }
    HIPCHK(hipMemcpyAsync(h->sig_stage.p, signals, (size_t)n * m * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->len_stage.p, full_len, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    *dsig = h->sig_stage.as<float>();
    *dlen = h->len_stage.as<int32_t>();
    return 0;
}

static int deliver_rows(adp_handle *h, int n, int flags, adp_row *rows_out)
{
    if (!rows_out) return 0;
    HIPCHK(hipMemcpyAsync(rows_out, h->rows.p, (size_t)n * sizeof(adp_row),
                          (flags & ADP_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return 0;
}

__global__ void k_mb_set_status(MbState *mbs, int n_mb, int status)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_mb) mbs[i].status = status;
}

// a read without any valid pooled block sinks its minibatch (the reference raises there)
__global__ void k_check_empty(const int32_t *nvalid, int n_reads, int mbsize, MbState *mbs)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    if (nvalid[r] <= 0 && mbs[r / mbsize].status == ADP_MB_OK) mbs[r / mbsize].status = ADP_MB_EMPTY_TRACE;
}

__global__ void k_mb_status_out(const MbState *mbs, int n_mb, int32_t *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_mb) out[i] = mbs[i].status;
}

__global__ void k_mb_params_out(const MbState *mbs, int n_mb, double *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_mb) {
        out[4 * i] = (double)mbs[i].med; out[4 * i + 1] = (double)mbs[i].mad;
        out[4 * i + 2] = (double)mbs[i].lo; out[4 * i + 3] = (double)mbs[i].hi;
    }
}

#ifdef ADP_ABLATE
// (common.h: ABLATED) the device's copy is refreshed when the environment's value is not the one this handle copied last
__device__ int g_ablate = 0;
static void sync_ablate(adp_handle *h)
{
    const char *ab = getenv("ADP_ABLATE");
    const int want = ab ? atoi(ab) : 0;
    if (want != h->ablate) {
        (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ablate), &want, sizeof(int), 0, hipMemcpyHostToDevice, h->stream);
        (void)hipStreamSynchronize(h->stream);
        h->ablate = want;
    }
}
#endif

static int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// ---- the open-pore arena of one API call --------------------------------------------------
// arena_begin: allocated, counter zeroed (on the handle's stream, ahead of every kernel of the call).  arena_end (the call's
// stream(s) drained): how much the call wanted; > capacity = lists were dropped: grow and tell the caller to run again.
// op_used: [0] arena words wanted, [1] the split conv stack's out-of-range flag, [2] reads selected for the CNN path's short-read
// fallback, [3] reads selected for its LLR second opinion, [4] reads whose tail window passed the truncation look's T1, or -- the two
// flags exclude each other -- reads selected for the LLR re-segmentation -- zeroed by arena_begin, read by arena_end.  Behind them the
// phases' counts for adp_debug_fetch (10 / 11 / 12 / 25), zeroed by the phase that runs:
// the fallback's [0] exception rows made, [1] rows re-validated; the second opinion's [0] rows replaced, [1] re-validated and still
// failing, [2] minibatches without one; the truncation look's [0] eligible reads, [1] T1 passed, [2] rows replaced; the
// re-segmentation's [0] eligible reads, [1] reads with a second poly(A) end, [2] rows replaced; the same three of the re-segmentation
// behind the second opinion (what = 26) and, as [3], the reads that one selected -- zeroed with its counts and read by arena_end
enum { OPW_FB = 5, OPW_SO = 7, OPW_PT = 10, OPW_RS = 13, OPW_SR = 16, OPW_END = 20 };
static unsigned int *phase_counts(adp_handle *h, int opw) { return h->op_used.as<unsigned int>() + opw; }
static int arena_begin(adp_handle *h)
{
    ALLOCCHK(h->op_used.ensure(OPW_END * 4) || (h->op_arena.cap == 0 && h->op_arena.ensure((size_t)65536 * 4)));
    HIPCHK(hipMemsetAsync(h->op_used.p, 0, 20, h->stream));
    return 0;
}
// -> 0 done, 1 run the call again (arena grown), < 0 error
// (cnn: the call ran the conv stack -- its out-of-range flag is read with the counter; set = repeat the call on the float32 kernels)
// (n_sel: the call ran k_cnn_fb_select -- its count comes with the same copy; left 0 when the call is to be repeated)
// (n_so: the same for k_cnn_so_select; n_pt: for k_pt_select, or k_rs_select; n_sr: for k_csr_select, whose word lies behind the counts)
static int arena_end(adp_handle *h, bool cnn = false, unsigned int *n_sel = nullptr, unsigned int *n_so = nullptr, unsigned int *n_pt = nullptr,
                     unsigned int *n_sr = nullptr)
{
    const bool conv_flag = cnn && h->cnn_mode == 1 && !h->cnn_redo_f32;
    if (n_sel) *n_sel = 0;
    if (n_so) *n_so = 0;
    if (n_pt) *n_pt = 0;
    if (n_sr) *n_sr = 0;
    if (!h->cfg.detect_open_pores && !conv_flag && !n_sel && !n_so && !n_pt && !n_sr) { h->op_last_used = 0; return 0; }
    unsigned int w[OPW_END] = {0};
    HIPCHK(hipMemcpyAsync(w, h->op_used.p, n_sr ? OPW_END * 4 : (n_pt ? 20 : 16), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (conv_flag && w[1]) { h->cnn_redo_f32 = true; return 1; }
    const bool arena_ok = !h->cfg.detect_open_pores || (size_t)w[0] * 4 <= h->op_arena.cap;
    if (n_sel && arena_ok) *n_sel = w[2];
    if (n_so && arena_ok) *n_so = w[3];
    if (n_pt && arena_ok) *n_pt = w[4];
    if (n_sr && arena_ok) *n_sr = w[OPW_SR + 3];
    if (!h->cfg.detect_open_pores) { h->op_last_used = 0; return 0; }
    const unsigned int used = w[0];
    h->op_last_used = used;
    if ((size_t)used * 4 <= h->op_arena.cap) return 0;
    ALLOCCHK(h->op_arena.ensure((size_t)used * 8));
    return 1;
}

// A call's attempts on the arena: attempt() runs behind arena_begin -> 0 done, 1 run the call again (arena_end grew the arena, or
// the conv stack goes to float32), < 0 error.  A repeat drops what the attempt recorded in the handle's profile and its lanes'.
// max_attempts: three, or what the call's phases need (cnn_after_first_pass)
template <class F>
static int call_attempts(adp_handle *h, adp_handle *const *lanes, int n_lanes, F &&attempt, int max_attempts = 3)
{
    for (int a = 0; a < max_attempts; a++) {
        RCCHK(arena_begin(h));
        const int rc = attempt();
        if (rc <= 0) return rc;
        drop_profile(h);
        for (int i = 0; i < n_lanes; i++) drop_profile(lanes[i]);
    }
    g_err = "the call's repeats (conv stack out of the float16 range, open-pore arena growth) are used up and the arena is still short";
    return ADP_ERR_CAPACITY;
}

// the resident matrix types of the detect calls' first passes: the whole matrix, one row per read of the launch (the long-slice
// series kernels and the shared sweeps work on these; a subset read in place -- SigIdx, SigIdxI16 -- has one candidate per read, or,
// behind the re-validating front pass, the read's whole list without prepared statistics: k_validate's own series then)
template <class SIG> struct sig_is_matrix { static constexpr bool value = std::is_same<SIG, SigF32>::value || std::is_same<SIG, SigI16>::value; };

template <int THREADS, int HB, int U, class SIG>
static int launch_cand_stats2(adp_handle *h, SIG sig, const int32_t *dlen, int n, int m, int kmax, int cap)
{
    typedef Cs2Sh<HB> Sh;
    RCCHK(lds_attr_once(h, (const void *)k_cand_stats2<SIG, THREADS, HB, U>, sizeof(Sh)));
    hipLaunchKernelGGL((k_cand_stats2<SIG, THREADS, HB, U>), dim3(n), dim3(THREADS), sizeof(Sh), h->stream, sig, dlen, n, m, h->bounds.as<int64_t>(), kmax, h->cfg,
                       (const float *)h->series.as<float>(), cap, (const int8_t *)h->have_series.as<int8_t>(), h->cstat.as<CandStat>());
    return 0;
}

// where a validation finds its candidates and leaves its rows: the handle's own buffers, unless the call still needs those
// (the second phase of adp_detect_cnn, cnn_fallback_run)
struct ValBufs { const int64_t *bounds; const int8_t *topk_none; adp_row *rows; };

// (FROM: k_validate<SIG, true> with the reads' adapter starts -- device int64 [n], or nullptr -- the only thing the switch changes)
template <bool FROM, class SIG>
static int launch_validate_t(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int kmax, int mbsize,
                             bool gate_mb, const ValBufs *vb, bool polya_truncated, const int64_t *starts)
{
    const int64_t *bounds = vb ? vb->bounds : h->bounds.as<int64_t>();
    adp_row *rows = vb ? vb->rows : h->rows.as<adp_row>();
    if (vb && std::is_same<SIG, SigF32>::value) { g_err = "launch_validate: the float32 series kernels work on the handle's own bounds"; return ADP_ERR_INVALID; }
    ValidateInT<SIG> in;
    in.sig = dsig; in.full_len = dlen; in.bounds = bounds; in.topk_none = vb ? vb->topk_none : h->topk_none.as<int8_t>();
    in.kmax = kmax; in.n_reads = n; in.m = m; in.mbsize = mbsize;
    in.mbs = gate_mb ? h->mbs.as<MbState>() : nullptr;
    in.scratch = h->vscratch.as<float>(); in.scratch_stride = h->vstride;
    in.starts = starts;
    // several candidates per read (the CNN path): moving-window series up to the LARGEST candidate for every read (the
    // window, not MVS_CAP, bounds them), then the order statistics of all candidates in shared sweeps (cand_stats.h)
    // (two shapes of k_cand_stats: big workgroups and wide levels beyond a 32 k preload, small ones below: cand_stats.h)
    const bool multi = sig_is_matrix<SIG>::value && !vb && kmax > 1 && h->cfg.mvs_detect_check && !h->cfg.mvs_detect_overwrite &&
                       h->cfg.pA_var_window <= MS_HIST && h->cfg.pA_mean_window <= MS_HIST;
    const int cap = multi ? h->vstride : MVS_CAP;
    ALLOCCHK(multi && (h->series.ensure((size_t)n * 2 * cap * 4) || h->cstat.ensure((size_t)n * kmax * sizeof(CandStat))));
    in.series = h->series.as<float>(); in.have_series = h->have_series.as<int8_t>(); in.series_cap = cap;
    in.cstat = multi ? h->cstat.as<CandStat>() : nullptr;
    if (h->cfg.mvs_detect_check && !h->cfg.mvs_detect_overwrite) {
        // one candidate per read (the LLR path): the same pipeline of waves over the slice [adapter end, poly(A) end) where it takes the
        // windows (round 4; the lane-per-read kernel k_mvs_series waits on 64 scattered rows per load instruction); ADP_SERIES_PIPE_LLR=0: as before
        bool piped = false;
        if constexpr (sig_is_matrix<SIG>::value) {
        constexpr bool f32 = std::is_same<SIG, SigF32>::value; // (one candidate per read on int16 rows, the LLR path: k_mvs_series<SigI16>, as before)
        const bool pipe_ok = sp_takes(h->cfg.pA_var_window, h->cfg.pA_mean_window) && env_int("ADP_SERIES_PIPE", 1);
        if (multi || (f32 && pipe_ok && kmax == 1 && env_int("ADP_SERIES_PIPE_LLR", 1))) {
            piped = true;
            Scope s(h, multi ? "k_mvs_series_wave" : "k_mvs_series");
            auto ring = [](int w) { int rb = 128; while (rb < w + MS_CHUNK) rb <<= 1; return rb; };
            const size_t lds = (size_t)MS_G * (ring(h->cfg.pA_var_window) + 4 + ring(h->cfg.pA_mean_window) + 4 + 4 * (MS_CHUNK + 4)) * 4; // (two out halves per wave)
            size_t &lds_set = f32 ? h->lds_series_set : h->lds_series_set_i16;
            if (lds > lds_set) { HIPCHK(hipFuncSetAttribute((const void *)k_mvs_series_wave<SIG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); lds_set = lds; }
            // the plan (slice starts / lengths, have[]) and the order by falling length (validate.h), then the chains
            ALLOCCHK(h->series_plan.ensure((size_t)n * 12 + 2 * MS_NBKT * 4));
            int32_t *pa = h->series_plan.as<int32_t>(), *pn = pa + n, *pp = pn + n;
            uint32_t *pc = reinterpret_cast<uint32_t *>(pp + n);
            HIPCHK(hipMemsetAsync(pc, 0, 2 * MS_NBKT * 4, h->stream));
            hipLaunchKernelGGL(k_series_plan, dim3((n + 255) / 256), dim3(256), 0, h->stream, dlen, n, m, h->bounds.as<int64_t>(), kmax, h->cfg, cap,
                               h->have_series.as<int8_t>(), pa, pn, pc);
            hipLaunchKernelGGL(k_series_order, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, cap, pn, pc, pc + MS_NBKT, pp);
            // round 4: the recurrences as a pipeline of waves (series_pipe.h) for the windows it takes; ADP_SERIES_PIPE=0: one wave per recurrence
            if (pipe_ok) {
                RCCHK(lds_attr_once(h, (const void *)k_mvs_series_pipe<SIG>, SP_LDS_FLOATS * 4));
                hipLaunchKernelGGL(k_mvs_series_pipe<SIG>, dim3((n + SP_G - 1) / SP_G), dim3(SP_THREADS), SP_LDS_FLOATS * 4, h->stream, dsig, n, m, pa, pn, pp,
                                   h->cfg.pA_var_window, h->cfg.pA_mean_window, h->series.as<float>(), cap, h->have_series.as<int8_t>());
            } else
            hipLaunchKernelGGL(k_mvs_series_wave<SIG>, dim3((n + MS_G - 1) / MS_G), dim3(128), lds, h->stream, dsig, n, m, pa, pn, pp, h->cfg,
                               h->series.as<float>(), cap, h->have_series.as<int8_t>());
        }
        }
        if (!piped) {
            Scope s(h, "k_mvs_series");
            hipLaunchKernelGGL(k_mvs_series<SIG>, dim3((n + 63) / 64), dim3(64), 0, h->stream, dsig, dlen, n, m, bounds, kmax, h->cfg,
                               h->series.as<float>(), cap, h->have_series.as<int8_t>());
        }
        if constexpr (sig_is_matrix<SIG>::value) {
        if (multi) {
            Scope s(h, "k_cand_stats");
            // two sweeps per array (cand_stats2.h)
            int rc;
                // (shapes tried on one box, 24 000 reads at the 200 k window / 32 000 at the default one: 512 threads x 8 loads in flight 14.3 ms,
                // x 4 14.7, 1024 threads 18.9-19.8; 256 threads x 4 3.5 ms, x 8 4.4, x 2 3.45, 128 threads 4.1-4.2)
                rc = h->m > 32768 ? launch_cand_stats2<512, 12, 8>(h, dsig, dlen, n, m, kmax, cap)
                                  : launch_cand_stats2<256, 10, 4>(h, dsig, dlen, n, m, kmax, cap);
            if (rc) return rc;
        }
        }
    } else {
        (void)hipMemsetAsync(h->have_series.p, 0, (size_t)n, h->stream);
    }
    int grid = n < h->vslots ? n : h->vslots;
#ifdef ADP_ABLATE
    sync_ablate(h);
#endif
    // open-pore lists longer than a row holds go to the arena of the CALL (arena_begin / arena_end: cumulative over every
    // launch of the call, shared by the lanes of a grouped call; a call that overflowed it is repeated on a larger one)
    adp_handle *a = h->owner ? h->owner : h;
    in.op_arena = a->op_arena.as<int32_t>(); in.op_used = a->op_used.as<unsigned int>(); in.op_cap = (unsigned int)(a->op_arena.cap / 4);
    { Scope s(h, "k_validate");
      hipLaunchKernelGGL((k_validate<SIG, FROM>), dim3(grid), dim3(64), 0, h->stream, in, h->cfg, rows, h->preq.as<PartReq>()); }
    if (polya_truncated) { // (Boundaries.polya_truncated: no RNA partition, signal_partitions.py:74-77)
        Scope s(h, "k_pt_preq");
        hipLaunchKernelGGL(k_pt_preq, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->preq.as<PartReq>(), n);
    }
    { Scope s(h, "k_partition_stats");
      // (the kernel is a template on the workgroup size: 512 threads x 2 and 1024 x 1 per CU, and the second pass walking a segment from its
      // end, were measured and dropped in round 5 -- 28.2 / 38.5 against 24.5 ms; +-1 %: profiles/r05_tried_and_dropped.txt)
      hipLaunchKernelGGL((k_partition_stats<SIG, BS_THREADS, 5>), dim3(n), dim3(BS_THREADS), sizeof(BlockScratch), h->stream, dsig, m, h->preq.as<PartReq>(),
                         rows); }
    return 0;
}

template <class SIG>
static int launch_validate(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int kmax, int mbsize,
                           bool gate_mb, const ValBufs *vb = nullptr, bool polya_truncated = false)
{
    return launch_validate_t<false>(h, dsig, dlen, n, m, kmax, mbsize, gate_mb, vb, polya_truncated, nullptr);
}

// N1 for all minibatches (n1_select.h): sampled guess, then ONE verified full pass per statistic when the copied
// bracket holds the rank (k_n1_finish), else the second pass; a missed window falls back to the aligned path.
template <class SIG>
static int launch_n1(adp_handle *h, SIG dsig, int n, int m, int T, int minibatch, int n_mb, bool profile,
                     const int32_t *tails = nullptr) // tails: full_len when ADP_TAILS_NAN holds
{
    hipStream_t st = h->stream;
    h->n1_fused_nmb = 0;
    MbState *mbs = h->mbs.as<MbState>();
    uint32_t *gh = h->ghist.as<uint32_t>(), *gb = h->gbelow.as<uint32_t>();
    unsigned long long *gc = h->gcnt.as<unsigned long long>();
    const int collect = ((long long)minibatch * T >= (1ll << 24)) ? 1 : 0; // only worth it (and sized) for big minibatches
    ALLOCCHK(collect && h->cbuf.ensure((size_t)n_mb * N1_CB_CAP * 4));
    uint32_t *cb = h->cbuf.as<uint32_t>();
    int bpm = 4096 / n_mb; if (bpm > 256) bpm = 256; if (bpm < 4) bpm = 4;
    dim3 hg(bpm, n_mb), pg(n_mb);
    // sample: 1/32 of the minibatch -- of EVERY read `col_div` pieces of ~96 samples, one in each col_div-th of the window
    // at a position that rotates from read to read (short windows: every 32nd read whole)
    const int pdiv = 32;
    int col_div = 1;
    if (T >= 8192) { col_div = T / (pdiv * 96); if (col_div > 64) col_div = 64; if (col_div < 2) col_div = 2; }
    int row_step = (col_div > 1) ? 1 : minibatch / 32; if (row_step < 1) row_step = 1;
    int sb = (minibatch + row_step - 1) / row_step; if (sb > bpm) sb = bpm; if (sb < 1) sb = 1;
    dim3 sg(sb, n_mb);
    const double thr = h->cfg.sig_norm_outlier_thresh;
    // big minibatches: both statistics from ONE pass (n1_fused.h); whatever it cannot verify is left to the passes below
    // (2^22 samples: the reference's defaults -- 1000 reads per minibatch at the preset's 16 000-sample window, 1.6e7 -- lie just
    // under 2^24, where this threshold stood until the end of round 3: the preset ran the three-pass path, 5.3 instead of 3.0 ms per
    // 96 000 reads.  A bracket that misses on a small minibatch costs the fused pass and falls through to those passes.)
    const long long fused_min = getenv("ADP_N1_FUSED_MIN") ? atoll(getenv("ADP_N1_FUSED_MIN")) : (1ll << 22);
    if ((long long)minibatch * T >= fused_min && T >= 64) {
        ALLOCCHK(h->cbuf.ensure((size_t)n_mb * N1_CB_CAP * 4) || h->fz.ensure((size_t)n_mb * sizeof(N1Fused)) ||
                 h->fcnt.ensure((size_t)n_mb * 8 * N1F_NCNT) || h->n1heavy.ensure((size_t)n_mb * N1H_WORDS * 4));
        cb = h->cbuf.as<uint32_t>();
        h->n1_fused_nmb = n_mb; // (adp_debug_fetch 24)
        N1Fused *fz = h->fz.as<N1Fused>();
        unsigned long long *fc = h->fcnt.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(fc, 0, (size_t)n_mb * 8 * N1F_NCNT, st));
        uint32_t *hvy = h->n1heavy.as<uint32_t>();
        HIPCHK(hipMemsetAsync(hvy, 0, (size_t)n_mb * N1H_WORDS * 4, st));
        { Scope s(h, !profile ? nullptr : "k_n1 sample passes");
        // the first level of a statistic's sample only picks the 2^21-key window the second level works in: an eighth of the sampled
        // rows does (ADP_N1_S0: 1 = every sampled row, as before); the second level, whose counts place the bracket, keeps them all
        const int s0 = (col_div > 1 && minibatch >= 64) ? env_int("ADP_N1_S0", 8) : 1;
        for (int mode = 0; mode < 2; mode++) {
            hipLaunchKernelGGL((k_n1_hist<0, SIG>), sg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, row_step * (s0 > 1 ? s0 : 1), N1_ALWAYS, cb, 0, col_div, pdiv, tails);
            hipLaunchKernelGGL((k_n1_pick<0, N1_SAMPLE>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
            hipLaunchKernelGGL((k_n1_hist<1, SIG>), sg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, row_step, N1_ALWAYS, cb, 0, col_div, pdiv, tails);
            hipLaunchKernelGGL((k_n1_pick<1, N1_SAMPLE>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
            hipLaunchKernelGGL(k_n1_fuse_setup, dim3((n_mb + 63) / 64), dim3(64), 0, st, mbs, fz, n_mb, mode);
        }
        // values shared by many of the samples to copy (quantised data): found in the sample, counted instead of copied
        // (a quarter of the sampled rows is plenty to see ties)
        hipLaunchKernelGGL(k_n1_heavy_scan<SIG>, dim3((sb + 3) / 4, n_mb), dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mbs, fz, hvy, row_step * 4, col_div, pdiv, tails);
        hipLaunchKernelGGL(k_n1_heavy_pick, pg, dim3(64), 0, st, mbs, fz, hvy, n_mb); }
        { Scope s(h, !profile ? nullptr : "k_n1_fused");
          hipLaunchKernelGGL(k_n1_fused<SIG>, hg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mbs, fz, fc, (float *)cb, hvy, tails); }
        { Scope s(h, !profile ? nullptr : "k_n1_fused_finish");
          hipLaunchKernelGGL(k_n1_fused_finish, pg, dim3(1024), 0, st, mbs, fz, fc, (const float *)cb, thr, (const uint32_t *)hvy); }
    }
    // behind the fused pass these launches only serve the (rare) minibatch it could not settle: with many minibatches in the call
    // such a minibatch would be left to 4096 / n_mb blocks -- one missed bracket among 96 Pareto-length minibatches cost 3.5 ms of a
    // 50 ms step -- so it gets at least 128 (the blocks of settled minibatches return at once)
    if ((long long)minibatch * T >= fused_min && T >= 64 && bpm < 128) hg = dim3(128, n_mb);
    for (int mode = 0; mode < 2; mode++) {
        // guess from a row sample
        hipLaunchKernelGGL((k_n1_hist<0, SIG>), sg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, row_step, N1_ALWAYS, cb, 0, col_div, pdiv, tails);
        hipLaunchKernelGGL((k_n1_pick<0, N1_SAMPLE>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
        hipLaunchKernelGGL((k_n1_hist<1, SIG>), sg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, row_step, N1_ALWAYS, cb, 0, col_div, pdiv, tails);
        hipLaunchKernelGGL((k_n1_pick<1, N1_SAMPLE>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
        // pass 1 over everything, verified
        { Scope s(h, !profile ? nullptr : (mode ? "k_n1_hist<1> mad" : "k_n1_hist<1> med"));
          hipLaunchKernelGGL((k_n1_hist<1, SIG>), hg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, 1, N1_ALWAYS, cb, collect, 1, 8, tails); }
        hipLaunchKernelGGL((k_n1_pick<1, N1_FULL>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
        hipLaunchKernelGGL(k_n1_finish, pg, dim3(1024), 0, st, mbs, cb, gc, gb, mode, thr);
        // fallback (runs only for minibatches whose guess missed)
        hipLaunchKernelGGL((k_n1_hist<0, SIG>), hg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, 1, N1_IF_BAD, cb, 0, 1, 8, tails);
        hipLaunchKernelGGL((k_n1_pick<0, N1_FALLBACK>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
        hipLaunchKernelGGL((k_n1_hist<1, SIG>), hg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, 1, N1_IF_BAD, cb, 0, 1, 8, tails);
        hipLaunchKernelGGL((k_n1_pick<1, N1_FALLBACK>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
        // pass 2 (only where the bracket did not settle it)
        { Scope s(h, !profile ? nullptr : (mode ? "k_n1_hist<2> mad" : "k_n1_hist<2> med"));
          hipLaunchKernelGGL((k_n1_hist<2, SIG>), hg, dim3(N1_THREADS), 0, st, dsig, n, m, T, minibatch, mode, mbs, gh, gb, gc, 1, N1_IF_NOT_DONE, cb, 0, 1, 8, tails); }
        hipLaunchKernelGGL((k_n1_pick<2, N1_FULL>), pg, dim3(256), 0, st, mbs, gh, gb, gc, mode, thr);
    }
    return 0;
}

// ---- the LLR path over a resident signal matrix: float32 pA (SigF32) or int16 ADC + calibration (SigI16) ----------------
// Three phases per group of minibatches: S (N1 + normalised pooling: streams the signal twice), C (cumulative sums, both
// gains passes, peak picking: float64 ALU / latency, touches only the pooled signal), V (validation + partition statistics:
// streams the signal twice more).  llr_enqueue puts one group on a handle's stream WITHOUT waiting for anything on the host;
// PhaseSync lets the caller order the phases of different groups against each other across streams.
struct PhaseSync {
    hipEvent_t wait[3] = {nullptr, nullptr, nullptr};  // before phase S / C / V: wait for this event (another stream's)
    hipEvent_t done[3] = {nullptr, nullptr, nullptr};  // after phase S / C / V: record this event
};

static __device__ __host__ inline SigF32 sig_from(const SigF32 &s, size_t r0, int m) { return SigF32{s.base + r0 * (size_t)m}; }
static __device__ __host__ inline SigI16 sig_from(const SigI16 &s, size_t r0, int m) { return SigI16{s.base + r0 * (size_t)m, s.scale + r0, s.offset + r0, s.full_len + r0}; }
// the rows sel[0 .. ) of a matrix, read where they lie
static inline SigIdx sig_subset(const SigF32 &s, const int32_t *sel) { return SigIdx{s.base, sel}; }
static inline SigIdxI16 sig_subset(const SigI16 &s, const int32_t *sel) { return SigIdxI16{s.base, s.scale, s.offset, s.full_len, sel}; }

// k_cumsum and k_cumsum_gather share the launch's waves (llr_stream.h; ADP_CUMSUM_GATHER=0: k_cumsum takes them all, same results)
static void launch_cumsum(adp_handle *h, int n)
{
    const int split = env_int("ADP_CUMSUM_GATHER", 1) != 0;
    hipLaunchKernelGGL(k_cumsum, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->down.as<float>(), h->nvalid.as<int32_t>(), h->Lp, n,
                       h->nck, h->ck.as<double2>(), h->tail.as<double2>(), split);
    if (split)
        hipLaunchKernelGGL(k_cumsum_gather, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->down.as<float>(), h->nvalid.as<int32_t>(), h->Lp, n,
                           h->nck, h->ck.as<double2>(), h->tail.as<double2>());
}

// k_gains' fast body for interior tiles (llr_stream.h; ADP_GAINS_TILE_FAST=0: every tile through the plain body, same results)
static int gains_tile_fast() { return env_int("ADP_GAINS_TILE_FAST", 1) != 0; }

// The window of pass 2 in pooled points behind the adapter candidate (llr_stream.h, peaks.h; 0: the whole trace).  ADP_G2_WINDOW, read
// per call: unset -> the default for a full detect call and the whole trace for a staged debug call (whose callers fetch whole
// buffers behind stages 6 and 7); set -> that value for both.  Same results either way.
#define G2_WINDOW_DEFAULT 1024
static int g2_window(int upto)
{
    const char *e = getenv("ADP_G2_WINDOW");
    if (!e || !*e) return upto >= 8 ? G2_WINDOW_DEFAULT : 0;
    const int w = env_int("ADP_G2_WINDOW", G2_WINDOW_DEFAULT);
    return w < 0 ? 0 : (w > (1 << 28) ? (1 << 28) : w);
}
// (mbs: the minibatch states to read instead of the handle's -- the re-segmentation's per-read copies, with mbsize = 1)
static void launch_gains2(adp_handle *h, int n, int mbsize, double *pkv, int win, const int32_t *redo, const MbState *mbs = nullptr)
{
    hipLaunchKernelGGL(k_gains<2>, dim3((n + GAINS_WPB - 1) / GAINS_WPB), dim3(64 * GAINS_WPB), 0, h->stream, h->down.as<float>(), h->nvalid.as<int32_t>(), h->Lp, h->nck,
                       h->ck.as<double2>(), h->tail.as<double2>(), h->adapter_idx.as<int32_t>(), mbsize, mbs ? mbs : h->mbs.as<MbState>(),
                       h->trace.as<double>(), h->bmax.as<double>(), h->bmin.as<double>(), h->nsum, h->t1.as<int2>(), 0, h->pk.as<int32_t>(), h->npk.as<int32_t>(), h->Lp / 2 + 1, h->gstat.as<double>(), n, 5, pkv, gains_tile_fast(),
                       win, h->wend.as<int32_t>(), redo);
}

// pkv: the maxima's heights as k_gains<2> listed them, or null.  ADP_PK_PREFIX=0: the whole list of maxima at once (peaks.h; same results)
// windowed: pass 2 left wend[r] and the reads it cannot decide go to the redo list; redo_pass: over that list, on whole traces
static void launch_polya_peak(adp_handle *h, int n, int mbsize, const double *pkv, bool windowed = false, bool redo_pass = false, const MbState *mbs = nullptr)
{
    const int grid = n < h->pslots ? n : h->pslots;
    hipLaunchKernelGGL(k_polya_peak, dim3(grid), dim3(64), (size_t)(((h->Lp / 2 + 1) + 8) / 16 + 2) * 4, h->stream, h->trace.as<double>(), h->nvalid.as<int32_t>(), h->Lp,
                       h->bmax.as<double>(), h->bmin.as<double>(), h->nsum, h->adapter_idx.as<int32_t>(), n, mbsize, mbs ? mbs : h->mbs.as<MbState>(),
                       h->pk.as<int32_t>(), h->mk.as<uint32_t>(), h->polya_idx.as<int32_t>(), h->npk.as<int32_t>(), pkv, env_int("ADP_PK_PREFIX", PK_PREFIX),
                       (windowed || redo_pass) ? h->wend.as<int32_t>() : (const int32_t *)nullptr, (windowed || redo_pass) ? h->redo.as<int32_t>() : (int32_t *)nullptr, redo_pass ? 1 : 0);
}

template <class SIG>
static int llr_enqueue(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int minibatch, int flags,
                       adp_row *rows_dev, int rows_kind /* hipMemcpyKind of the row delivery */, int32_t *mb_status_dev, double *mb_params_dev,
                       int upto, const PhaseSync *ps)
{
    int rc = 0;
    const int n_mb = (n + minibatch - 1) / minibatch;
    h->last_n = n; h->last_nmb = n_mb;
    ALLOCCHK(h->mbs.ensure((size_t)n_mb * sizeof(MbState)) || h->ghist.ensure((size_t)n_mb * N1_BINS * 4) || h->gbelow.ensure((size_t)n_mb * 8) || h->gcnt.ensure((size_t)n_mb * 8 * N1_NCNT));
    rc = alloc_all(h, n, true);
    if (rc) return rc;
    hipStream_t st = h->stream;
#ifdef ADP_ABLATE
    sync_ablate(h);
#endif
    if (ps && ps->wait[0]) HIPCHK(hipStreamWaitEvent(st, ps->wait[0], 0));
    MbState *mbs = h->mbs.as<MbState>();
    HIPCHK(hipMemsetAsync(mbs, 0, (size_t)n_mb * sizeof(MbState), st));
    HIPCHK(hipMemsetAsync(h->ghist.p, 0, (size_t)n_mb * N1_BINS * 4, st));
    HIPCHK(hipMemsetAsync(h->gbelow.p, 0, (size_t)n_mb * 8, st));
    HIPCHK(hipMemsetAsync(h->gcnt.p, 0, (size_t)n_mb * 8 * N1_NCNT, st));
    const int T = h->T;
    bool sp_forked = false, sp_done = false;
    if (h->L <= 0) {
        hipLaunchKernelGGL(k_mb_set_status, dim3((n_mb + 255) / 256), dim3(256), 0, st, mbs, n_mb, ADP_MB_EMPTY_TRACE);
        if (ps) for (int k = 0; k < 2; k++) { if (k && ps->wait[k]) HIPCHK(hipStreamWaitEvent(st, ps->wait[k], 0)); if (ps->done[k]) HIPCHK(hipEventRecord(ps->done[k], st)); }
    } else {
        // ---- phase S
        const int32_t *tails = (flags & ADP_TAILS_NAN) ? dlen : nullptr;
        rc = launch_n1(h, dsig, n, m, T, minibatch, n_mb, true, tails);
        if (rc) return rc;
        // K1 riding the pooling pass (k_norm_pool<SIG, true>): when both pooling factors agree and min_obs_adapter is a multiple of
        // them the start-peak scan costs no sweep of its own (ADP_SP_FUSED=0: the separate k_start_peak on the side stream)
        const bool sp_fused = upto >= 8 && (flags & ADP_WITH_START_PEAK) && h->layout == ADP_LAYOUT_MINIBATCH &&
                              h->cfg.sp_downscale_factor == h->ds && h->off % h->ds == 0 && T > h->off && env_int("ADP_SP_FUSED", 1) != 0;
        if (sp_fused) {
            ALLOCCHK(h->sphead.ensure((size_t)n * sizeof(SpHead)));
            Scope s(h, "k_sp_head");
            hipLaunchKernelGGL(k_sp_head<SIG>, dim3(n), dim3(64), (size_t)64 * h->cfg.sp_downscale_factor * 4, st, dsig, dlen, n, m, h->cfg, h->off, h->sphead.as<SpHead>());
        }
        if (upto >= 2 && sp_fused) {
            { Scope s(h, "k_norm_pool");
              // (float32 rows only: the int16 rows' conversion pushes the prefetching variant to 112 registers, 4 waves per SIMD -- 24 vs 14 ms)
              auto kern = (h->ds == 10 && std::is_same<SIG, SigF32>::value && env_int("ADP_NP_PREFETCH", 1)) ? k_norm_pool<SIG, true, 5> : k_norm_pool<SIG, true, 0>;
              hipLaunchKernelGGL(kern, dim3(n), dim3(256), (size_t)NP_TILE * h->ds * 4, st, dsig, m, T, h->off, h->ds, h->L, h->Lp,
                                 minibatch, mbs, h->down.as<float>(), h->nvalid.as<int32_t>(), (const int64_t *)nullptr,
                                 dlen, (flags & ADP_TAILS_NAN) ? 1 : 0, h->sphead.as<SpHead>(), (float)h->cfg.open_pore_pa); }
            const int cov0 = h->off / h->ds, cov1 = cov0 + (T - h->off) / h->ds;
            Scope s(h, "k_sp_tail");
            hipLaunchKernelGGL(k_sp_tail<SIG>, dim3(n), dim3(64), (size_t)64 * h->cfg.sp_downscale_factor * 4, st, dsig, dlen, n, m, h->cfg, cov0, cov1,
                               (const SpHead *)h->sphead.as<SpHead>(), h->sp.as<SpOut>());
            sp_done = true;
        } else if (upto >= 2) {
            Scope s(h, "k_norm_pool");
            const int64_t *rng = nullptr;
            if (h->layout == ADP_LAYOUT_SINGLE_READ) {
                // the reference pools the unpadded read: its last, ragged block is filled up with zeros at the READ's end
                // (downscale.py:22-29), which is what the per-read range [0, min(T, full_len)) does here
                ALLOCCHK(h->rng0.ensure((size_t)n * 16));
                std::vector<int64_t> hr((size_t)2 * n);
                for (int i = 0; i < n; i++) { hr[2 * i] = 0; hr[2 * i + 1] = T; }
                HIPCHK(hipMemcpyAsync(h->rng0.p, hr.data(), (size_t)n * 16, hipMemcpyHostToDevice, st));
                HIPCHK(hipStreamSynchronize(st)); // (hr goes out of scope; this layout is never grouped)
                rng = h->rng0.as<int64_t>();
            }
            auto kern = (h->ds == 10 && !rng && std::is_same<SIG, SigF32>::value && env_int("ADP_NP_PREFETCH", 1)) ? k_norm_pool<SIG, false, 5> : k_norm_pool<SIG, false, 0>;
            hipLaunchKernelGGL(kern, dim3(n), dim3(256), (size_t)NP_TILE * h->ds * 4, st, dsig, m, T, h->off, h->ds, h->L, h->Lp,
                               minibatch, mbs, h->down.as<float>(), h->nvalid.as<int32_t>(), rng,
                               dlen, (flags & ADP_TAILS_NAN) ? 1 : 0, (SpHead *)nullptr, 0.f);
        }
        if (upto >= 2)
            hipLaunchKernelGGL(k_check_empty, dim3((n + 255) / 256), dim3(256), 0, st, h->nvalid.as<int32_t>(), n, minibatch, mbs);
        if (ps && ps->done[0]) HIPCHK(hipEventRecord(ps->done[0], st));
        if (upto >= 8 && (flags & ADP_WITH_START_PEAK) && !sp_fused) {
            // the start-peak scan depends on nothing computed here: it streams the signal on the side stream while the
            // main stream runs the ALU-bound cumulative sums and gains
            HIPCHK(hipEventRecord(h->ev_fork, st));
            HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
            { Scope s(h, "k_start_peak", h->stream2);
              hipLaunchKernelGGL(k_start_peak<SIG>, dim3(n), dim3(64), (size_t)64 * h->cfg.sp_downscale_factor * 4, h->stream2, dsig, dlen, n, m, h->cfg, h->sp.as<SpOut>()); }
            HIPCHK(hipEventRecord(h->ev_join, h->stream2));
            sp_forked = true;
        }
        // ---- phase C
        if (ps && ps->wait[1]) HIPCHK(hipStreamWaitEvent(st, ps->wait[1], 0));
        if (upto >= 3) {
            Scope s(h, "k_cumsum");
            launch_cumsum(h, n);
        }
        if (upto >= 4) {
            Scope s(h, "k_gains<1>");
            hipLaunchKernelGGL(k_gains<1>, dim3((n + GAINS_WPB - 1) / GAINS_WPB), dim3(64 * GAINS_WPB), 0, st, h->down.as<float>(), h->nvalid.as<int32_t>(), h->Lp, h->nck,
                               h->ck.as<double2>(), h->tail.as<double2>(), h->adapter_idx.as<int32_t>(), minibatch, mbs,
                               h->trace.as<double>(), h->bmax.as<double>(), h->bmin.as<double>(), h->nsum, h->t1.as<int2>(), 0, h->pk.as<int32_t>(), h->npk.as<int32_t>(), h->Lp / 2 + 1, h->gstat.as<double>(), n, h->oh1, nullptr, gains_tile_fast());
        }
        if (upto >= 5) {
            Scope s(h, "k_adapter_peak");
            hipLaunchKernelGGL(k_adapter_peak, dim3(n), dim3(64), 0, st, h->trace.as<double>(), h->nvalid.as<int32_t>(), h->Lp,
                               h->bmax.as<double>(), h->bmin.as<double>(), h->nsum, h->t1.as<int2>(), minibatch, mbs,
                               h->cfg.adapter_peak_prominence, h->cfg.adapter_peak_rel_height,
                               h->cfg.adapter_peak_width / h->ds, h->adapter_idx.as<int32_t>(), h->gstat.as<double>());
        }
        // (ADP_PK_VALUES=0: k_polya_peak gathers the heights from the trace, as before round 4; a handle made without the buffer keeps doing so)
        double *pkvp = (env_int("ADP_PK_VALUES", 1) && h->pkv.cap >= (size_t)n * (h->Lp / 2 + 1) * 8) ? h->pkv.as<double>() : nullptr;
        // pass 2 over a window behind the adapter candidate; the reads the window does not settle are listed on the device and
        // both kernels run again over the list with the whole trace -- no count comes back to the host, the launches cover the
        // worst case and leave at once where the list ends
        int win = g2_window(upto);
        // (a window whose first tiles already hold the longest trace is the whole trace for every read: no list, no second launches)
        if (win > 0 && (win + 1 + TRACE_TILE - 1) / TRACE_TILE * TRACE_TILE >= h->L) win = 0;
        if (upto >= 6) {
            if (win > 0) HIPCHK(hipMemsetAsync(h->redo.p, 0, 4, st));
            Scope s(h, "k_gains<2>");
            launch_gains2(h, n, minibatch, pkvp, win, nullptr);
        }
        if (upto >= 7) {
            { Scope s(h, "k_polya_peak");
              launch_polya_peak(h, n, minibatch, pkvp, win > 0); }
            if (win > 0) {
                { Scope s(h, "k_gains<2> redo");
                  launch_gains2(h, n, minibatch, pkvp, 0, h->redo.as<int32_t>()); }
                { Scope s(h, "k_polya_peak redo");
                  launch_polya_peak(h, n, minibatch, pkvp, false, true); }
            }
        }
        if (ps && ps->done[1]) HIPCHK(hipEventRecord(ps->done[1], st));
    }
    if (upto >= 8) {
        // ---- phase V
        if (ps && ps->wait[2]) HIPCHK(hipStreamWaitEvent(st, ps->wait[2], 0));
        if (h->L > 0)
            hipLaunchKernelGGL(k_llr_bounds, dim3((n + 255) / 256), dim3(256), 0, st, h->adapter_idx.as<int32_t>(),
                               h->polya_idx.as<int32_t>(), n, h->ds, h->pos_off, h->bounds.as<int64_t>(), h->topk_none.as<int8_t>(), h->layout == ADP_LAYOUT_SINGLE_READ ? 1 : 0);
        rc = launch_validate(h, dsig, dlen, n, m, 1, minibatch, true);
        if (rc) return rc;
        if (flags & ADP_WITH_START_PEAK) {
            if (sp_forked) HIPCHK(hipStreamWaitEvent(st, h->ev_join, 0));
            else if (!sp_done) {
                Scope s(h, "k_start_peak");
                hipLaunchKernelGGL(k_start_peak<SIG>, dim3(n), dim3(64), (size_t)64 * h->cfg.sp_downscale_factor * 4, st, dsig, dlen, n, m, h->cfg, h->sp.as<SpOut>());
            }
            hipLaunchKernelGGL(k_sp_decorate, dim3((n + 255) / 256), dim3(256), 0, st, h->sp.as<SpOut>(), h->rows.as<adp_row>(), n, 0,
                               (const int32_t *)nullptr);
        }
        if (rows_dev)
            HIPCHK(hipMemcpyAsync(rows_dev, h->rows.p, (size_t)n * sizeof(adp_row), (hipMemcpyKind)rows_kind, st));
    }
    if (mb_status_dev)
        hipLaunchKernelGGL(k_mb_status_out, dim3((n_mb + 255) / 256), dim3(256), 0, st, mbs, n_mb, mb_status_dev);
    if (mb_params_dev)
        hipLaunchKernelGGL(k_mb_params_out, dim3((n_mb + 255) / 256), dim3(256), 0, st, mbs, n_mb, mb_params_dev);
    if (ps && ps->done[2]) HIPCHK(hipEventRecord(ps->done[2], st));
    HIPCHK(hipGetLastError());
    return ADP_OK;
}

// ---- the truncation look (ADP_FLAG_TRUNCATED, polya_truncated.h) --------------------------------------------------------------
static bool trunc_wanted(int flags, const adp_row *rows) { return (flags & ADP_FLAG_TRUNCATED) && rows; }
// what the flag cannot go with, said before anything is launched
static int trunc_supported(const adp_handle *h)
{
    const adp_cfg &c = h->cfg;
    const int W = c.median_shift_window;
    if (!c.mvs_detect_check) { g_err = "ADP_FLAG_TRUNCATED needs mvs_detect_check (its tests are the MVS check's)"; return ADP_ERR_UNSUPPORTED; }
    if (c.mvs_detect_overwrite) { g_err = "ADP_FLAG_TRUNCATED does not go with mvs_detect_overwrite"; return ADP_ERR_UNSUPPORTED; }
    if (h->layout == ADP_LAYOUT_SINGLE_READ) { g_err = "ADP_FLAG_TRUNCATED does not go with the single-read layout"; return ADP_ERR_UNSUPPORTED; }
    if (W > PT_WMAX) { g_err = "ADP_FLAG_TRUNCATED: median_shift_window is longer than the tail test holds in LDS (4096)"; return ADP_ERR_UNSUPPORTED; }
    if (c.pA_var_window < 1 || c.pA_mean_window < 1 || c.pA_var_window + 2 >= W || c.pA_mean_window + 2 >= W) {
        g_err = "ADP_FLAG_TRUNCATED: pA_mean_window and pA_var_window must lie in [1, median_shift_window - 3]"; return ADP_ERR_UNSUPPORTED;
    }
    return 0;
}
// T1 over the n rows of the CALL's device row buffer once every read's final row is in it, and the selection; the count reaches the
// host in arena_end's copy (n_pt).
static int trunc_enqueue_t1(adp_handle *h, const float *dsig, const int32_t *dlen, int n, int m, adp_row *rows)
{
    int8_t *verdict;
    ALLOCCHK(h->pt_sel.ensure((size_t)n * 4));
    RCCHK(sub_carve(h, [&](Carve &c) { verdict = c.take<int8_t>(n); }));
    unsigned int *counts = phase_counts(h, OPW_PT);
    h->pt_looked = true;
    HIPCHK(hipMemsetAsync(counts, 0, 12, h->stream));
    { Scope s(h, "k_pt_t1");
      hipLaunchKernelGGL(k_pt_t1, dim3(n), dim3(64), (size_t)3 * h->cfg.median_shift_window * 4, h->stream, dsig, dlen, n, m, h->cfg, rows, verdict); }
    { Scope s(h, "k_pt_select");
      hipLaunchKernelGGL(k_pt_select, dim3(1), dim3(SEL_THREADS), 0, h->stream, (const int8_t *)verdict, n, h->pt_sel.as<int32_t>(),
                         h->op_used.as<unsigned int>() + 4, counts); }
    return 0;
}
// T2 and the merge for the n_t1 reads that passed T1, enqueued on the handle's stream.  T2's rows have a buffer of their own (the
// handle's may be the call's); their open-pore lists append to the call's arena: the caller looks at its counter once more.
static int trunc_run_t2(adp_handle *h, const float *dsig, const int32_t *dlen, int m, adp_row *rows, int n_t1)
{
    int rc = alloc_all(h, n_t1, false);
    if (rc) return rc;
    const size_t N = (size_t)n_t1;
    int64_t *b2; int32_t *dlen_sub; int8_t *tsub; adp_row *rows2;
    RCCHK(sub_carve(h, [&](Carve &c) { // (T1's verdicts are spent)
        b2 = c.take<int64_t>(2 * N); dlen_sub = c.take<int32_t>(N); tsub = c.take<int8_t>(N); rows2 = c.take<adp_row>(N);
    }));
    const int32_t *sel = h->pt_sel.as<int32_t>();
    { Scope s(h, "k_pt_gather");
      hipLaunchKernelGGL(k_pt_gather, dim3((n_t1 + 255) / 256), dim3(256), 0, h->stream, sel, n_t1, m, dlen, (const adp_row *)rows, dlen_sub, b2, tsub); }
    const ValBufs vb{b2, tsub, rows2};
    rc = launch_validate(h, SigIdx{dsig, sel}, dlen_sub, n_t1, m, 1, n_t1, false, &vb, true);
    if (rc) return rc;
    { Scope s(h, "k_pt_merge");
      hipLaunchKernelGGL(k_pt_merge, dim3(n_t1), dim3(64), 0, h->stream, sel, n_t1, (const adp_row *)rows2, rows, phase_counts(h, OPW_PT)); }
    HIPCHK(hipGetLastError());
    return 0;
}
// The look behind a call whose rows are final in `rows` (device) and whose lanes, if any, have drained: T1 and the selection in
// front of the arena counter, which brings their count, then T2 where a tail window passed -> 0 done, 1 run the call again (arena
// grown), < 0 error.
static int trunc_finish(adp_handle *h, const float *dsig, const int32_t *dlen, int n, int m, adp_row *rows)
{
    unsigned int n_pt = 0;
    RCCHK(trunc_enqueue_t1(h, dsig, dlen, n, m, rows));
    const int rc = arena_end(h, false, nullptr, nullptr, &n_pt); // (with n_pt it copies the counter and waits for the stream)
    if (rc || !n_pt) return rc;
    RCCHK(trunc_run_t2(h, dsig, dlen, m, rows, (int)n_pt));
    HIPCHK(hipStreamSynchronize(h->stream));
    return arena_end(h);
}
// ---- the re-segmentation of failed reads (ADP_LLR_RESEGMENT, llr_resegment.h) ---------------------------------------------------
static bool reseg_wanted(int flags, const adp_row *rows) { return (flags & ADP_LLR_RESEGMENT) && rows; }
// what the flag cannot go with, said before anything is launched
static int reseg_supported(const adp_handle *h, int flags)
{
    if (flags & ADP_FLAG_TRUNCATED) { g_err = "ADP_LLR_RESEGMENT does not go with ADP_FLAG_TRUNCATED (the truncation look validates from start 0)"; return ADP_ERR_UNSUPPORTED; }
    if (h->cfg.mvs_detect_overwrite) { g_err = "ADP_LLR_RESEGMENT does not go with mvs_detect_overwrite"; return ADP_ERR_UNSUPPORTED; }
    if (h->layout == ADP_LAYOUT_SINGLE_READ) { g_err = "ADP_LLR_RESEGMENT does not go with the single-read layout"; return ADP_ERR_UNSUPPORTED; }
    return 0;
}
// the per-subset arrays of a re-segmentation over (up to) N reads: the bounds and adapter starts of its validation, full_len,
// polya_end_topk's None-ness, each read's own minibatch state, the rows of the validation
struct RsPieces {
    Piece<int64_t> b2, starts; Piece<int32_t> dlen_sub; Piece<int8_t> tsub; Piece<MbState> mbs_sub; Piece<adp_row> rows2;
    void take(Carve &c, size_t N)
    {
        b2 = c.take<int64_t>(2 * N); starts = c.take<int64_t>(N); dlen_sub = c.take<int32_t>(N); tsub = c.take<int8_t>(N);
        mbs_sub = c.take<MbState>(N); rows2 = c.take<adp_row>(N);
    }
};
// What lies between a re-segmentation's gather and its merge (the LLR primary's, reseg_run; the one behind the CNN primary's second
// opinion, cnn_sr_run): the second segmentation of the n_rs gathered reads -- sig: the subset's rows read where they lie; the
// gather left pass 2's starts in h->adapter_idx -- p2 into the bounds with counts[1], and the validation from the reads' adapter
// starts into p.rows2.  tails_nan: the pooling pass stops at a read's end (ADP_TAILS_NAN, or int16 rows)
template <class SUB>
static int reseg_trace_validate(adp_handle *h, SUB sig, const RsPieces &p, int m, bool tails_nan, int n_rs, unsigned int *counts)
{
    hipStream_t st = h->stream;
    const size_t N = (size_t)n_rs;
    const Piece<int64_t> &b2 = p.b2, &starts = p.starts; const Piece<int32_t> &dlen_sub = p.dlen_sub; const Piece<int8_t> &tsub = p.tsub;
    const Piece<MbState> &mbs_sub = p.mbs_sub; const Piece<adp_row> &rows2 = p.rows2;
    // the trace phase as llr_enqueue runs it (an eligible read has a poly(A) end: h->L > 0), every read its own "minibatch"
    { Scope s(h, "k_norm_pool (resegment)");
      hipLaunchKernelGGL((k_norm_pool<SUB>), dim3(n_rs), dim3(256), (size_t)NP_TILE * h->ds * 4, st, sig, m, h->T, h->off, h->ds, h->L, h->Lp, 1,
                         (const MbState *)mbs_sub.p, h->down.as<float>(), h->nvalid.as<int32_t>(), (const int64_t *)nullptr, (const int32_t *)dlen_sub.p,
                         tails_nan ? 1 : 0); }
    { Scope s(h, "k_cumsum (resegment)");
      launch_cumsum(h, n_rs); }
    double *pkvp = (env_int("ADP_PK_VALUES", 1) && h->pkv.cap >= N * (h->Lp / 2 + 1) * 8) ? h->pkv.as<double>() : nullptr;
    int win = g2_window(8);
    if (win > 0 && (win + 1 + TRACE_TILE - 1) / TRACE_TILE * TRACE_TILE >= h->L) win = 0;
    if (win > 0) HIPCHK(hipMemsetAsync(h->redo.p, 0, 4, st));
    { Scope s(h, "k_gains<2> (resegment)");
      launch_gains2(h, n_rs, 1, pkvp, win, nullptr, mbs_sub.p); }
    { Scope s(h, "k_polya_peak (resegment)");
      launch_polya_peak(h, n_rs, 1, pkvp, win > 0, false, mbs_sub.p); }
    if (win > 0) {
        Scope s(h, "k_gains<2> / k_polya_peak redo (resegment)");
        launch_gains2(h, n_rs, 1, pkvp, 0, h->redo.as<int32_t>(), mbs_sub.p);
        launch_polya_peak(h, n_rs, 1, pkvp, false, true, mbs_sub.p);
    }
    { Scope s(h, "k_rs_bounds");
      hipLaunchKernelGGL(k_rs_bounds, dim3((n_rs + 255) / 256), dim3(256), 0, st, (const int32_t *)h->polya_idx.as<int32_t>(), n_rs, h->ds, h->pos_off, b2.p, tsub.p, counts); }
    const ValBufs vb{b2.p, tsub.p, rows2.p};
    return launch_validate_t<true>(h, sig, dlen_sub.p, n_rs, m, 1, n_rs, false, &vb, false, starts.p);
}
// The second segmentation, its validation and the merge for the n_rs selected reads, enqueued on the handle's stream.  The first
// pass has drained: its stage buffers on this handle are spent (a grouped call's owner has none yet) and take the subset's trace
// phase, read j of the subset at position j.  The second rows have a buffer of their own (the handle's may be the call's); their
// open-pore lists append to the call's arena: the caller looks at its counter once more.
// mbs: the call's minibatch states (the handle's own, or the copies a grouped call's lanes left in rs_mbs)
static int reseg_run(adp_handle *h, const float *dsig, const int32_t *dlen, int m, int minibatch, int flags, adp_row *rows, const MbState *mbs, int n_rs)
{
    hipStream_t st = h->stream;
    RCCHK(alloc_all(h, n_rs, true));
    RsPieces p;
    RCCHK(sub_carve(h, [&](Carve &c) { p.take(c, (size_t)n_rs); }));
    const int32_t *sel = h->rs_sel.as<int32_t>();
    unsigned int *counts = phase_counts(h, OPW_RS);
    { Scope s(h, "k_rs_gather");
      hipLaunchKernelGGL(k_rs_gather, dim3((n_rs + 255) / 256), dim3(256), 0, st, sel, n_rs, minibatch, mbs, dlen, (const adp_row *)rows, h->ds, h->pos_off,
                         p.dlen_sub.p, p.starts.p, p.b2.p, p.tsub.p, h->adapter_idx.as<int32_t>(), p.mbs_sub.p); }
    RCCHK(reseg_trace_validate(h, SigIdx{dsig, sel}, p, m, (flags & ADP_TAILS_NAN) != 0, n_rs, counts));
    { Scope s(h, "k_rs_merge");
      hipLaunchKernelGGL(k_rs_merge, dim3(n_rs), dim3(64), 0, st, sel, n_rs, (const adp_row *)p.rows2.p, rows, counts); }
    HIPCHK(hipGetLastError());
    return 0;
}
// The phase behind a call whose first rows are all in `rows` (device) and whose lanes, if any, have drained: the selection in front
// of the arena counter, which brings its count, then the rest where a read was selected -> 0 done, 1 run the call again (arena
// grown), < 0 error
static int reseg_finish(adp_handle *h, const float *dsig, const int32_t *dlen, int n, int m, int minibatch, int flags, adp_row *rows, const MbState *mbs)
{
    ALLOCCHK(h->rs_sel.ensure((size_t)n * 4));
    unsigned int *counts = phase_counts(h, OPW_RS);
    h->rs_ran = true;
    HIPCHK(hipMemsetAsync(counts, 0, 12, h->stream));
    { Scope s(h, "k_rs_select");
      hipLaunchKernelGGL(k_rs_select, dim3(1), dim3(SEL_THREADS), 0, h->stream, (const adp_row *)rows, n, minibatch, mbs, h->rs_sel.as<int32_t>(),
                         h->op_used.as<unsigned int>() + 4, counts); }
    unsigned int n_rs = 0;
    const int rc = arena_end(h, false, nullptr, nullptr, &n_rs); // (with the count it copies the counter and waits for the stream)
    if (rc || !n_rs) return rc;
    if (n_rs > (unsigned int)n) { g_err = "ADP_LLR_RESEGMENT: selection count out of range"; return ADP_ERR_HIP; }
    RCCHK(reseg_run(h, dsig, dlen, m, minibatch, flags, rows, mbs, (int)n_rs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return arena_end(h);
}
// What the LLR path does behind llr_enqueue's last group, in both execution forms: the arena counter and, with look, the truncation
// look on the rows, or, with reseg, the re-segmentation (float32 signals only: adp_detect_llr_i16 refuses both flags; they exclude
// each other) -> as arena_end.  mbs: the call's minibatch states, for the re-segmentation
static int llr_after_first_pass(adp_handle *h, SigF32 dsig, const int32_t *dlen, int n, int m, int minibatch, int flags, adp_row *rows, bool look, bool reseg,
                                const MbState *mbs)
{
    if (reseg) return reseg_finish(h, dsig.base, dlen, n, m, minibatch, flags, rows, mbs);
    return look ? trunc_finish(h, dsig.base, dlen, n, m, rows) : arena_end(h);
}
static int llr_after_first_pass(adp_handle *h, SigI16, const int32_t *, int, int, int, int, adp_row *, bool, bool, const MbState *) { return arena_end(h); }

// how a call's minibatches are cut into groups: ADP_GROUPS (unset / 1: one group = the plain serial pipeline, 0: automatic = three
// groups per lane, k: aim at k groups); ADP_LANES (streams the groups rotate over, default 2); ADP_STAGGER (bit p set: phase p of
// group g + 1 starts after phase p of group g; default 1 = the streaming S phases take turns, which keeps neighbouring groups one
// phase apart)

static int lane_get(adp_handle *h, int i, int reads, adp_handle **out)
{
    adp_handle *l = h->lane[i];
    if (!l) {
        int rc = adp_create(h->device, &h->cfg, h->max_reads, h->m, &l);
        if (rc) return rc;
        l->owner = h;
        l->n_cu = h->n_cu;
        h->lane[i] = l;
    }
    l->profiling = h->profiling;
    *out = l;
    (void)reads;
    return 0;
}

template <class SIG>
static int llr_grouped(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int minibatch, int flags, adp_row *rows_out,
                       int32_t *mb_status, int mb_per_group, int n_lanes)
{
    const int n_mb = (n + minibatch - 1) / minibatch;
    const int G = (n_mb + mb_per_group - 1) / mb_per_group;
    const int stagger = env_int("ADP_STAGGER", 1);
    h->last_n = n; h->last_nmb = n_mb; h->last_grouped = true;
    const bool out_dev = (flags & ADP_OUT_DEVICE) != 0;
    ALLOCCHK(h->mbstat.ensure((size_t)n_mb * 4) || h->mbparams.ensure((size_t)n_mb * 32) || (rows_out && !out_dev && h->rows.ensure((size_t)n * sizeof(adp_row))));
    while (h->ev_sync.size() < (size_t)G * 3) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ev_sync.push_back(e);
    }
    adp_handle *lanes[ADP_MAX_LANES];
    for (int i = 0; i < n_lanes; i++) {
        RCCHK(lane_get(h, i, mb_per_group * minibatch, &lanes[i]));
        drop_profile(lanes[i]);
    }
    adp_row *rows_dev = rows_out ? (out_dev ? rows_out : h->rows.as<adp_row>()) : nullptr;
    const bool reseg = reseg_wanted(flags, rows_dev);
    ALLOCCHK(reseg && h->rs_mbs.ensure((size_t)n_mb * sizeof(MbState)));
    RCCHK(call_attempts(h, lanes, n_lanes, [&]() -> int {
        HIPCHK(hipEventRecord(h->ev_start, h->stream));      // (inputs staged on this stream, arena counter zeroed)
        for (int i = 0; i < n_lanes; i++) HIPCHK(hipStreamWaitEvent(lanes[i]->stream, h->ev_start, 0));
        for (int g = 0; g < G; g++) {
            adp_handle *l = lanes[g % n_lanes];
            const int mb0 = g * mb_per_group, r0 = mb0 * minibatch;
            const int ng = (n - r0) < mb_per_group * minibatch ? (n - r0) : mb_per_group * minibatch;
            PhaseSync ps;
            for (int p = 0; p < 3; p++) {
                ps.done[p] = h->ev_sync[(size_t)g * 3 + p];
                if (g > 0 && (stagger >> p & 1)) ps.wait[p] = h->ev_sync[(size_t)(g - 1) * 3 + p];
            }
            const int rc = llr_enqueue(l, sig_from(dsig, (size_t)r0, m), dlen + r0, ng, m, minibatch, flags, rows_dev ? rows_dev + r0 : nullptr,
                                       hipMemcpyDeviceToDevice, h->mbstat.as<int32_t>() + mb0, h->mbparams.as<double>() + 4 * (size_t)mb0, 8, &ps);
            if (rc) { for (int i = 0; i < n_lanes; i++) (void)hipStreamSynchronize(lanes[i]->stream); return rc; }
            // (the lane's states are zeroed for its next group: the re-segmentation reads the call's from the owner's copy)
            if (reseg) HIPCHK(hipMemcpyAsync(h->rs_mbs.as<MbState>() + mb0, l->mbs.p, (size_t)((ng + minibatch - 1) / minibatch) * sizeof(MbState),
                                             hipMemcpyDeviceToDevice, l->stream));
        }
        for (int i = 0; i < n_lanes; i++) HIPCHK(hipStreamSynchronize(lanes[i]->stream));
        return llr_after_first_pass(h, dsig, dlen, n, m, minibatch, flags, rows_dev, trunc_wanted(flags, rows_dev), reseg, h->rs_mbs.as<MbState>());
    }));
    if (rows_out && !out_dev) HIPCHK(hipMemcpyAsync(rows_out, h->rows.p, (size_t)n * sizeof(adp_row), hipMemcpyDeviceToHost, h->stream));
    if (mb_status) HIPCHK(hipMemcpyAsync(mb_status, h->mbstat.p, (size_t)n_mb * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

template <class SIG>
static int llr_pipeline_t(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int minibatch, int flags,
                          adp_row *rows_out, int32_t *mb_status, int upto)
{
    const int n_mb = (n + minibatch - 1) / minibatch;
    // grouped execution is OPT-IN (ADP_GROUPS > 1): measured on MI355X, overlapping the float64 gains of one group with the
    // streaming passes of its neighbour buys nothing (+-1.5 %, profiles/r03_overlap_*: the kernels do run side by side -- two or
    // more resident for 82 % of the busy time -- and stretch each other by the same factor; even a PURE read beside a PURE
    // float64 FMA kernel reaches only 0.81-0.88 of the serial time on this chip), while one launch over all reads of the
    // call has the shortest tails.  What grouping does buy is memory: the lanes' workspace is sized for one group.
    int want = env_int("ADP_GROUPS", 1), n_lanes = env_int("ADP_LANES", 2);
    if (n_lanes < 1) n_lanes = 1;
    if (n_lanes > ADP_MAX_LANES) n_lanes = ADP_MAX_LANES;
    if (want <= 0) want = 3 * n_lanes;
    if (upto == 8 && h->layout == ADP_LAYOUT_MINIBATCH && n_mb >= 2 && want > 1) {
        int per = (n_mb + want - 1) / want;
        if (per < 1) per = 1;
        if ((n_mb + per - 1) / per < n_lanes) n_lanes = (n_mb + per - 1) / per;
        return llr_grouped(h, dsig, dlen, n, m, minibatch, flags, rows_out, mb_status, per, n_lanes);
    }
    h->last_grouped = false;
    // ADP_FLAG_TRUNCATED: the look rides behind the validation on the device rows (the caller's, or the handle's -- host rows are
    // then delivered once, behind it); its T1 count comes back with the arena counter
    // ADP_LLR_RESEGMENT: the same arrangement (the two flags exclude each other; `pt` below stands for either)
    const bool look = upto >= 8 && trunc_wanted(flags, rows_out), reseg = upto >= 8 && reseg_wanted(flags, rows_out);
    const bool pt = look || reseg, out_dev = (flags & ADP_OUT_DEVICE) != 0;
    return call_attempts(h, nullptr, 0, [&]() -> int {
        RCCHK(llr_enqueue(h, dsig, dlen, n, m, minibatch, flags, upto >= 8 && !(pt && !out_dev) ? rows_out : nullptr,
                          out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, nullptr, nullptr, upto, nullptr));
        if (mb_status) {
            // through a small device buffer -> host
            hipLaunchKernelGGL(k_mb_status_out, dim3((n_mb + 255) / 256), dim3(256), 0, h->stream, h->mbs.as<MbState>(), n_mb, h->gbelow.as<int32_t>());
            HIPCHK(hipMemcpyAsync(mb_status, h->gbelow.p, (size_t)n_mb * 4, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        if (upto < 8) return 0;
        const int rc = llr_after_first_pass(h, dsig, dlen, n, m, minibatch, flags, out_dev ? rows_out : h->rows.as<adp_row>(), look, reseg, h->mbs.as<MbState>());
        if (rc == 0 && pt && !out_dev) {
            HIPCHK(hipMemcpyAsync(rows_out, h->rows.p, (size_t)n * sizeof(adp_row), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
        return rc;
    });
}

static int llr_pipeline(adp_handle *h, const float *signals, const int32_t *full_len, int n, int m, int minibatch, int flags,
                        adp_row *rows_out, int32_t *mb_status, int upto)
{
    if (!h || !signals || !full_len || n < 1 || minibatch < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (n > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    if (h->layout == ADP_LAYOUT_SINGLE_READ && minibatch != 1) { g_err = "the single-read layout normalises every read on its own: minibatch must be 1"; return ADP_ERR_INVALID; }
    if (flags & ADP_CNN_SECOND_RESEGMENT) { g_err = "ADP_CNN_SECOND_RESEGMENT goes with adp_detect_cnn and ADP_CNN_SECOND_LLR (the CNN primary)"; return ADP_ERR_UNSUPPORTED; }
    h->pt_looked = false; h->rs_ran = false;
    if (reseg_wanted(flags, rows_out)) RCCHK(reseg_supported(h, flags));
    if (trunc_wanted(flags, rows_out)) RCCHK(trunc_supported(h));
    RCCHK(begin_call(h));
    const float *dsig; const int32_t *dlen;
    int rc = stage_inputs(h, signals, full_len, n, m, flags, &dsig, &dlen);
    if (rc) return rc;
    return llr_pipeline_t(h, SigF32{dsig}, dlen, n, m, minibatch, flags, rows_out, mb_status, upto);
}

extern "C" {

int adp_set_layout(adp_handle *h, int layout)
{
    if (!h || (layout != ADP_LAYOUT_MINIBATCH && layout != ADP_LAYOUT_SINGLE_READ)) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const int old = h->layout;
    h->layout = layout;
    int rc = geom(h);
    if (rc) { h->layout = old; (void)geom(h); }
    return rc;
}

int adp_detect_llr(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m, int minibatch, int flags,
                   adp_row *rows_out, int32_t *mb_status)
{
    return llr_pipeline(h, signals, full_len, n_reads, m, minibatch, flags, rows_out, mb_status, 8);
}

int adp_detect_llr_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset, int n_reads,
                       int m, int minibatch, int flags, adp_row *rows_out, int32_t *mb_status)
{
    if (!h || !raw || !full_len || !scale || !offset || n_reads < 1 || minibatch < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!(flags & ADP_IN_DEVICE)) { g_err = "adp_detect_llr_i16 takes device pointers (ADP_IN_DEVICE)"; return ADP_ERR_INVALID; }
    if (n_reads > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    if (h->layout == ADP_LAYOUT_SINGLE_READ) { g_err = "the single-read layout takes float32 input"; return ADP_ERR_UNSUPPORTED; }
    if (m & 3) { g_err = "int16 rows need m % 4 == 0 (8-byte aligned rows)"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_FLAG_TRUNCATED) { g_err = "ADP_FLAG_TRUNCATED takes float32 input (adp_calibrate_i16 + adp_detect_llr)"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_LLR_RESEGMENT) { g_err = "ADP_LLR_RESEGMENT takes float32 input (adp_calibrate_i16 + adp_detect_llr)"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_CNN_SECOND_RESEGMENT) { g_err = "ADP_CNN_SECOND_RESEGMENT goes with adp_detect_cnn and ADP_CNN_SECOND_LLR (the CNN primary)"; return ADP_ERR_UNSUPPORTED; }
    h->rs_ran = false;
    RCCHK(begin_call(h));
    // (samples at or beyond min(full_len, m) read as NaN: the padding is implied, so the passes always stop at a read's end)
    return llr_pipeline_t(h, SigI16{raw, scale, offset, full_len}, full_len, n_reads, m, minibatch, flags | ADP_TAILS_NAN, rows_out, mb_status, 8);
}

__global__ void k_debug_log(const double *in, double *out, int n)
{
    __shared__ __attribute__((aligned(16))) double lt_[3 * LOGCR_N];
    for (int i = threadIdx.x; i < 3 * LOGCR_N; i += blockDim.x) lt_[i] = g_logcr_table[i];
    __syncthreads();
    const LDS double *lt = (const LDS double *)lt_;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = log_cr_impl(in[i], lt, [](double u) { return log(u); });
}

int adp_debug_log(adp_handle *h, const double *host_in, double *host_out, int n)
{
    if (!h || !host_in || !host_out || n < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    double *d = nullptr;
    HIPCHK(hipMalloc(&d, (size_t)n * 16));
    HIPCHK(hipMemcpyAsync(d, host_in, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_debug_log, dim3((n + 255) / 256), dim3(256), 0, h->stream, d, d + n, n);
    HIPCHK(hipMemcpyAsync(host_out, d + n, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(d));
    return ADP_OK;
}

// fdiv_shared against the IEEE division for `count` consecutive float bit patterns from `first_bits` on (both signs)
__global__ void k_debug_divcheck(float d, uint32_t first_bits, uint32_t count, unsigned long long *mism)
{
    const float y = 1.0f / d;
    unsigned long long bad = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const float a = __uint_as_float(first_bits + i);
        if (a != a || __builtin_isinf(a)) continue;
        const float q = fdiv_shared(a, d, y), w = a / d;
        const float qn = fdiv_shared(-a, d, y), wn = -a / d;
        if (__float_as_uint(q) != __float_as_uint(w) || __float_as_uint(qn) != __float_as_uint(wn)) bad++;
    }
    if (bad) atomicAdd(mism, bad);
}

int adp_debug_divcheck(adp_handle *h, float d, uint32_t first_bits, uint32_t count, uint64_t *mismatches_out)
{
    if (!h || !mismatches_out) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    unsigned long long *dm = nullptr;
    HIPCHK(hipMalloc(&dm, 8));
    HIPCHK(hipMemsetAsync(dm, 0, 8, h->stream));
    hipLaunchKernelGGL(k_debug_divcheck, dim3(4096), dim3(256), 0, h->stream, d, first_bits, count, dm);
    HIPCHK(hipMemcpyAsync(mismatches_out, dm, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(dm));
    return ADP_OK;
}

int adp_debug_llr_upto(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m, int minibatch,
                       int flags, int stage)
{
    return llr_pipeline(h, signals, full_len, n_reads, m, minibatch, flags, nullptr, nullptr, stage);
}

int adp_detect_start_peak(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m, int minibatch,
                          int flags, adp_row *rows_out)
{
    if (!h || !signals || !full_len || n_reads < 1 || minibatch < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (n_reads > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    if (flags & ADP_FLAG_TRUNCATED) { g_err = "ADP_FLAG_TRUNCATED goes with adp_detect_llr and adp_detect_cnn"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_LLR_RESEGMENT) { g_err = "ADP_LLR_RESEGMENT goes with adp_detect_llr"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_CNN_SECOND_RESEGMENT) { g_err = "ADP_CNN_SECOND_RESEGMENT goes with adp_detect_cnn and ADP_CNN_SECOND_LLR (the CNN primary)"; return ADP_ERR_UNSUPPORTED; }
    RCCHK(begin_call(h));
    const float *dsig; const int32_t *dlen;
    int rc = stage_inputs(h, signals, full_len, n_reads, m, flags, &dsig, &dlen);
    if (rc) return rc;
    hipStream_t st = h->stream;
    rc = alloc_all(h, n_reads < minibatch ? n_reads : minibatch, false);
    if (rc) return rc;
    // the pandas float-column quirk couples the reads of ONE minibatch: process minibatch by minibatch (one arena for the
    // whole call: the offsets in the rows of every minibatch stay valid until the next call)
    return call_attempts(h, nullptr, 0, [&]() -> int {
        for (int s0 = 0; s0 < n_reads; s0 += minibatch) {
            int n = n_reads - s0 < minibatch ? n_reads - s0 : minibatch;
            const float *sg = dsig + (size_t)s0 * m;
            const int32_t *ln = dlen + s0;
            HIPCHK(hipMemsetAsync(h->any_none.p, 0, 4, st));
            { Scope s(h, "k_start_peak");
              hipLaunchKernelGGL(k_start_peak<SigF32>, dim3(n), dim3(64), (size_t)64 * h->cfg.sp_downscale_factor * 4, st, SigF32{sg}, ln, n, m, h->cfg, h->sp.as<SpOut>()); }
            hipLaunchKernelGGL(k_sp_bounds, dim3((n + 255) / 256), dim3(256), 0, st, h->sp.as<SpOut>(), n, h->bounds.as<int64_t>(),
                               h->topk_none.as<int8_t>(), h->any_none.as<int32_t>());
            RCCHK(launch_validate(h, SigF32{sg}, ln, n, m, 1, minibatch, false));
            hipLaunchKernelGGL(k_sp_decorate, dim3((n + 255) / 256), dim3(256), 0, st, h->sp.as<SpOut>(), h->rows.as<adp_row>(), n, 1,
                               h->any_none.as<int32_t>());
            if (rows_out) {
                HIPCHK(hipMemcpyAsync(rows_out + s0, h->rows.p, (size_t)n * sizeof(adp_row),
                                      (flags & ADP_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
            }
            HIPCHK(hipStreamSynchronize(st));
        }
        HIPCHK(hipGetLastError());
        return arena_end(h);
    });
}

// adp_validate_candidates and adp_validate_candidates_from: starts == nullptr -- every start is 0, k_validate<SigF32, false>
static int validate_candidates(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m, const int64_t *bounds,
                               const int64_t *starts, int k, int flags, adp_row *rows_out)
{
    if (!h || !signals || !full_len || !bounds || n_reads < 1 || k < 1 || k > ADP_MAX_CAND) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (n_reads > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    const bool truncated = (flags & ADP_POLYA_TRUNCATED) != 0;
    if (truncated && h->cfg.mvs_detect_check && h->cfg.mvs_detect_overwrite) { g_err = "ADP_POLYA_TRUNCATED does not go with mvs_detect_overwrite"; return ADP_ERR_UNSUPPORTED; }
    RCCHK(begin_call(h));
    const float *dsig; const int32_t *dlen;
    int rc = stage_inputs(h, signals, full_len, n_reads, m, flags, &dsig, &dlen);
    if (rc) return rc;
    hipStream_t st = h->stream;
    rc = alloc_all(h, n_reads, false);
    if (rc) return rc;
    ALLOCCHK(starts && h->bounds_stage.ensure((size_t)n_reads * 8)); // (the starts: nothing else of this call stages bounds)
    return call_attempts(h, nullptr, 0, [&]() -> int {
        const hipMemcpyKind kind = ((flags & ADP_IN_DEVICE) && !(flags & ADP_BOUNDS_HOST)) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIPCHK(hipMemcpyAsync(h->bounds.p, bounds, (size_t)n_reads * (1 + k) * 8, kind, st));
        if (starts) HIPCHK(hipMemcpyAsync(h->bounds_stage.p, starts, (size_t)n_reads * 8, kind, st));
        HIPCHK(hipMemsetAsync(h->topk_none.p, (flags & ADP_TOPK_NONE) ? 1 : 0, (size_t)n_reads, st));
        if (starts) RCCHK(launch_validate_t<true>(h, SigF32{dsig}, dlen, n_reads, m, k, n_reads, false, nullptr, truncated, h->bounds_stage.as<int64_t>()));
        else RCCHK(launch_validate(h, SigF32{dsig}, dlen, n_reads, m, k, n_reads, false, nullptr, truncated));
        RCCHK(deliver_rows(h, n_reads, flags, rows_out));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        return arena_end(h);
    });
}

int adp_validate_candidates(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m,
                            const int64_t *bounds, int k, int flags, adp_row *rows_out)
{
    return validate_candidates(h, signals, full_len, n_reads, m, bounds, nullptr, k, flags, rows_out);
}

int adp_validate_candidates_from(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m,
                                 const int64_t *bounds, const int64_t *starts, int k, int flags, adp_row *rows_out)
{
    return validate_candidates(h, signals, full_len, n_reads, m, bounds, starts, k, flags, rows_out);
}

} // extern "C"

// ---- the adapter's front boundary with its rows validated again (adapter_front_revalidate.h; the detector: modules.hip) ----
// One group of selected reads: gather, the validation from the trimmed starts over the rows where they lie, merge.
struct AfrBufs { Piece<int32_t> sel_a, sel_b, len_sub, reval; Piece<unsigned int> counts; Piece<int64_t> bounds, starts; Piece<int8_t> topk; Piece<adp_row> rows2; };
template <class SIG>
static int afr_group(adp_handle *h, SIG dsig, const int32_t *dlen, int m, const AfStaged &af, const AfrBufs &b, const int32_t *sel, int n_sel, bool truncated)
{
    const int kmax = truncated ? 1 : ADP_MAX_CAND;
    { Scope s(h, "k_afr_gather");
      hipLaunchKernelGGL(k_afr_gather, dim3((n_sel + 255) / 256), dim3(256), 0, h->stream, sel, n_sel, kmax, truncated ? 1 : 0, dlen, (const adp_row *)af.rows,
                         (const int64_t *)af.shift, b.len_sub.p, b.bounds.p, b.topk.p, b.starts.p); }
    const ValBufs vb{b.bounds.p, b.topk.p, b.rows2.p};
    RCCHK(launch_validate_t<true>(h, sig_subset(dsig, sel), b.len_sub.p, n_sel, m, kmax, n_sel, false, &vb, truncated, b.starts.p));
    { Scope s(h, "k_afr_merge");
      hipLaunchKernelGGL(k_afr_merge, dim3(n_sel), dim3(64), 0, h->stream, sel, n_sel, (const adp_row *)b.rows2.p, af.rows, b.reval.p); }
    HIPCHK(hipGetLastError());
    return 0;
}

// what the re-validating forms refuse beyond af_check, before anything is launched
static int afr_check(adp_handle *h, const int32_t *full_len, int n_reads, int m, const adp_adapter_front_args *args, int flags, const int32_t *reval_out)
{
    if (!full_len || !reval_out) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (args->min_adapter_len < 1) { g_err = "adp_adapter_front_revalidate: min_adapter_len must be >= 1 (an empty adapter slice has no median)"; return ADP_ERR_INVALID; }
    if (n_reads > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    if (h->cfg.mvs_detect_check && h->cfg.mvs_detect_overwrite) { g_err = "adp_adapter_front_revalidate does not go with mvs_detect_overwrite"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_OUT_DEVICE) { g_err = "adp_adapter_front_revalidate takes host rows (the call opens its own open-pore arena)"; return ADP_ERR_UNSUPPORTED; }
    return ADP_OK;
}

// dsig(af): the resident matrix once the detector has staged it
template <class MK>
static int afr_run(adp_handle *h, MK &&dsig_of, const float *sig, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset,
                   int n_reads, int m, adp_row *rows, const adp_adapter_front_args *args, int flags, int32_t *info_out, int64_t *shift_out,
                   int64_t *cand_out, double *diff_out, int32_t *reval_out)
{
    RCCHK(begin_call(h));
    hipStream_t st = h->stream;
    const int32_t *dlen = full_len;
    if (!(flags & ADP_IN_DEVICE)) {
        ALLOCCHK(h->len_stage.ensure((size_t)n_reads * 4));
        HIPCHK(hipMemcpyAsync(h->len_stage.p, full_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
        dlen = h->len_stage.as<int32_t>();
    }
    AfStaged af;
    RCCHK(af_detect_staged(h, sig, raw, dlen, scale, offset, n_reads, m, rows, args, flags, &af));
    RCCHK(alloc_all(h, n_reads, false));
    const size_t N = (size_t)n_reads;
    AfrBufs b;
    RCCHK(sub_carve(h, [&](Carve &c) {
        b.sel_a = c.take<int32_t>(N); b.sel_b = c.take<int32_t>(N); b.len_sub = c.take<int32_t>(N); b.reval = c.take<int32_t>(2 * N);
        b.counts = c.take<unsigned int>(4); b.bounds = c.take<int64_t>(N * (1 + ADP_MAX_CAND)); b.starts = c.take<int64_t>(N);
        b.topk = c.take<int8_t>(N); b.rows2 = c.take<adp_row>(N);
    }));
    const auto dsig = dsig_of(af);
    bool first = true;
    const int rc = call_attempts(h, nullptr, 0, [&]() -> int {
        // (a repeat on a larger arena starts from the rows as they came: the merge wrote into the staged copy)
        if (!first) HIPCHK(hipMemcpyAsync(af.rows, rows, N * sizeof(adp_row), hipMemcpyHostToDevice, st));
        first = false;
        { Scope s(h, "k_afr_select");
          hipLaunchKernelGGL(k_afr_select, dim3(1), dim3(SEL_THREADS), 0, st, (const int32_t *)af.info, (const adp_row *)af.rows, n_reads, b.sel_a.p, b.sel_b.p,
                             b.counts.p, b.reval.p); }
        unsigned int cnt[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(cnt, b.counts.p, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (cnt[0] > (unsigned int)n_reads || cnt[1] > (unsigned int)n_reads) { g_err = "adp_adapter_front_revalidate: selection count out of range"; return ADP_ERR_HIP; }
        if (cnt[0]) RCCHK(afr_group(h, dsig, dlen, m, af, b, b.sel_a.p, (int)cnt[0], false));
        if (cnt[1]) RCCHK(afr_group(h, dsig, dlen, m, af, b, b.sel_b.p, (int)cnt[1], true));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        return arena_end(h);
    });
    if (rc) return rc;
    // (behind the attempts: a repeat selects by the detector's acceptance column, which this overwrites with "replaced")
    hipLaunchKernelGGL(k_afr_info, dim3((n_reads + 255) / 256), dim3(256), 0, st, af.info, (const int32_t *)b.reval.p, n_reads);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rows, af.rows, N * sizeof(adp_row), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(reval_out, b.reval.p, N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(info_out, af.info, N * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(shift_out, af.shift, N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cand_out, af.cand, N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(diff_out, af.diff, N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ADP_OK;
}

extern "C" {

int adp_adapter_front_revalidate(adp_handle *h, const float *sig, const int32_t *full_len, int n_reads, int m, adp_row *rows,
                                 const adp_adapter_front_args *args, int flags, int32_t *info_out, int64_t *shift_out,
                                 int64_t *cand_out, double *diff_out, int32_t *reval_out)
{
    RCCHK(af_check(h, sig, n_reads, m, rows, args, info_out, shift_out, cand_out, diff_out));
    RCCHK(afr_check(h, full_len, n_reads, m, args, flags, reval_out));
    return afr_run(h, [](const AfStaged &af) { return SigF32{af.sig}; }, sig, nullptr, full_len, nullptr, nullptr, n_reads, m, rows, args, flags,
                   info_out, shift_out, cand_out, diff_out, reval_out);
}

int adp_adapter_front_revalidate_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale,
                                     const float *offset, int n_reads, int m, adp_row *rows, const adp_adapter_front_args *args,
                                     int flags, int32_t *info_out, int64_t *shift_out, int64_t *cand_out, double *diff_out,
                                     int32_t *reval_out)
{
    RCCHK(af_check(h, raw, n_reads, m, rows, args, info_out, shift_out, cand_out, diff_out));
    if (!full_len || !scale || !offset) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!(flags & ADP_IN_DEVICE)) { g_err = "adp_adapter_front_revalidate_i16 takes device pointers (ADP_IN_DEVICE)"; return ADP_ERR_INVALID; }
    if (m % 4 != 0) { g_err = "adp_adapter_front_revalidate_i16: m must be a multiple of 4"; return ADP_ERR_UNSUPPORTED; }
    RCCHK(afr_check(h, full_len, n_reads, m, args, flags, reval_out));
    return afr_run(h, [=](const AfStaged &) { return SigI16{raw, scale, offset, full_len}; }, nullptr, raw, full_len, scale, offset, n_reads, m, rows,
                   args, flags, info_out, shift_out, cand_out, diff_out, reval_out);
}

// C3 on the device: top-k behind given arg-maxes (dapos / dppos device int64 [n]) -> dcand / dcnt in ct_out (asynchronous)
static int cnn_topk_dev(adp_handle *h, const float *scores, const long long *dapos, const long long *dppos, int n, int mbsize, int Lo, int k)
{
    if ((long long)(mbsize < n ? mbsize : n) * Lo >= (1ll << 31)) { g_err = "minibatch * Lo too large for 32-bit flat positions"; return ADP_ERR_UNSUPPORTED; }
    const size_t half = (size_t)Lo / 2 + 1;
    const int wpr = (int)((half + 4 + 15) / 16 + 2);
    const size_t lds = (size_t)wpr * 4;
    if (lds > 60000) { g_err = "Lo too large for the LDS state of k_cnn_topk"; return ADP_ERR_UNSUPPORTED; }
    ALLOCCHK(h->ct_pk.ensure((size_t)n * 2 * half * 4) || h->ct_pv.ensure((size_t)n * half * 4) || h->ct_st.ensure((size_t)n * wpr * 4) ||
             h->ct_lnz.ensure((size_t)n * 4) || h->ct_out.ensure(((size_t)n * (k + 1) + 1) * 4));
    int32_t *dcand = h->ct_out.as<int32_t>(), *dcnt = dcand + (size_t)n * k;
    const int n_mb = (n + mbsize - 1) / mbsize;
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(k_cnn_rowlink, dim3(n_mb), dim3(1024), 0, st, dapos, dppos, n, mbsize, h->ct_lnz.as<int32_t>());
    { Scope s(h, "k_cnn_topk");
      hipLaunchKernelGGL(k_cnn_topk, dim3(n), dim3(64), lds, st, scores, dapos, dppos, h->ct_lnz.as<int32_t>(), n, mbsize, Lo, k,
                         h->ct_pk.as<int32_t>(), h->ct_pk.as<int32_t>() + (size_t)n * half, h->ct_pv.as<float>(), h->ct_st.as<uint32_t>(), wpr, dcand, dcnt); }
    return 0;
}

int adp_cnn_topk(adp_handle *h, const float *scores_dev, const int64_t *adapter_pos_dev, const int64_t *polya_pos_dev,
                 int n_reads, int Lo, int k, int32_t *cand_out, int32_t *n_peaks_out)
{
    if (!h || !scores_dev || !adapter_pos_dev || !polya_pos_dev || !cand_out || !n_peaks_out || n_reads < 1 || Lo < 3 ||
        k < 1 || k > ADP_MAX_CAND) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    int rc = cnn_topk_dev(h, scores_dev, (const long long *)adapter_pos_dev, (const long long *)polya_pos_dev, n_reads, n_reads, Lo, k);
    if (rc) return rc;
    hipStream_t st = h->stream;
    int32_t *dcand = h->ct_out.as<int32_t>(), *dcnt = dcand + (size_t)n_reads * k;
    HIPCHK(hipMemcpyAsync(cand_out, dcand, (size_t)n_reads * k * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(n_peaks_out, dcnt, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return ADP_OK;
}

// cnn_predict + the scaling of cnn_detect: scores (device) -> h->bounds [n, 1 + max(k, 1)] (asynchronous)
static int cnn_predict_dev(adp_handle *h, const float *scores, int n, int mbsize, int Lo, int *kmax_out)
{
    const adp_cfg &c = h->cfg;
    const int k = c.polya_cand_k, kk = k < 1 ? 1 : k;
    if (k > ADP_MAX_CAND) { g_err = "polya_cand_k too large"; return ADP_ERR_UNSUPPORTED; }
    if (n > h->max_reads) { g_err = "n_reads exceeds the handle's capacity"; return ADP_ERR_CAPACITY; }
    ALLOCCHK(h->ct_ap.ensure((size_t)n * 16) || h->bounds.ensure((size_t)n * (1 + ADP_MAX_CAND) * 8));
    long long *dap = h->ct_ap.as<long long>(), *dpp = dap + n;
    const int na = (c.max_obs_adapter - c.min_obs_adapter) / c.downscale_factor;
    hipStream_t st = h->stream;
    { Scope s(h, "k_cnn_argmax");
      hipLaunchKernelGGL(k_cnn_argmax, dim3(n), dim3(64), 0, st, scores, n, Lo, na, k, dap, dpp); }
    const int32_t *dcand = nullptr, *dcnt = nullptr;
    if (k > 1) {
        int rc = cnn_topk_dev(h, scores, dap, dpp, n, mbsize, Lo, k);
        if (rc) return rc;
        dcand = h->ct_out.as<int32_t>(); dcnt = dcand + (size_t)n * k;
    }
    const int n_mb = (n + mbsize - 1) / mbsize;
    hipLaunchKernelGGL(k_cnn_bounds, dim3(n_mb), dim3(1024), 0, st, dap, dpp, dcand, dcnt, n, mbsize, k, c.downscale_factor, c.min_obs_adapter,
                       h->bounds.as<int64_t>());
    *kmax_out = kk;
    return 0;
}

int adp_cnn_predict(adp_handle *h, const float *scores_dev, int n_reads, int minibatch, int Lo, int64_t *bounds_out)
{
    if (!h || !scores_dev || !bounds_out || n_reads < 1 || minibatch < 1 || Lo < 3) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    int kk = 1;
    int rc = cnn_predict_dev(h, scores_dev, n_reads, minibatch, Lo, &kk);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(bounds_out, h->bounds.p, (size_t)n_reads * (1 + kk) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// C1 on the handle's stream: pooled values (k_cnn_pool), then their per-read median / MAD scaling in place (k_cnn_prepare).
// sp_head (the fused start-peak scan of a detect call, else null): k_sp_head's state of these reads, which K1 riding the pooling
// pass (k_cnn_pool<SIG, true>) completes for k_sp_tail
extern "C++" {
template <class SIG>
static int launch_cnn_prepare(adp_handle *h, SIG dsig, int n_reads, int m, int off, int ds, int Lc, float *dout, SpHead *sp_head = nullptr)
{
    ALLOCCHK(h->npk.ensure((size_t)n_reads * 4)); // (npk: unused on this path)
    int32_t *nan_cnt = h->npk.as<int32_t>();
    HIPCHK(hipMemsetAsync(nan_cnt, 0, (size_t)n_reads * 4, h->stream));
    { Scope s(h, "k_cnn_pool");
      if (sp_head)
          hipLaunchKernelGGL((k_cnn_pool<SIG, true>), dim3(n_reads), dim3(256), (size_t)4 * 64 * ds * 4, h->stream, dsig, n_reads, m, off, ds, Lc, dout, nan_cnt,
                             sp_head, (float)h->cfg.open_pore_pa);
      else
          hipLaunchKernelGGL((k_cnn_pool<SIG, false>), dim3(n_reads), dim3(256), (size_t)4 * 64 * ds * 4, h->stream, dsig, n_reads, m, off, ds, Lc, dout, nan_cnt); }
    { Scope s(h, "k_cnn_prepare");
      hipLaunchKernelGGL(k_cnn_prepare, dim3(n_reads), dim3(64), 0, h->stream, n_reads, Lc, dout, (const int32_t *)nan_cnt); }
    return 0;
}
} // extern "C++"

int adp_cnn_prepare(adp_handle *h, const float *signals, int n_reads, int m, int flags, float *prepared_out)
{
    if (!h || !signals || !prepared_out || n_reads < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (m != h->m) { g_err = "m differs from the handle's"; return ADP_ERR_CAPACITY; }
    RCCHK(begin_call(h));
    const int off = h->cfg.min_obs_adapter, ds = h->cfg.downscale_factor;
    if (m <= off) { g_err = "preload shorter than min_obs_adapter"; return ADP_ERR_INVALID; }
    const int Lc = (m - off + ds - 1) / ds;
    const float *dsig = signals;
    if (!(flags & ADP_IN_DEVICE)) {
        if (h->sig_stage.ensure((size_t)n_reads * m * 4)) { g_err = "staging allocation failed"; return ADP_ERR_HIP; }
        HIPCHK(hipMemcpyAsync(h->sig_stage.p, signals, (size_t)n_reads * m * 4, hipMemcpyHostToDevice, h->stream));
        dsig = h->sig_stage.as<float>();
    }
    float *dout = prepared_out;
    if (!(flags & ADP_OUT_DEVICE)) {
        if (h->bounds_stage.ensure((size_t)n_reads * Lc * 4)) { g_err = "staging allocation failed"; return ADP_ERR_HIP; }
        dout = h->bounds_stage.as<float>();
    }
    { int rc2 = launch_cnn_prepare(h, SigF32{dsig}, n_reads, m, off, ds, Lc, dout); if (rc2) return rc2; }
    if (!(flags & ADP_OUT_DEVICE))
        HIPCHK(hipMemcpyAsync(prepared_out, dout, (size_t)n_reads * Lc * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// offsets (floats) of the layers inside the weight buffer: w0 [64][1][7], b0 [64], w1 [64][64][7], b1 [64], w2, b2, w3 [64][2][7], b3 [2]
#define CNN_W0 0
#define CNN_B0 (CNN_W0 + CNN_C * CNN_K)
#define CNN_W1 (CNN_B0 + CNN_C)
#define CNN_B1 (CNN_W1 + CNN_C * CNN_C * CNN_K)
#define CNN_W2 (CNN_B1 + CNN_C)
#define CNN_B2 (CNN_W2 + CNN_C * CNN_C * CNN_K)
#define CNN_W3 (CNN_B2 + CNN_C)
#define CNN_B3 (CNN_W3 + CNN_C * 2 * CNN_K)
#define CNN_WTOTAL (CNN_B3 + 2)

int adp_cnn_set_weights(adp_handle *h, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                        const float *b2, const float *w3, const float *b3)
{
    if (!h || !w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    ALLOCCHK(h->cnn_w.ensure((size_t)CNN_WTOTAL * 4));
    std::vector<float> all((size_t)CNN_WTOTAL);
    memcpy(&all[CNN_W0], w0, sizeof(float) * CNN_C * CNN_K); memcpy(&all[CNN_B0], b0, sizeof(float) * CNN_C);
    memcpy(&all[CNN_W1], w1, sizeof(float) * CNN_C * CNN_C * CNN_K); memcpy(&all[CNN_B1], b1, sizeof(float) * CNN_C);
    memcpy(&all[CNN_W2], w2, sizeof(float) * CNN_C * CNN_C * CNN_K); memcpy(&all[CNN_B2], b2, sizeof(float) * CNN_C);
    memcpy(&all[CNN_W3], w3, sizeof(float) * CNN_C * 2 * CNN_K); memcpy(&all[CNN_B3], b3, sizeof(float) * 2);
    HIPCHK(hipMemcpyAsync(h->cnn_w.p, all.data(), (size_t)CNN_WTOTAL * 4, hipMemcpyHostToDevice, h->stream));
    // the 64 -> 64 layers once more as split float16 B fragments (cnn_conv_split.h), scaled by a power of two per layer so that the
    // largest weight lands in [2^13, 2^14)
    ALLOCCHK(h->cnn_wsp.ensure(((size_t)2 * CNS_WSP_LAYER + CNS_W3SP + CNS_W0SP) * 2));
    for (int layer = 0; layer < 2; layer++) {
        const float *wl = &all[layer ? CNN_W2 : CNN_W1];
        float mx = 0.f;
        for (int i = 0; i < CNN_C * CNN_C * CNN_K; i++) { const float a = fabsf(wl[i]); if (a > mx && a < INFINITY) mx = a; }
        int e = 0;
        if (mx > 0.f) (void)frexpf(mx, &e); // mx = f 2^e, f in [0.5, 1)
        int se = 14 - e;
        if (se > 100) se = 100;
        if (se < -100) se = -100;
        h->cnn_sw[layer] = ldexpf(1.0f, se);
        hipLaunchKernelGGL(k_cns_split_weights, dim3((2 * CNS_KSTEPS * 64 + 255) / 256), dim3(256), 0, h->stream,
                           h->cnn_w.as<float>() + (layer ? CNN_W2 : CNN_W1), h->cnn_sw[layer], h->cnn_wsp.as<_Float16>() + (size_t)layer * CNS_WSP_LAYER);
    }
    { // layer 3 as A fragments of one more GEMM in layer 2's kernel (k_cns_split_w3), scaled like the others
        float mx = 0.f;
        for (int i = 0; i < CNN_C * 2 * CNN_K; i++) { const float a = fabsf(w3[i]); if (a > mx && a < INFINITY) mx = a; }
        int e = 0;
        if (mx > 0.f) (void)frexpf(mx, &e);
        int se = 14 - e;
        if (se > 100) se = 100;
        if (se < -100) se = -100;
        h->cnn_sw[2] = ldexpf(1.0f, se);
        hipLaunchKernelGGL(k_cns_split_w3, dim3(1), dim3(256), 0, h->stream, h->cnn_w.as<float>() + CNN_W3, h->cnn_sw[2], h->cnn_wsp.as<_Float16>() + (size_t)2 * CNS_WSP_LAYER);
    }
    { // layer 0 as A fragments of a small GEMM in layer 1's prologue (k_cns_split_w0)
        float mx = 0.f;
        for (int i = 0; i < CNN_C * CNN_K; i++) { const float a = fabsf(w0[i]); if (a > mx && a < INFINITY) mx = a; }
        int e = 0;
        if (mx > 0.f) (void)frexpf(mx, &e);
        int se = 14 - e;
        if (se > 100) se = 100;
        if (se < -100) se = -100;
        h->cnn_sw[3] = ldexpf(1.0f, se);
        hipLaunchKernelGGL(k_cns_split_w0, dim3(1), dim3(128), 0, h->stream, h->cnn_w.as<float>() + CNN_W0, h->cnn_sw[3],
                           h->cnn_wsp.as<_Float16>() + (size_t)2 * CNS_WSP_LAYER + CNS_W3SP);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cnn_have_w = true;
    return ADP_OK;
}

extern "C++" {
template <int NT>
static int launch_conv64(adp_handle *h, const float *in, float *out, const float *w, const float *b, int n, int L1, int Lpad, int tiles)
{
    const size_t lds = (size_t)2 * CNN_C * (64 * NT + 8) * 4;
    RCCHK(lds_attr_once(h, (const void *)k_cnn_conv64<NT>, lds));
    long long total = (long long)n * tiles;
    int grid = (int)(total < h->n_cu ? total : h->n_cu);
    hipLaunchKernelGGL(k_cnn_conv64<NT>, dim3(grid), dim3(256), lds, h->stream, in, out, w, b, n, L1, Lpad, tiles);
    return 0;
}
} // extern "C++"

extern "C++" {
// k_cnn_conv64s in one of its two roles: the LDS size and the persistent grid they share.  The arguments behind `flag` are LAST's (layer 3's
// fragments, bias and scale, the scores), `first` is FIRST's; each launcher below passes nothing for the other role's.
template <int NT, bool LAST>
static int launch_conv64s(adp_handle *h, const _Float16 *in, _Float16 *out, const _Float16 *wsp, const float *b, float sw, int n, int L1,
                          int Lrows, int tiles, int32_t *flag, const _Float16 *w3sp, const float *b3, float inv_s3, float *scores, int Lo,
                          CnsFirst first)
{
    // (LAST: layer 3 in the epilogue -- tiles that advance by 64 NT - 2 positions, the taps' partial sums of a tile in LDS behind the two tile buffers)
    const size_t lds = (size_t)2 * (((size_t)(64 * NT + 6) * CNS_ROWB + 1023) / 1024 * 1024) + (LAST ? (size_t)2 * CNN_K * 64 * NT * 4 : 0);
    RCCHK(lds_attr_once(h, (const void *)k_cnn_conv64s<NT, LAST>, lds));
    long long total = (long long)n * tiles;
    if (total >= (1ll << 31)) { g_err = "too many tiles for one launch of k_cnn_conv64s"; return ADP_ERR_UNSUPPORTED; }
    int grid = (int)(total < h->n_cu ? total : h->n_cu);
    hipLaunchKernelGGL((k_cnn_conv64s<NT, LAST>), dim3(grid), dim3(256), lds, h->stream, in, out, wsp, b, sw, 1.0f / sw, n, L1, Lrows, tiles, flag,
                       w3sp, b3, inv_s3, scores, Lo, first);
    return 0;
}
// The split stack's kernels over the n reads of a chunk, each launcher with the arguments of its role (wh: the handle that owns the weights).
// Layers 0 + 1: the prepared signal x in, layer 1's rows out; tiles that advance by 64 NT - 6 positions
template <int NT>
static int launch_conv_first(adp_handle *h, adp_handle *wh, const float *x, int Lc, _Float16 *rows, int n, int L1, int Lrows, int32_t *flag)
{
    Scope s(h, "k_cnn_conv64 (layer 1)");
    const _Float16 *wsp = wh->cnn_wsp.as<_Float16>();
    const float *W = wh->cnn_w.as<float>();
    const CnsFirst first{x, Lc, wsp + (size_t)2 * CNS_WSP_LAYER + CNS_W3SP, W + CNN_B0, wh->cnn_sw[3]};
    return launch_conv64s<NT, false>(h, nullptr, rows, wsp, W + CNN_B1, wh->cnn_sw[0], n, L1, Lrows, (L1 + 64 * NT - 7) / (64 * NT - 6), flag,
                                     nullptr, nullptr, 0.f, nullptr, 0, first);
}
// Layers 2 + 3: layer 1's rows in, the scores out (`dump`: one row for the stores that have no output); tiles that advance by 64 NT - 2
template <int NT>
static int launch_conv_last(adp_handle *h, adp_handle *wh, const _Float16 *rows, _Float16 *dump, float *scores, int Lo, int n, int L1, int Lrows,
                            int32_t *flag)
{
    Scope s(h, "k_cnn_conv64 (layer 2)");
    const _Float16 *wsp = wh->cnn_wsp.as<_Float16>();
    const float *W = wh->cnn_w.as<float>();
    return launch_conv64s<NT, true>(h, rows, dump, wsp + CNS_WSP_LAYER, W + CNN_B2, wh->cnn_sw[1], n, L1, Lrows, (L1 + 64 * NT - 3) / (64 * NT - 2), flag,
                                    wsp + (size_t)2 * CNS_WSP_LAYER, W + CNN_B3, 1.0f / (wh->cnn_sw[2] * CNS_ASCALE), scores, Lo, CnsFirst{});
}
// the chunks of a call: layers 0 + 1, then layers 2 + 3
template <int NT>
static int conv_split_chunks(adp_handle *h, adp_handle *wh, const float *prepared, int n_reads, int C, int Lc, int L1, int Lo, int Lrows,
                             _Float16 *rows, _Float16 *dump, int32_t *flag, float *scores_out)
{
    for (int s0 = 0; s0 < n_reads; s0 += C) {
        const int n = n_reads - s0 < C ? n_reads - s0 : C;
        RCCHK(launch_conv_first<NT>(h, wh, prepared + (size_t)s0 * Lc, Lc, rows, n, L1, Lrows, flag));
        RCCHK(launch_conv_last<NT>(h, wh, rows, dump, scores_out + (size_t)s0 * 2 * Lo, Lo, n, L1, Lrows, flag));
    }
    return 0;
}
} // extern "C++"

// the conv stack on split float16 operands (cnn_conv_split.h); the out-of-range flag is the second word of the call's arena counter
static int cnn_forward_split(adp_handle *h, adp_handle *wh, const float *prepared, int n_reads, int Lc, int L1, int Lo, int NT, float *scores_out)
{
    const int PB = 64 * NT, tiles = (L1 + PB - 1) / PB, Lrows = CNS_FRONT + tiles * PB + 4;
    const size_t per_read = (size_t)Lrows * CNS_ROWB;
    size_t cap_reads = ((size_t)4 << 30) / per_read; // an activation buffer of at most 4 GiB
    if (cap_reads < 1) cap_reads = 1;
    if (cap_reads > 65535) cap_reads = 65535;        // (the grid.y limit of layer 0's retired kernel, here and below; kept so that the chunks keep the shapes they had)
    int C = (int)((size_t)n_reads < cap_reads ? (size_t)n_reads : cap_reads);
    // cnn_rows: layer 1's rows, the only activations in HBM
    if (h->cnn_Lpad != Lrows || h->cnn_L1 != L1 || h->cnn_chunk < C) {
        ALLOCCHK(h->cnn_rows.ensure((size_t)C * per_read + CNS_SLACK)); // (+ what the tile DMAs read past the last read's rows)
        HIPCHK(hipMemsetAsync(h->cnn_rows.p, 0, h->cnn_rows.cap, h->stream)); // the padding rows are never written again
        h->cnn_Lpad = Lrows; h->cnn_L1 = L1; h->cnn_chunk = (int)((h->cnn_rows.cap - CNS_SLACK) / per_read); if (h->cnn_chunk > 65535) h->cnn_chunk = 65535;
    }
    C = h->cnn_chunk < n_reads ? h->cnn_chunk : n_reads;
    ALLOCCHK(h->cnn_dump.ensure(CNS_ROWB)); // written by the LAST kernel's stores without an output, never read: no clearing
    ALLOCCHK(wh->op_used.ensure(16));
    int32_t *flag = wh->op_used.as<int32_t>() + 1;
    _Float16 *rows = h->cnn_rows.as<_Float16>(), *dump = h->cnn_dump.as<_Float16>();
    return NT == 4 ? conv_split_chunks<4>(h, wh, prepared, n_reads, C, Lc, L1, Lo, Lrows, rows, dump, flag, scores_out)
         : NT == 3 ? conv_split_chunks<3>(h, wh, prepared, n_reads, C, Lc, L1, Lo, Lrows, rows, dump, flag, scores_out)
                   : conv_split_chunks<2>(h, wh, prepared, n_reads, C, Lc, L1, Lo, Lrows, rows, dump, flag, scores_out);
}

// the conv stack over device buffers, asynchronous on the handle's stream
static int cnn_forward_dev(adp_handle *h, const float *prepared, int n_reads, int Lc, float *scores_out)
{
    adp_handle *wh = h->owner ? h->owner : h; // (a lane runs with its parent's weights)
    if (!wh->cnn_have_w) { g_err = "adp_cnn_set_weights has not been called"; return ADP_ERR_INVALID; }
    const int L1 = (Lc + 2 * 3 - CNN_K) / 3 + 1, Lo = (L1 - 1) * 3 - 2 * 3 + CNN_K;
    // positions per workgroup step: the NT (32-position tiles per wave) that wastes least of the last step
    int NT = 4; { long long best = -1; for (int nt = 4; nt >= 2; nt--) { const long long pb = 64 * nt, cover = (L1 + pb - 1) / pb * pb; if (best < 0 || cover < best) { best = cover; NT = nt; } } }
    if (wh->cnn_mode == 1 && !wh->cnn_redo_f32) return cnn_forward_split(h, wh, prepared, n_reads, Lc, L1, Lo, NT, scores_out);
    const int PB = 64 * NT, tiles = (L1 + PB - 1) / PB, Lpad = tiles * PB + 8;
    size_t per_read = (size_t)CNN_C * Lpad * 4;
    size_t cap_reads = ((size_t)4 << 30) / per_read; // two activation buffers of at most 4 GiB each
    if (cap_reads < 1) cap_reads = 1;
    if (cap_reads > 65535) cap_reads = 65535;        // (the first / last layer's kernels take the chunk's reads as grid.y)
    int C = (int)((size_t)n_reads < cap_reads ? (size_t)n_reads : cap_reads);
    // (buffers of its own: a call that falls back from the split stack -- an activation beyond the float16 range -- and the split
    // call after it used to share one pair and cleared up to 2 x 4 GiB of padding on every change of kind)
    if (h->cnn_f_Lpad != Lpad || h->cnn_f_L1 != L1 || h->cnn_f_chunk < C) {
        for (int k = 0; k < 2; k++) {
            ALLOCCHK(h->cnn_actf[k].ensure((size_t)C * per_read));
            HIPCHK(hipMemsetAsync(h->cnn_actf[k].p, 0, h->cnn_actf[k].cap, h->stream)); // the padding columns are never written again
        }
        h->cnn_f_Lpad = Lpad; h->cnn_f_L1 = L1; h->cnn_f_chunk = (int)(h->cnn_actf[0].cap / per_read); if (h->cnn_f_chunk > 65535) h->cnn_f_chunk = 65535;
    }
    C = h->cnn_f_chunk < n_reads ? h->cnn_f_chunk : n_reads;
    const float *W = wh->cnn_w.as<float>();
    float *A = h->cnn_actf[0].as<float>(), *B = h->cnn_actf[1].as<float>();
    for (int s0 = 0; s0 < n_reads; s0 += C) {
        const int n = n_reads - s0 < C ? n_reads - s0 : C;
        const float *x = prepared + (size_t)s0 * Lc;
        float *sc = scores_out + (size_t)s0 * 2 * Lo;
        { Scope s(h, "k_cnn_conv_in");
          hipLaunchKernelGGL(k_cnn_conv_in, dim3((L1 + 255) / 256, n), dim3(256), 0, h->stream, x, Lc, L1, Lpad, W + CNN_W0, W + CNN_B0, A); }
        for (int layer = 0; layer < 2; layer++) {
            Scope s(h, layer ? "k_cnn_conv64 (layer 2)" : "k_cnn_conv64 (layer 1)");
            const float *in = layer ? B : A; float *out = layer ? A : B;
            const float *w = W + (layer ? CNN_W2 : CNN_W1), *b = W + (layer ? CNN_B2 : CNN_B1);
            int rc = NT == 4 ? launch_conv64<4>(h, in, out, w, b, n, L1, Lpad, tiles)
                   : NT == 3 ? launch_conv64<3>(h, in, out, w, b, n, L1, Lpad, tiles)
                             : launch_conv64<2>(h, in, out, w, b, n, L1, Lpad, tiles);
            if (rc) return rc;
        }
        { Scope s(h, "k_cnn_conv_out");
          hipLaunchKernelGGL(k_cnn_conv_out, dim3((L1 + 255) / 256, n), dim3(256), 0, h->stream, A, L1, Lpad, Lo, W + CNN_W3, W + CNN_B3, sc); }
    }
    return 0;
}

int adp_cnn_forward(adp_handle *h, const float *prepared, int n_reads, int Lc, float *scores_out)
{
    if (!h || !prepared || !scores_out || n_reads < 1 || Lc < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    RCCHK(begin_call(h));
    h->cnn_redo_f32 = false;
    for (int attempt = 0; attempt < 2; attempt++) {
        ALLOCCHK(h->op_used.ensure(16));
        HIPCHK(hipMemsetAsync(h->op_used.as<int32_t>() + 1, 0, 4, h->stream));
        int rc = cnn_forward_dev(h, prepared, n_reads, Lc, scores_out);
        if (rc) return rc;
        HIPCHK(hipGetLastError());
        int32_t flag = 0;
        if (h->cnn_mode == 1 && !h->cnn_redo_f32) HIPCHK(hipMemcpyAsync(&flag, h->op_used.as<int32_t>() + 1, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (!flag) break;
        h->cnn_redo_f32 = true; // an activation left the float16 range: once more on the float32 kernels
        drop_profile(h);
    }
    return ADP_OK;
}

// combined_detect_cnn up to (not including) the short-read fallback: C1 prepare -> C2 conv stack -> C3 predict -> V1 with the
// k candidates, enqueued on the handle's stream without waiting for anything on the host.  bounds_dst (may be NULL): int64
// [n, 1 + max(k, 1)] what cnn_detect returns, copied with bounds_kind.
// the start-peak overlay of the CNN path (ADP_WITH_START_PEAK): can K1 ride the pooling pass?
// (from here to adp_detect_cnn: templates on the matrix type -- SigF32 for adp_detect_cnn, SigI16 for adp_detect_cnn_i16)
extern "C++" {
static bool cnn_sp_fused(const adp_handle *h)
{
    const adp_cfg &c = h->cfg;
    return c.sp_downscale_factor == c.downscale_factor && c.min_obs_adapter % c.downscale_factor == 0 && env_int("ADP_SP_FUSED", 1) != 0;
}
static void cnn_sp_decorate(adp_handle *h, const SpOut *sp, adp_row *rows, int n)
{
    hipLaunchKernelGGL(k_sp_decorate, dim3((n + 255) / 256), dim3(256), 0, h->stream, sp, rows, n, 0, (const int32_t *)nullptr);
}
// sp_out (ADP_WITH_START_PEAK, else null): K1's results of these reads -- a slice of the CALL's buffer, the owner handle's, because
// the phases behind the first pass run there -- are computed beside the pass and overlaid on its rows (k_sp_decorate, mode 0).
template <class SIG>
static int cnn_enqueue(adp_handle *h, SIG dsig, const int32_t *dlen, int n_reads, int m, int minibatch, adp_row *rows_dst,
                       int rows_kind, int64_t *bounds_dst, int bounds_kind, SpOut *sp_out = nullptr)
{
    const int off = h->cfg.min_obs_adapter, ds = h->cfg.downscale_factor;
    const int Lc = (m - off + ds - 1) / ds, L1 = (Lc - 1) / 3 + 1, Lo = 3 * L1 - 2;
    ALLOCCHK(h->cnn_x.ensure((size_t)n_reads * Lc * 4) || h->cnn_sc.ensure((size_t)n_reads * 2 * Lo * 4));
    hipStream_t st = h->stream;
    int rc = alloc_all(h, n_reads, false);
    if (rc) return rc;
    // K1 riding the pooling pass (k_cnn_pool<SIG, true>): when both pooling factors agree and min_obs_adapter is a multiple of them the
    // start-peak scan costs no sweep of its own; else, and with ADP_SP_FUSED=0, the separate k_start_peak streams the signal on the
    // side stream beside the conv stack (matrix cores, little HBM traffic)
    const size_t sp_lds = (size_t)64 * h->cfg.sp_downscale_factor * 4;
    const bool sp_fused = sp_out && cnn_sp_fused(h);
    SpHead *sp_head = nullptr;
    if (sp_fused) {
        ALLOCCHK(h->sphead.ensure((size_t)n_reads * sizeof(SpHead)));
        sp_head = h->sphead.as<SpHead>();
        Scope s(h, "k_sp_head");
        hipLaunchKernelGGL(k_sp_head<SIG>, dim3(n_reads), dim3(64), sp_lds, st, dsig, dlen, n_reads, m, h->cfg, off, sp_head);
    }
    rc = launch_cnn_prepare(h, dsig, n_reads, m, off, ds, Lc, h->cnn_x.as<float>(), sp_head);
    if (rc) return rc;
    if (sp_fused) {
        const int cov0 = off / ds, cov1 = cov0 + (m - off) / ds;
        Scope s(h, "k_sp_tail");
        hipLaunchKernelGGL(k_sp_tail<SIG>, dim3(n_reads), dim3(64), sp_lds, st, dsig, dlen, n_reads, m, h->cfg, cov0, cov1, (const SpHead *)sp_head, sp_out);
    } else if (sp_out) {
        HIPCHK(hipEventRecord(h->ev_fork, st)); // (the signal is staged on this stream)
        HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        { Scope s(h, "k_start_peak", h->stream2);
          hipLaunchKernelGGL(k_start_peak<SIG>, dim3(n_reads), dim3(64), sp_lds, h->stream2, dsig, dlen, n_reads, m, h->cfg, sp_out); }
        HIPCHK(hipEventRecord(h->ev_join, h->stream2));
    }
    // (from here on an error return must not leave the side stream's scan running into the caller's next use of sp_out)
    struct SpJoin { hipStream_t side; bool armed; ~SpJoin() { if (armed) (void)hipStreamSynchronize(side); } } sp_join{h->stream2, sp_out && !sp_fused};
    rc = cnn_forward_dev(h, h->cnn_x.as<float>(), n_reads, Lc, h->cnn_sc.as<float>());
    if (rc) return rc;
    int kk = 1;
    rc = cnn_predict_dev(h, h->cnn_sc.as<float>(), n_reads, minibatch, Lo, &kk);
    if (rc) return rc;
    if (bounds_dst) HIPCHK(hipMemcpyAsync(bounds_dst, h->bounds.p, (size_t)n_reads * (1 + kk) * 8, (hipMemcpyKind)bounds_kind, st));
    HIPCHK(hipMemsetAsync(h->topk_none.p, 0, (size_t)n_reads, st));
    rc = launch_validate(h, dsig, dlen, n_reads, m, kk, n_reads, false);
    if (rc) return rc;
    if (sp_out) {
        if (!sp_fused) { HIPCHK(hipStreamWaitEvent(st, h->ev_join, 0)); sp_join.armed = false; }
        cnn_sp_decorate(h, sp_out, h->rows.as<adp_row>(), n_reads);
    }
    if (rows_dst) HIPCHK(hipMemcpyAsync(rows_dst, h->rows.p, (size_t)n_reads * sizeof(adp_row), (hipMemcpyKind)rows_kind, st));
    HIPCHK(hipGetLastError());
    return ADP_OK;
}

extern "C++" {
__global__ void k_refine_out(const MbState *mbs, const int32_t *nvalid, const int32_t *polya_idx, const int64_t *ranges, int n,
                             int ds, int64_t *out, int32_t *status)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int st = 0;
    if (mbs[r].status == ADP_MB_MAD_ZERO) st = ADP_F_EXC_MAD_ZERO;
    else if (nvalid[r] <= 0) st = ADP_F_EXC_EMPTY_TRACE;
    int p = polya_idx[r];
    out[r] = (st == 0 && p > 0) ? (int64_t)p * ds + ranges[2 * r] : 0;
    status[r] = st;
}

// The fallback's chain (combined.py:258-301) over n reads, enqueued on the handle's stream (alloc_all(h, n, true) done): per-read
// normalisation, the LLR trace (offsets 5/5) over [drng[2r], drng[2r+1]) and P4 on it -> dout[r] the new poly(A) end in samples or 0,
// dstat[r] 0 or the ADP_F_EXC_* code of the exception the reference raises.  dlen, drng, dout, dstat: device arrays over the n reads.
template <class SIG>
static int refine_chain(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, const int64_t *drng, int64_t *dout, int32_t *dstat)
{
    hipStream_t st = h->stream;
    ALLOCCHK(h->mbs.ensure((size_t)n * sizeof(MbState)) || h->ghist.ensure((size_t)n * N1_BINS * 4) || h->gbelow.ensure((size_t)n * 8) || h->gcnt.ensure((size_t)n * 8 * N1_NCNT));
    MbState *mbs = h->mbs.as<MbState>();
    HIPCHK(hipMemsetAsync(mbs, 0, (size_t)n * sizeof(MbState), st));
    HIPCHK(hipMemsetAsync(h->ghist.p, 0, (size_t)n * N1_BINS * 4, st));
    HIPCHK(hipMemsetAsync(h->gbelow.p, 0, (size_t)n * 8, st));
    HIPCHK(hipMemsetAsync(h->adapter_idx.p, 0, (size_t)n * 4, st));
    HIPCHK(hipMemsetAsync(h->gcnt.p, 0, (size_t)n * 8 * N1_NCNT, st));
    { Scope s(h, "k_n1 (refine)");
      int rc = launch_n1(h, dsig, n, m, h->T, 1, n, false); // per-read normalisation: every read is its own minibatch
      if (rc) return rc; }
    { Scope s(h, "k_norm_pool (refine)");
      hipLaunchKernelGGL(k_norm_pool<SIG>, dim3(n), dim3(256), (size_t)NP_TILE * h->ds * 4, st, dsig, m, h->T, h->off, h->ds, h->L, h->Lp, 1, mbs,
                         h->down.as<float>(), h->nvalid.as<int32_t>(), drng, dlen); }
    { Scope s(h, "k_gains (refine)");
      launch_cumsum(h, n);
      hipLaunchKernelGGL(k_gains<1>, dim3((n + GAINS_WPB - 1) / GAINS_WPB), dim3(64 * GAINS_WPB), 0, st, h->down.as<float>(), h->nvalid.as<int32_t>(), h->Lp, h->nck,
                         h->ck.as<double2>(), h->tail.as<double2>(), h->adapter_idx.as<int32_t>(), 1, mbs, h->trace.as<double>(),
                         h->bmax.as<double>(), h->bmin.as<double>(), h->nsum, h->t1.as<int2>(), 1, h->pk.as<int32_t>(), h->npk.as<int32_t>(), h->Lp / 2 + 1, (double *)nullptr, n, 5, nullptr, gains_tile_fast()); }
    { Scope s(h, "k_polya_peak (refine)");
      launch_polya_peak(h, n, 1, nullptr); // (k_gains<1> lists no heights)
      hipLaunchKernelGGL(k_refine_out, dim3((n + 255) / 256), dim3(256), 0, st, mbs, h->nvalid.as<int32_t>(), h->polya_idx.as<int32_t>(),
                         drng, n, h->ds, dout, dstat); }
    return 0;
}
} // extern "C++"

// ---- the short-read fallback of combined_detect_cnn (combined.py:251-301) behind the first pass (cnn_fallback.h) -----------------
static bool cnn_fallback_wanted(const adp_handle *h, int flags, const adp_row *rows)
{
    return (flags & ADP_CNN_FALLBACK) && h->cfg.fallback_to_llr_short_reads && rows;
}
// rows / bounds: the CALL's device row buffer and predictions (int64 [n, bstride]) once every read's first pass is in them.
// Enqueues the selection on the handle's stream; the count reaches the host in arena_end's copy.
static int cnn_fallback_select(adp_handle *h, const int32_t *dlen, int n, const adp_row *rows, const int64_t *bounds, int bstride)
{
    ALLOCCHK(h->fb_sel.ensure((size_t)n * 4));
    Scope s(h, "k_cnn_fb_select");
    hipLaunchKernelGGL(k_cnn_fb_select, dim3(1), dim3(SEL_THREADS), 0, h->stream, rows, bounds, bstride, dlen, n, 2ll * h->cfg.max_obs_adapter,
                       h->fb_sel.as<int32_t>(), h->op_used.as<unsigned int>() + 2);
    return 0;
}

// The second phase over the n_sel selected reads, enqueued on the handle's stream: the chain, the re-validation (k = 1,
// polya_end_topk given) and the merge into `rows`.  The selected signal rows are read where they lie (SigIdx); the re-validated
// rows and their candidates have buffers of their own -- the handle's hold the first pass (launch_validate's ValBufs).  Open-pore
// lists of re-validated rows go to the same arena of the call: the caller looks at its counter once more.
template <class SIG>
static int cnn_fallback_run(adp_handle *h, SIG dsig, const int32_t *dlen, int m, adp_row *rows, const int64_t *bounds, int bstride, int n_sel)
{
    hipStream_t st = h->stream;
    int rc = alloc_all(h, n_sel, true);
    if (rc) return rc;
    const size_t N = (size_t)n_sel;
    int64_t *drng, *dout, *db2; int32_t *dstat, *dlen_sub; int8_t *topk; adp_row *rows2;
    RCCHK(sub_carve(h, [&](Carve &c) { // ranges, new poly(A) ends, bounds of the re-validation, status, full_len, topk_none, rows
        drng = c.take<int64_t>(2 * N); dout = c.take<int64_t>(N); db2 = c.take<int64_t>(2 * N);
        dstat = c.take<int32_t>(N); dlen_sub = c.take<int32_t>(N); topk = c.take<int8_t>(N); rows2 = c.take<adp_row>(N);
    }));
    unsigned int *counts = phase_counts(h, OPW_FB);
    const int32_t *sel = h->fb_sel.as<int32_t>();
    const auto sig = sig_subset(dsig, sel);
    HIPCHK(hipMemsetAsync(counts, 0, 8, st));
    HIPCHK(hipMemsetAsync(topk, 0, N, st)); // (polya_end_topk is given)
    { Scope s(h, "k_cnn_fb_gather");
      hipLaunchKernelGGL(k_cnn_fb_gather, dim3((n_sel + 255) / 256), dim3(256), 0, st, sel, n_sel, 0, bounds, bstride, dlen, dlen_sub, drng,
                         (const int64_t *)nullptr, (const int32_t *)nullptr, (int64_t *)nullptr); }
    rc = refine_chain(h, sig, dlen_sub, n_sel, m, drng, dout, dstat);
    if (rc) return rc;
    { Scope s(h, "k_cnn_fb_gather");
      hipLaunchKernelGGL(k_cnn_fb_gather, dim3((n_sel + 255) / 256), dim3(256), 0, st, sel, n_sel, 1, bounds, bstride, dlen, dlen_sub, drng,
                         (const int64_t *)dout, (const int32_t *)dstat, db2); }
    const ValBufs vb{db2, topk, rows2};
    rc = launch_validate(h, sig, dlen_sub, n_sel, m, 1, n_sel, false, &vb);
    if (rc) return rc;
    { Scope s(h, "k_cnn_fb_merge");
      hipLaunchKernelGGL(k_cnn_fb_merge, dim3(n_sel), dim3(64), 0, st, sel, n_sel, (const int64_t *)dout, (const int32_t *)dstat,
                         (const adp_row *)rows2, rows, counts); }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- the LLR second opinion for reads the CNN path fails (ADP_CNN_SECOND_LLR, cnn_second_opinion.h) ------------------------------
static bool cnn_second_wanted(int flags, const adp_row *rows) { return (flags & ADP_CNN_SECOND_LLR) && rows; }
static bool cnn_sp_wanted(int flags, const adp_row *rows) { return (flags & ADP_WITH_START_PEAK) && rows; }
// rows: the CALL's device row buffer once every read's row of the CNN path is in it (behind the first pass, and again behind the
// fallback's merge when that ran).  The count reaches the host in arena_end's copy.
static int cnn_second_select(adp_handle *h, int n, const adp_row *rows)
{
    ALLOCCHK(h->so_sel.ensure((size_t)n * 4));
    Scope s(h, "k_cnn_so_select");
    hipLaunchKernelGGL(k_cnn_so_select, dim3(1), dim3(SEL_THREADS), 0, h->stream, rows, n, h->so_sel.as<int32_t>(), h->op_used.as<unsigned int>() + 3);
    return 0;
}

// The second opinion for the n_so selected reads, enqueued on the handle's stream.  The LLR primary is the LLR path's own up to
// k_polya_peak (llr_enqueue, stage 7) over ALL n reads in their minibatches -- N1 and the minibatch status are those
// adp_detect_llr computes -- with its boundaries in a buffer of this phase (the handle's bounds / topk_none / rows hold the CNN
// path's).  The validation (k = 1) reads the selected rows in place and leaves its rows in the phase's own; the merge copies those
// that passed into `rows`.  Open-pore lists of the second rows append to the call's arena: the caller looks at its counter once more.
//
// sr (ADP_CNN_SECOND_RESEGMENT, else null; cnn_second_resegment.h): the re-segmentation of the reads whose second row fails too.  Its
// arrays -- sized for the whole subset, which bounds its selection -- are pieces of the SAME carve, so that the second rows it reads
// stay where they are until its merge has run; its selection is enqueued here, behind the merge, and its count comes back with
// the arena counter the caller reads next.
struct SrPieces { RsPieces rs; Piece<int32_t> sel_j, sel_r; const adp_row *rows2_so = nullptr; };
static bool cnn_sr_wanted(int flags, const adp_row *rows) { return (flags & ADP_CNN_SECOND_RESEGMENT) && (flags & ADP_CNN_SECOND_LLR) && rows; }
static int cnn_tails(int flags, SigF32) { return flags & ADP_TAILS_NAN; }
// (int16 rows: the padding is implied, so the passes always stop at a read's end -- as adp_detect_llr_i16 runs them)
static int cnn_tails(int, SigI16) { return ADP_TAILS_NAN; }
template <class SIG>
static int cnn_second_run(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int minibatch, int flags, adp_row *rows, int n_so, SrPieces *sr)
{
    hipStream_t st = h->stream;
    const int tails = cnn_tails(flags, dsig);
    int rc = llr_enqueue(h, dsig, dlen, n, m, minibatch, tails, nullptr, 0, nullptr, nullptr, 7, nullptr);
    if (rc) return rc;
    const size_t R = (size_t)n, N = (size_t)n_so;
    int64_t *ball, *b2; int32_t *dlen_sub; int8_t *tall, *tsub; adp_row *rows2;
    RCCHK(sub_carve(h, [&](Carve &c) { // LLR bounds and topk_none of all reads; of the subset: bounds of the validation, full_len, topk_none, rows
        ball = c.take<int64_t>(2 * R); tall = c.take<int8_t>(R);
        b2 = c.take<int64_t>(2 * N); dlen_sub = c.take<int32_t>(N); tsub = c.take<int8_t>(N); rows2 = c.take<adp_row>(N);
        if (sr) { sr->rs.take(c, N); sr->sel_j = c.take<int32_t>(N); sr->sel_r = c.take<int32_t>(N); }
    }));
    unsigned int *counts = phase_counts(h, OPW_SO);
    const int32_t *sel = h->so_sel.as<int32_t>();
    const MbState *mbs = h->mbs.as<MbState>();
    HIPCHK(hipMemsetAsync(counts, 0, 12, st));
    if (h->L > 0) // (else every minibatch is ADP_MB_EMPTY_TRACE: k_cnn_so_gather reads no bounds)
        hipLaunchKernelGGL(k_llr_bounds, dim3((n + 255) / 256), dim3(256), 0, st, h->adapter_idx.as<int32_t>(), h->polya_idx.as<int32_t>(), n, h->ds,
                           h->pos_off, ball, tall, 0);
    { Scope s(h, "k_cnn_so_gather");
      hipLaunchKernelGGL(k_cnn_so_gather, dim3((n_so + 255) / 256), dim3(256), 0, st, sel, n_so, minibatch, mbs, dlen, (const int64_t *)ball,
                         (const int8_t *)tall, dlen_sub, b2, tsub); }
    const ValBufs vb{b2, tsub, rows2};
    rc = launch_validate(h, sig_subset(dsig, sel), dlen_sub, n_so, m, 1, n_so, false, &vb);
    if (rc) return rc;
    { Scope s(h, "k_cnn_so_merge");
      hipLaunchKernelGGL(k_cnn_so_merge, dim3(n_so), dim3(64), 0, st, sel, n_so, minibatch, mbs, (const adp_row *)rows2, rows, counts); }
    if (sr) {
        unsigned int *sr_counts = phase_counts(h, OPW_SR);
        sr->rows2_so = rows2;
        h->sr_ran = true;
        HIPCHK(hipMemsetAsync(sr_counts, 0, 16, st)); // (the three counts and the selection's)
        Scope s(h, "k_csr_select");
        hipLaunchKernelGGL(k_csr_select, dim3(1), dim3(SEL_THREADS), 0, st, sel, n_so, minibatch, mbs, (const adp_row *)rows2, sr->sel_j.p, sr->sel_r.p,
                           sr_counts + 3, sr_counts);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- the re-segmentation behind the second opinion (ADP_CNN_SECOND_RESEGMENT, cnn_second_resegment.h) -----------------------------------
// what the flag cannot go with, said before anything is launched
static int cnn_sr_supported(const adp_handle *h, int flags, const adp_row *rows)
{
    if (!(flags & ADP_CNN_SECOND_LLR) || !rows) { g_err = "ADP_CNN_SECOND_RESEGMENT needs ADP_CNN_SECOND_LLR and rows_out"; return ADP_ERR_INVALID; }
    if (flags & ADP_FLAG_TRUNCATED) { g_err = "ADP_CNN_SECOND_RESEGMENT does not go with ADP_FLAG_TRUNCATED (the truncation look validates from start 0)"; return ADP_ERR_UNSUPPORTED; }
    if (h->cfg.mvs_detect_overwrite) { g_err = "ADP_CNN_SECOND_RESEGMENT does not go with mvs_detect_overwrite"; return ADP_ERR_UNSUPPORTED; }
    if (h->layout == ADP_LAYOUT_SINGLE_READ) { g_err = "ADP_CNN_SECOND_RESEGMENT does not go with the single-read layout"; return ADP_ERR_UNSUPPORTED; }
    return 0;
}
// The second segmentation, its validation and the merge for the n_sr reads k_csr_select listed, enqueued on the handle's stream
// behind cnn_second_run, whose carve `sr` is a part of.  The stage buffers llr_enqueue filled over all reads of the call on THIS
// handle (pooled signal, cumulative sums, trace, peak lists) were last read by k_llr_bounds, which ran in front of the second
// opinion's validation on the same stream: they are spent and take the subset's trace phase, read i of the subset at position i
// (alloc_all over n reads covers n_sr <= n).  The minibatch states stay: llr_enqueue ran over all reads, so h->mbs is the call's.
// The new rows' open-pore lists append to the call's arena: the caller looks at its counter once more.
template <class SIG>
static int cnn_sr_run(adp_handle *h, SIG dsig, const int32_t *dlen, int m, int minibatch, int flags, adp_row *rows, const SrPieces &sr, int n_sr)
{
    hipStream_t st = h->stream;
    unsigned int *counts = phase_counts(h, OPW_SR);
    const RsPieces &p = sr.rs;
    { Scope s(h, "k_csr_gather");
      hipLaunchKernelGGL(k_csr_gather, dim3((n_sr + 255) / 256), dim3(256), 0, st, (const int32_t *)sr.sel_j.p, (const int32_t *)sr.sel_r.p, n_sr, minibatch,
                         (const MbState *)h->mbs.as<MbState>(), dlen, sr.rows2_so, h->ds, h->pos_off, p.dlen_sub.p, p.starts.p, p.b2.p, p.tsub.p,
                         h->adapter_idx.as<int32_t>(), p.mbs_sub.p); }
    RCCHK(reseg_trace_validate(h, sig_subset(dsig, sr.sel_r.p), p, m, cnn_tails(flags, dsig) != 0, n_sr, counts));
    { Scope s(h, "k_csr_merge");
      hipLaunchKernelGGL(k_csr_merge, dim3(n_sr), dim3(64), 0, st, (const int32_t *)sr.sel_j.p, (const int32_t *)sr.sel_r.p, n_sr, (const adp_row *)p.rows2.p,
                         sr.rows2_so, rows, counts); }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- what adp_detect_cnn does behind the first pass, in both execution forms ---------------------------------------------------------
// Called once every read's first-pass row lies in `rows`, the CALL's device row buffer (null: the caller wants no rows), and its
// predictions in `bounds` (int64 [n, bstride]); the lanes of a grouped call have drained.  sp (ADP_WITH_START_PEAK, else null): K1's
// results of the call.  -> 0 done, 1 run the call again, < 0 error; *changed: a phase wrote to `rows` behind the first pass.
//
// The fallback: its selection's count comes back with the arena counter at the call's one synchronisation point -- a call without
// selected reads (every call over full-length reads) ends there.  Otherwise the second phase follows and merges its rows over the
// first ones.  Its re-validated rows append to the call's arena; a read's open-pore list depends on its adapter end alone, so the
// second phase wants at most what the first one did and an arena grown for the first (to twice its demand) holds both: three
// attempts are still enough.
// The second opinion (ADP_CNN_SECOND_LLR) works the same way on the rows behind the fallback: its selection is enqueued with the
// fallback's (and once more behind a fallback merge), its count comes back in the same copy, and a call whose reads all passed
// ends there.  Its rows' open-pore lists depend on the LLR adapter end: they may want more than the first pass did, and the
// counter is cumulative over the call -- attempt 1 can fall short in the first pass, attempt 2 in this phase, attempt 3 holds both.
// The re-segmentation behind the second opinion (ADP_CNN_SECOND_RESEGMENT) is a fourth phase that writes lists, behind one more
// look at the counter; its rows' lists depend on the second opinion's "poly(A) end" and no earlier phase bounds them.  The bound in
// general: the counter adds up what the call WANTED, every phase wants the same in every attempt, and an attempt that falls short in
// phase p leaves an arena of twice the demand up to and including p -- so the next attempt gets past p, and a call needs at most one
// attempt per phase that can want more than the phases in front of it, plus the one that succeeds.  The fallback cannot (above), so
// that is first pass, second opinion, re-segmentation: FOUR attempts with the flag (cnn_attempts), three without, as before.
// The start-peak overlay: K1 ran beside the first pass and decorated its rows; the fallback and the second opinion deliver whole
// rows of their own validation, so the overlay is applied once more to the call's row buffer behind each (k_sp_decorate is
// idempotent); the truncation look's merge keeps the columns (k_pt_merge).
// The truncation look (ADP_FLAG_TRUNCATED) comes behind all of that, on every read's final row: one more synchronisation for its
// T1 count, and T2 only where a tail window passed.
static int cnn_attempts(int flags, const adp_row *rows) { return (flags & ADP_CNN_SECOND_RESEGMENT) && (flags & ADP_CNN_SECOND_LLR) && rows ? 4 : 3; }
template <class SIG>
static int cnn_after_first_pass(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int minibatch, int flags, adp_row *rows,
                                const int64_t *bounds, int bstride, const SpOut *sp, bool *changed)
{
    const bool fb = cnn_fallback_wanted(h, flags, rows), so = cnn_second_wanted(flags, rows);
    *changed = false;
    if (fb) RCCHK(cnn_fallback_select(h, dlen, n, rows, bounds, bstride));
    if (so) RCCHK(cnn_second_select(h, n, rows));
    unsigned int n_sel = 0, n_so = 0;
    int rc = arena_end(h, true, fb ? &n_sel : nullptr, so ? &n_so : nullptr); // (with a count to read it waits for the stream)
    if (rc < 0) return rc;
    h->fb_n_sel = n_sel; h->so_n_sel = 0;
    if (rc == 0 && n_sel) {
        *changed = true;
        RCCHK(cnn_fallback_run(h, dsig, dlen, m, rows, bounds, bstride, (int)n_sel));
        if (sp) cnn_sp_decorate(h, sp, rows, n); // (re-validated rows come bare; idempotent on the others)
        if (so) RCCHK(cnn_second_select(h, n, rows)); // (the merge changed rows: select again)
        HIPCHK(hipStreamSynchronize(h->stream));
        rc = arena_end(h, false, nullptr, so ? &n_so : nullptr);
        if (rc < 0) return rc;
    }
    if (rc == 0 && n_so) {
        *changed = true;
        h->so_n_sel = n_so;
        const bool sr = cnn_sr_wanted(flags, rows);
        SrPieces srp;
        unsigned int n_sr = 0;
        RCCHK(cnn_second_run(h, dsig, dlen, n, m, minibatch, flags, rows, (int)n_so, sr ? &srp : nullptr));
        if (sp) cnn_sp_decorate(h, sp, rows, n); // (the second opinion's rows come bare)
        HIPCHK(hipStreamSynchronize(h->stream));
        rc = arena_end(h, false, nullptr, nullptr, nullptr, sr ? &n_sr : nullptr);
        if (rc < 0) return rc;
        if (rc == 0 && n_sr) {
            if (n_sr > n_so) { g_err = "ADP_CNN_SECOND_RESEGMENT: selection count out of range"; return ADP_ERR_HIP; }
            RCCHK(cnn_sr_run(h, dsig, dlen, m, minibatch, flags, rows, srp, (int)n_sr));
            if (sp) cnn_sp_decorate(h, sp, rows, n); // (the re-segmented rows come bare as well)
            HIPCHK(hipStreamSynchronize(h->stream));
            rc = arena_end(h);
            if (rc < 0) return rc;
        }
    }
    if constexpr (std::is_same<SIG, SigF32>::value) { // (a float32-row phase: adp_detect_cnn_i16 refuses the flag)
    if (rc == 0 && trunc_wanted(flags, rows)) {
        *changed = true; // (T1 marks every row)
        rc = trunc_finish(h, dsig.base, dlen, n, m, rows);
    }
    }
    return rc;
}

// Chunks of whole minibatches over two lanes, free-running: while one lane's chunk is in the conv stack (matrix cores, one
// wave per SIMD, little HBM traffic), the other's is in the candidate validation -- the moving-window recurrences (latency of one
// wave's instruction stream, ~11 ms per launch whatever the number of reads), the order-statistics sweeps (HBM), the partition
// statistics.  Reads of different minibatches never interact on this path (find_peaks / row compaction are per minibatch).
template <class SIG>
static int cnn_grouped(adp_handle *h, SIG dsig, const int32_t *dlen, int n, int m, int minibatch, int flags, adp_row *rows_out,
                       int64_t *bounds_out, int mb_per_group, int n_lanes)
{
    const int n_mb = (n + minibatch - 1) / minibatch;
    const int G = (n_mb + mb_per_group - 1) / mb_per_group;
    const int k = h->cfg.polya_cand_k, kk = k < 1 ? 1 : k;
    const bool out_dev = (flags & ADP_OUT_DEVICE) != 0;
    // the fallback runs once on this handle, over the call's device row buffer, when all lanes have drained: it needs the
    // predictions of all reads here whether the caller wants them or not
    const bool fb = cnn_fallback_wanted(h, flags, rows_out);
    // K1's results of the whole call live in this handle's buffer (adp_detect_cnn sized it): the lanes write their slices
    SpOut *sp = cnn_sp_wanted(flags, rows_out) ? h->sp.as<SpOut>() : nullptr;
    h->last_n = n; h->last_nmb = n_mb; h->last_grouped = true;
    ALLOCCHK((rows_out && !out_dev && h->rows.ensure((size_t)n * sizeof(adp_row))) || ((bounds_out || fb) && h->bounds.ensure((size_t)n * (1 + ADP_MAX_CAND) * 8)));
    adp_handle *lanes[ADP_MAX_LANES];
    for (int i = 0; i < n_lanes; i++) {
        RCCHK(lane_get(h, i, mb_per_group * minibatch, &lanes[i]));
        drop_profile(lanes[i]);
    }
    adp_row *rows_dev = rows_out ? (out_dev ? rows_out : h->rows.as<adp_row>()) : nullptr;
    int64_t *bounds_dev = (bounds_out || fb) ? h->bounds.as<int64_t>() : nullptr;
    RCCHK(call_attempts(h, lanes, n_lanes, [&]() -> int {
        HIPCHK(hipEventRecord(h->ev_start, h->stream));
        for (int i = 0; i < n_lanes; i++) HIPCHK(hipStreamWaitEvent(lanes[i]->stream, h->ev_start, 0));
        for (int g = 0; g < G; g++) {
            adp_handle *l = lanes[g % n_lanes];
            const int r0 = g * mb_per_group * minibatch;
            const int ng = (n - r0) < mb_per_group * minibatch ? (n - r0) : mb_per_group * minibatch;
            const int rc = cnn_enqueue(l, sig_from(dsig, (size_t)r0, m), dlen + r0, ng, m, minibatch, rows_dev ? rows_dev + r0 : nullptr, hipMemcpyDeviceToDevice,
                                       bounds_dev ? bounds_dev + (size_t)r0 * (1 + kk) : nullptr, hipMemcpyDeviceToDevice, sp ? sp + r0 : nullptr);
            if (rc) { for (int i = 0; i < n_lanes; i++) (void)hipStreamSynchronize(lanes[i]->stream); return rc; }
        }
        for (int i = 0; i < n_lanes; i++) HIPCHK(hipStreamSynchronize(lanes[i]->stream));
        bool changed;
        return cnn_after_first_pass(h, dsig, dlen, n, m, minibatch, flags, rows_dev, bounds_dev, 1 + kk, sp, &changed);
    }, cnn_attempts(flags, rows_out)));
    if (rows_out && !out_dev) HIPCHK(hipMemcpyAsync(rows_out, h->rows.p, (size_t)n * sizeof(adp_row), hipMemcpyDeviceToHost, h->stream));
    if (bounds_out) HIPCHK(hipMemcpyAsync(bounds_out, h->bounds.p, (size_t)n * (1 + kk) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

// what both detect calls of the CNN path refuse behind begin_call
static int cnn_ready(const adp_handle *h, int m)
{
    if (m <= h->cfg.min_obs_adapter) { g_err = "preload shorter than min_obs_adapter"; return ADP_ERR_INVALID; }
    if (!h->cnn_have_w) { g_err = "adp_cnn_set_weights has not been called"; return ADP_ERR_INVALID; }
    return 0;
}
// A detect call of the CNN path over a resident matrix (its arguments checked, begin_call and cnn_ready done), in either execution form
template <class SIG>
static int cnn_pipeline_t(adp_handle *h, SIG dsig, const int32_t *dlen, int n_reads, int m, int minibatch, int flags, adp_row *rows_out,
                          int64_t *bounds_out)
{
    h->cnn_redo_f32 = false;
    // (K1's results of the whole call: sized here, before any phase's workspace call could move the buffer under them)
    ALLOCCHK(cnn_sp_wanted(flags, rows_out) && h->sp.ensure((size_t)n_reads * sizeof(SpOut)));
    // ADP_CNN_GROUPS (opt-in): unset / 1 = one chunk on one stream; 0 = automatic (chunks of about a quarter of the call, at most
    // what the conv stack's activation buffers hold, over two lanes); k = aim at k chunks.  Measured at the 200 k window (8000
    // reads, profiles/r03_cnn_chunks.txt): 4 chunks over 2 lanes 107.5 ms against 95.4 ms for one chunk -- the moving-window
    // series costs the same ~11 ms per LAUNCH whatever the number of reads (one wave's instruction stream per chain), so
    // chunking multiplies it, and the conv stack stretches by as much as its neighbours gain; equal at the default window.
    const int n_mb = (n_reads + minibatch - 1) / minibatch;
    int want = env_int("ADP_CNN_GROUPS", 1), n_lanes = env_int("ADP_CNN_LANES", 2);
    if (n_lanes < 1) n_lanes = 1;
    if (n_lanes > ADP_MAX_LANES) n_lanes = ADP_MAX_LANES;
    if (want <= 0) want = 4;
    if (n_mb >= 2 && want > 1) {
        int per = (n_mb + want - 1) / want;
        // a chunk beyond the activation buffers' capacity would be cut again inside the conv stack: keep chunks below it
        const int off = h->cfg.min_obs_adapter, ds = h->cfg.downscale_factor;
        const int Lc = (m - off + ds - 1) / ds, L1 = (Lc - 1) / 3 + 1;
        const size_t per_read = (size_t)CNN_C * ((size_t)L1 + 264) * 4;
        long long cap_mb = (long long)(((size_t)4 << 30) / per_read) / minibatch;
        if (cap_mb >= 1 && per > cap_mb) per = (int)cap_mb;
        if (per < 1) per = 1;
        const int G = (n_mb + per - 1) / per;
        if (G < n_lanes) n_lanes = G;
        if (G >= 2) return cnn_grouped(h, dsig, dlen, n_reads, m, minibatch, flags, rows_out, bounds_out, per, n_lanes);
    }
    // One chunk: the first pass delivers the caller's rows in-stream, and a call whose later phases change nothing ends at its one
    // synchronisation point.  Device rows are merged where the caller has them; host rows are merged in the handle's buffer and
    // delivered once more behind the phases.
    const bool out_dev = (flags & ADP_OUT_DEVICE) != 0;
    SpOut *sp = cnn_sp_wanted(flags, rows_out) ? h->sp.as<SpOut>() : nullptr;
    const int kk = h->cfg.polya_cand_k < 1 ? 1 : h->cfg.polya_cand_k; // (the stride of the predictions, as cnn_predict_dev lays them out)
    return call_attempts(h, nullptr, 0, [&]() -> int {
        RCCHK(cnn_enqueue(h, dsig, dlen, n_reads, m, minibatch, rows_out, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          bounds_out, hipMemcpyDeviceToHost, sp));
        HIPCHK(hipStreamSynchronize(h->stream));
        adp_row *rows_dev = rows_out ? (out_dev ? rows_out : h->rows.as<adp_row>()) : nullptr;
        bool changed;
        const int rc = cnn_after_first_pass(h, dsig, dlen, n_reads, m, minibatch, flags, rows_dev, h->bounds.as<int64_t>(), 1 + kk, sp, &changed);
        if (rc == 0 && changed && !out_dev) {
            HIPCHK(hipMemcpyAsync(rows_out, h->rows.p, (size_t)n_reads * sizeof(adp_row), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
        return rc;
    }, cnn_attempts(flags, rows_out));
}
} // extern "C++"

// combined_detect_cnn in one call: up to its short-read fallback, or with ADP_CNN_FALLBACK (and cfg.fallback_to_llr_short_reads)
// the whole of it.  bounds_out (host, may be NULL): int64 [n, 1 + max(k, 1)], what cnn_detect returns.
int adp_detect_cnn(adp_handle *h, const float *signals, const int32_t *full_len, int n_reads, int m, int minibatch, int flags,
                   adp_row *rows_out, int64_t *bounds_out)
{
    if (!h || !signals || !full_len || n_reads < 1 || minibatch < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (n_reads > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    if (flags & ADP_LLR_RESEGMENT) { g_err = "ADP_LLR_RESEGMENT goes with adp_detect_llr (the LLR primary)"; return ADP_ERR_UNSUPPORTED; }
    h->fb_n_sel = h->so_n_sel = 0; h->pt_looked = false; h->sr_ran = false;
    if (flags & ADP_CNN_SECOND_RESEGMENT) RCCHK(cnn_sr_supported(h, flags, rows_out));
    if (trunc_wanted(flags, rows_out)) RCCHK(trunc_supported(h));
    RCCHK(begin_call(h));
    RCCHK(cnn_ready(h, m));
    const float *dsig; const int32_t *dlen;
    int rc = stage_inputs(h, signals, full_len, n_reads, m, flags, &dsig, &dlen);
    if (rc) return rc;
    return cnn_pipeline_t(h, SigF32{dsig}, dlen, n_reads, m, minibatch, flags, rows_out, bounds_out);
}

// The same over raw int16 rows (include/adapted_hip_i16.h): every kernel that touches the signal reads the ADC samples and forms pA
// in registers; the phases, their order and their buffers are adp_detect_cnn's.
int adp_detect_cnn_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset, int n_reads,
                       int m, int minibatch, int flags, adp_row *rows_out, int64_t *bounds_out)
{
    if (!h || !raw || !full_len || !scale || !offset || n_reads < 1 || minibatch < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (!(flags & ADP_IN_DEVICE)) { g_err = "adp_detect_cnn_i16 takes device pointers (ADP_IN_DEVICE)"; return ADP_ERR_INVALID; }
    if (n_reads > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    if (h->layout == ADP_LAYOUT_SINGLE_READ) { g_err = "the single-read layout takes float32 input"; return ADP_ERR_UNSUPPORTED; }
    if (m & 3) { g_err = "int16 rows need m % 4 == 0 (8-byte aligned rows)"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_FLAG_TRUNCATED) { g_err = "ADP_FLAG_TRUNCATED takes float32 input (adp_calibrate_i16 + adp_detect_cnn)"; return ADP_ERR_UNSUPPORTED; }
    if (flags & ADP_LLR_RESEGMENT) { g_err = "ADP_LLR_RESEGMENT goes with adp_detect_llr (the LLR primary)"; return ADP_ERR_UNSUPPORTED; }
    h->fb_n_sel = h->so_n_sel = 0; h->pt_looked = false; h->sr_ran = false;
    if (flags & ADP_CNN_SECOND_RESEGMENT) RCCHK(cnn_sr_supported(h, flags, rows_out));
    RCCHK(begin_call(h));
    RCCHK(cnn_ready(h, m));
    // (samples at or beyond min(full_len, m) read as NaN: the padding is implied)
    return cnn_pipeline_t(h, SigI16{raw, scale, offset, full_len}, full_len, n_reads, m, minibatch, flags, rows_out, bounds_out);
}

int adp_llr_refine_polya(adp_handle *h, const float *signals, const int32_t *full_len, int n, int m, const int64_t *ranges,
                         int flags, int64_t *polya_out, int32_t *status_out)
{
    if (!h || !signals || !full_len || !ranges || !polya_out || !status_out || n < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    if (n > h->max_reads || m != h->m) { g_err = "n_reads/m exceed the handle's capacity"; return ADP_ERR_CAPACITY; }
    RCCHK(begin_call(h));
    const float *dsig; const int32_t *dlen;
    int rc = stage_inputs(h, signals, full_len, n, m, flags, &dsig, &dlen);
    if (rc) return rc;
    hipStream_t st = h->stream;
    rc = alloc_all(h, n, true);
    if (rc) return rc;
    ALLOCCHK(h->bounds_stage.ensure((size_t)n * 16 + (size_t)n * 12));
    int64_t *drng = h->bounds_stage.as<int64_t>();
    int64_t *dout = drng + 2 * (size_t)n;
    int32_t *dstat = reinterpret_cast<int32_t *>(dout + n);
    HIPCHK(hipMemcpyAsync(drng, ranges, (size_t)n * 16, (flags & ADP_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    rc = refine_chain(h, SigF32{dsig}, dlen, n, m, drng, dout, dstat);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(polya_out, dout, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(status_out, dstat, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return ADP_OK;
}

int adp_open_pores_arena(adp_handle *h, int32_t *out, uint64_t cap, uint64_t *used)
{
    if (!h || !used || (cap && !out)) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    *used = h->op_last_used;
    const uint64_t n = h->op_last_used < cap ? h->op_last_used : cap;
    if (n) {
        HIPCHK(hipMemcpyAsync(out, h->op_arena.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return ADP_OK;
}

int adp_synth_fill(adp_handle *h, float *dev_signals, const int32_t *dev_full_len, int n, int m, uint32_t seed,
                   uint32_t first_read, int decorate)
{
    if (!h || !dev_signals || n < 1 || m < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    const double ih_sd = std::sqrt(8.0 * (256.0 * 256.0 - 1.0) / 12.0);
    SynthConst k;
    k.sd_adapter = (float)(7.0 / ih_sd); k.sd_polya = (float)(2.5 / ih_sd); k.sd_rna = (float)(3.0 / ih_sd);
    k.sd_level = (float)(14.0 / ih_sd);
    hipLaunchKernelGGL(k_synth, dim3((m + 255) / 256, n), dim3(256), 0, h->stream, dev_signals, dev_full_len, n, m, seed, first_read,
                       decorate, k);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_dev_alloc(adp_handle *h, uint64_t bytes, void **out)
{
    if (!h || !out) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMalloc(out, bytes));
    return ADP_OK;
}
int adp_dev_free(adp_handle *h, void *p)
{
    if (!h) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipFree(p));
    return ADP_OK;
}
int adp_memcpy_h2d(adp_handle *h, void *dst, const void *src, uint64_t bytes)
{
    if (!h) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}
// grid = (ceil(m / 1024), n); block = 256: four samples per thread
__global__ void __launch_bounds__(256) k_calibrate_i16(const int16_t *__restrict__ raw, const int32_t *__restrict__ full_len,
                                                        const float *__restrict__ scale, const float *__restrict__ offset, int m,
                                                        float *__restrict__ out)
{
    const int r = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= m) return;
    const int len = full_len[r] < m ? full_len[r] : m;
    const float sc = scale[r], of = offset[r];
    const int16_t *src = raw + (size_t)r * m + i0;
    float *dst = out + (size_t)r * m + i0;
    const float nanv = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (i0 + j < m) dst[j] = (i0 + j < len) ? sc * ((float)src[j] + of) : nanv;
}

int adp_calibrate_i16(adp_handle *h, const int16_t *raw, const int32_t *full_len, const float *scale, const float *offset,
                      int n_reads, int m, float *signals_out)
{
    if (!h || !raw || !full_len || !scale || !offset || !signals_out || n_reads < 1 || m < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_calibrate_i16, dim3((m + 1023) / 1024, n_reads), dim3(256), 0, h->stream, raw, full_len, scale, offset, m, signals_out);
    HIPCHK(hipGetLastError());
    return ADP_OK;
}

int adp_expand_ragged(adp_handle *h, const void *packed, int is_int16, const int64_t *offsets, const int32_t *full_len,
                      const float *scale, const float *offset, int n_reads, int m, float *signals_out)
{
    if (!h || !packed || !offsets || !full_len || !signals_out || n_reads < 1 || m < 1 || (is_int16 && (!scale || !offset))) {
        g_err = "bad argument"; return ADP_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(h->device));
    const dim3 grid((m + 1023) / 1024, n_reads);
    if (is_int16)
        hipLaunchKernelGGL(k_expand_ragged<int16_t>, grid, dim3(256), 0, h->stream, (const int16_t *)packed, offsets, full_len, scale, offset, m, signals_out);
    else
        hipLaunchKernelGGL(k_expand_ragged<float>, grid, dim3(256), 0, h->stream, (const float *)packed, offsets, full_len,
                           (const float *)nullptr, (const float *)nullptr, m, signals_out);
    HIPCHK(hipGetLastError());
    return ADP_OK;
}

int adp_expand_ragged_i16(adp_handle *h, const int16_t *packed, const int64_t *offsets, const int32_t *full_len, int n_reads, int m,
                          int16_t *raw_out)
{
    if (!h || !packed || !offsets || !full_len || !raw_out || n_reads < 1 || m < 1) { g_err = "bad argument"; return ADP_ERR_INVALID; }
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_expand_ragged_raw, dim3((m + 1023) / 1024, n_reads), dim3(256), 0, h->stream, packed, offsets, full_len, m, raw_out);
    HIPCHK(hipGetLastError());
    return ADP_OK;
}

int adp_host_alloc(adp_handle *h, uint64_t bytes, void **out)
{
    if (!h || !out) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return ADP_OK;
}
int adp_host_free(adp_handle *h, void *p)
{
    if (!h) return ADP_ERR_INVALID;
    HIPCHK(hipHostFree(p));
    return ADP_OK;
}
int adp_memcpy_h2d_async(adp_handle *h, void *dst, const void *src_pinned, uint64_t bytes)
{
    if (!h) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(dst, src_pinned, bytes, hipMemcpyHostToDevice, h->stream3));
    return ADP_OK;
}
int adp_copy_mark(adp_handle *h, int slot)
{
    if (!h || slot < 0 || slot >= 16) return ADP_ERR_INVALID;
    if (!h->ev_copy[slot]) HIPCHK(hipEventCreateWithFlags(&h->ev_copy[slot], hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->ev_copy[slot], h->stream3));
    return ADP_OK;
}
int adp_copy_wait(adp_handle *h, int slot)
{
    if (!h || slot >= 16) return ADP_ERR_INVALID;
    if (slot < 0) { HIPCHK(hipStreamSynchronize(h->stream3)); return ADP_OK; }
    if (!h->ev_copy[slot]) return ADP_ERR_INVALID;
    HIPCHK(hipEventSynchronize(h->ev_copy[slot]));
    return ADP_OK;
}
int adp_memcpy_d2h(adp_handle *h, void *dst, const void *src, uint64_t bytes)
{
    if (!h) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ADP_OK;
}

int adp_kernel_times(adp_handle *h, const char **names_out, float *ms_out, int cap)
{
    if (!h) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    int k = 0;
    const adp_handle *src[1 + ADP_MAX_LANES] = {h};
    int ns = 1;
    if (h->last_grouped) for (int i = 0; i < ADP_MAX_LANES; i++) if (h->lane[i]) src[ns++] = h->lane[i];
    for (int q = 0; q < ns; q++) {
        for (const ProfEntry &e : src[q]->prof) {
            if (k >= cap) break;
            float ms = 0.f;
            HIPCHK(hipEventSynchronize(e.b));
            HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
            names_out[k] = e.name;
            ms_out[k] = ms;
            k++;
        }
    }
    return k;
}

int adp_debug_fetch(adp_handle *h, int what, void *host_out, uint64_t bytes)
{
    if (!h || !host_out) return ADP_ERR_INVALID;
    HIPCHK(hipSetDevice(h->device));
    const void *src = nullptr;
    switch (what) {
    case 0: {
        if (h->last_grouped) {
            if (bytes > (uint64_t)h->last_nmb * 32) return ADP_ERR_INVALID;
            HIPCHK(hipMemcpyAsync(host_out, h->mbparams.p, bytes, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            return ADP_OK;
        }
        if (h->ghist.cap < (size_t)h->last_nmb * 32) return ADP_ERR_INVALID;
        hipLaunchKernelGGL(k_mb_params_out, dim3((h->last_nmb + 255) / 256), dim3(256), 0, h->stream, h->mbs.as<MbState>(),
                           h->last_nmb, h->ghist.as<double>());
        src = h->ghist.p; break; }
    case 1: src = h->nvalid.p; break;
    case 2: src = h->down.p; break;
    case 3: src = h->trace.p; break;
    case 4: src = h->adapter_idx.p; break;
    case 5: src = h->polya_idx.p; break;
    case 6: { int32_t lp = h->Lp; if (bytes < 4) return ADP_ERR_INVALID; memcpy(host_out, &lp, 4); return ADP_OK; }
    case 7: src = h->t1.p; break;
    case 10: { // the last adp_detect_cnn call's fallback: reads selected, exception rows made, rows re-validated
        if (bytes < 12) return ADP_ERR_INVALID;
        int32_t c[3] = {(int32_t)h->fb_n_sel, 0, 0};
        if (h->fb_n_sel) { HIPCHK(hipMemcpyAsync(c + 1, phase_counts(h, OPW_FB), 8, hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); }
        memcpy(host_out, c, 12); return ADP_OK; }
    case 11: { // the last adp_detect_cnn call's LLR second opinion: reads selected, rows replaced, re-validated and still failing, minibatches without one
        if (bytes < 16) return ADP_ERR_INVALID;
        int32_t c[4] = {(int32_t)h->so_n_sel, 0, 0, 0};
        if (h->so_n_sel) { HIPCHK(hipMemcpyAsync(c + 1, phase_counts(h, OPW_SO), 12, hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); }
        memcpy(host_out, c, 16); return ADP_OK; }
    case 12: { // the truncation look of the last adp_detect_llr / adp_detect_cnn call: eligible reads, T1 passed, rows replaced
        if (bytes < 12) return ADP_ERR_INVALID;
        int32_t c[3] = {0, 0, 0};
        if (h->pt_looked) { HIPCHK(hipMemcpyAsync(c, phase_counts(h, OPW_PT), 12, hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); }
        memcpy(host_out, c, 12); return ADP_OK; }
    case 25: { // the re-segmentation of the last adp_detect_llr call: eligible reads, reads with a second poly(A) end, rows replaced
        if (bytes < 12) return ADP_ERR_INVALID;
        int32_t c[3] = {0, 0, 0};
        if (h->rs_ran) { HIPCHK(hipMemcpyAsync(c, phase_counts(h, OPW_RS), 12, hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); }
        memcpy(host_out, c, 12); return ADP_OK; }
    case 26: { // the re-segmentation behind the last adp_detect_cnn(_i16) call's second opinion: eligible reads, reads with a second poly(A) end, rows replaced
        if (bytes < 12) return ADP_ERR_INVALID;
        int32_t c[3] = {0, 0, 0};
        if (h->sr_ran) { HIPCHK(hipMemcpyAsync(c, phase_counts(h, OPW_SR), 12, hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); }
        memcpy(host_out, c, 12); return ADP_OK; }
    case 9: src = h->have_series.p; if (bytes > h->have_series.cap) return ADP_ERR_INVALID; break; // 1: the read's moving-window series were prepared by a series kernel
    // what the kernels of phase C hand to each other (llr_stream.h, peaks.h), each copy bounded by its buffer
    case 13: src = h->ck.p; if (bytes > h->ck.cap) return ADP_ERR_INVALID; break;
    case 14: src = h->tail.p; if (bytes > h->tail.cap) return ADP_ERR_INVALID; break;
    case 15: src = h->bmax.p; if (bytes > h->bmax.cap) return ADP_ERR_INVALID; break;
    case 16: src = h->bmin.p; if (bytes > h->bmin.cap) return ADP_ERR_INVALID; break;
    case 17: src = h->gstat.p; if (bytes > h->gstat.cap) return ADP_ERR_INVALID; break;
    case 18: src = h->npk.p; if (bytes > h->npk.cap) return ADP_ERR_INVALID; break;
    case 19: src = h->pk.p; if (bytes > h->pk.cap) return ADP_ERR_INVALID; break;
    case 20: // (a handle made with ADP_PK_VALUES=0 has no such buffer)
        if (!h->pkv.p) { g_err = "this handle keeps no heights beside its maxima lists (ADP_PK_VALUES=0)"; return ADP_ERR_INVALID; }
        src = h->pkv.p; if (bytes > h->pkv.cap) return ADP_ERR_INVALID; break;
    case 22: src = h->wend.p; if (bytes > h->wend.cap) return ADP_ERR_INVALID; break; // how far pass 2 computed each read's trace
    case 23: src = h->redo.p; if (bytes > h->redo.cap) return ADP_ERR_INVALID; break; // the windowed pass 2's redo list: count, reads
    case 21: { // the minibatches' status words (ADP_MB_*), as the kernels of the last plain call left them
        if (h->last_grouped || !h->mbs.p || h->last_nmb < 1 || bytes > (uint64_t)h->last_nmb * 4 || h->gbelow.cap < (size_t)h->last_nmb * 4) return ADP_ERR_INVALID;
        hipLaunchKernelGGL(k_mb_status_out, dim3((h->last_nmb + 255) / 256), dim3(256), 0, h->stream, h->mbs.as<MbState>(), h->last_nmb, h->gbelow.as<int32_t>());
        src = h->gbelow.p; break; }
    case 24: { // the fused N1 state of the last plain call, N1F_DEBUG_WORDS 32-bit words per minibatch: plain copies of fz, mbs, n1heavy
        const int n_mb = h->last_nmb;
        if (h->last_grouped || n_mb < 1 || h->n1_fused_nmb != n_mb || !h->fz.p || !h->mbs.p || !h->n1heavy.p) {
            g_err = "the last call on this handle did not take the single-pass N1 route"; return ADP_ERR_INVALID;
        }
        if (bytes != (uint64_t)n_mb * N1F_DEBUG_WORDS * 4) return ADP_ERR_INVALID;
        static_assert(sizeof(N1Fused) == 40 && 12 + 2 + 2 * N1H_MAX == N1F_DEBUG_WORDS, "layout of adp_debug_fetch(24)");
        std::vector<N1Fused> f((size_t)n_mb);
        std::vector<MbState> s((size_t)n_mb);
        std::vector<uint32_t> hv((size_t)n_mb * N1H_WORDS);
        HIPCHK(hipMemcpyAsync(f.data(), h->fz.p, f.size() * sizeof(N1Fused), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(s.data(), h->mbs.p, s.size() * sizeof(MbState), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(hv.data(), h->n1heavy.p, hv.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        uint32_t *o = (uint32_t *)host_out;
        for (int mb = 0; mb < n_mb; mb++, o += N1F_DEBUG_WORDS) {
            memcpy(o, &f[mb], 40);
            o[10] = (uint32_t)s[mb].fused; o[11] = (uint32_t)s[mb].status;
            const uint32_t *g = hv.data() + (size_t)mb * N1H_WORDS;
            o[12] = g[N1H_NH]; o[13] = g[N1H_NH + 1];
            memcpy(o + 14, g + N1H_KEYS, N1H_MAX * 4);
            memcpy(o + 14 + N1H_MAX, g + N1H_CNTS, N1H_MAX * 4);
        }
        return ADP_OK; }
    case 8: { if (bytes < 64 || bytes > sizeof(unsigned long long) * ADP_NDBG) return ADP_ERR_INVALID;
              HIPCHK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dbg), bytes, 0, hipMemcpyDeviceToHost));
              static unsigned long long tally[ADP_NTALLY][8];
              HIPCHK(hipMemcpyFromSymbol(tally, HIP_SYMBOL(g_bs_tally), sizeof(tally), 0, hipMemcpyDeviceToHost));
              unsigned long long *o = (unsigned long long *)host_out;
              for (int j = 0; j < 5; j++) { o[j] = 0; for (int i = 0; i < ADP_NTALLY; i++) o[j] += tally[i][j]; }
              return ADP_OK; }
    default: return ADP_ERR_INVALID;
    }
    // (the stage buffers belong to the plain pipeline: a grouped call keeps them in its lanes, a handle that has not run the LLR path has none)
    if (!src || (what != 0 && h->last_grouped)) { g_err = "no stage buffers of a plain (one-group) LLR call on this handle"; return ADP_ERR_INVALID; }
    HIPCHK(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (what == 0) HIPCHK(hipMemsetAsync(h->ghist.p, 0, (size_t)h->last_nmb * 32, h->stream));
    return ADP_OK;
}

} // extern "C"
