// handle.h -- what the library's translation units (adapted_hip.hip: the detect path; modules.hip: the reference-module
// drop-ins) share on the host: the error string, the handle, the pieces of its carved buffers (carve.h) and the start / profiling
// scope of a call.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "adapted_hip.h"
#include "carve.h"

#define ADP_HIDDEN __attribute__((visibility("hidden")))

// what adp_last_error returns: one object per thread (defined in adapted_hip.hip)
extern ADP_HIDDEN thread_local std::string g_err;

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                       \
            return ADP_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)
// a helper's non-zero return code (g_err already set) ends the caller
#define RCCHK(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
// device memory that did not grow (DevBuf::ensure, one or several joined with ||) ends the caller
#define ALLOCCHK(failed) do { if (failed) { g_err = "device allocation failed"; return ADP_ERR_HIP; } } while (0)

// grow-only device memory, released with its owner (not copyable: two owners would free it twice)
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        if (p) { if (hipFree(p) != hipSuccess) return -1; p = nullptr; cap = 0; }
        if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return -1; }
        cap = bytes;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

struct ProfEntry { const char *name; hipEvent_t a, b; };
#define ADP_MAX_LANES 4

struct adp_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream3 = nullptr;          // copy stream (adp_memcpy_h2d_async)
    hipEvent_t ev_copy[16] = {};            // adp_copy_mark / adp_copy_wait
    hipStream_t stream2 = nullptr;          // side stream: the start-peak scan (HBM-bound) beside the float64 gains (ALU-bound)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    adp_cfg cfg;
    int max_reads = 0, m = 0;
    // geometry of the LLR path
    int T = 0, off = 0, ds = 1, L = 0, Lp = 0, nck = 0, nsum = 0;
    DevBuf mbs, ghist, gbelow, gcnt, cbuf, fz, fcnt, n1heavy, ct_pk, ct_pv, ct_out, gstat, down, nvalid, ck, tail, trace, bmax, bmin, t1, adapter_idx, polya_idx;
    DevBuf bounds, topk_none, rows, preq, series, have_series, vscratch, pk, pkv, npk, wend, redo, mk, st, sp, any_none, sig_stage, len_stage, bounds_stage;
    int vslots = 0, vstride = 0, pslots = 0;
    bool profiling = false;
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    int last_n = 0, last_nmb = 0;
    int n1_fused_nmb = 0; // minibatches of the last launch_n1 if it took the single-pass route (n1_fused.h), else 0
    int layout = 0;   // ADP_LAYOUT_*: 1 = the single-read API (pooled from sample 0)
    int oh1 = 5;      // head offset of the first gains pass
    int pos_off = 0;  // added to pooled indices * ds for sample positions
    DevBuf rng0;      // per-read [0, T) ranges of the single-read layout
    // CNN head: weights of the four layers; the split stack's activations (cnn_conv_split.h): rows [chunk][Lrows][272 B] of layer 1, the
    // only ones in HBM (their padding is laid down per geometry: cnn_Lpad, cnn_L1, cnn_chunk), and the one row that takes the last
    // kernel's stores without an output
    DevBuf cnn_w, cnn_rows, cnn_dump, cnn_x, cnn_sc, ct_st, ct_lnz, ct_ap, cstat, op_arena, op_used, series_plan;
    DevBuf ws;              // the module entry points (modules.hip): one call's staging and scratch (ws_carve)
    // the phases behind a detect call's first pass (cnn_fallback.h, cnn_second_opinion.h, polya_truncated.h): the reads each one
    // selected [reads of the call] -- fb_sel and so_sel are both live between the first pass and the counter read -- and the
    // per-subset arrays and rows of the phase that is running (carved by it: each runs to completion before the next starts)
    DevBuf fb_sel, so_sel, pt_sel, sub_ws;
    // what adp_debug_fetch(10 / 11 / 12) reports beside the phases' device counts (the tail of op_used): the reads the last
    // adp_detect_cnn call selected for the fallback / the second opinion (0: that phase did not run), and whether the last
    // detect call looked for truncated tails
    unsigned int fb_n_sel = 0, so_n_sel = 0;
    bool pt_looked = false;
    // the re-segmentation of adp_detect_llr (ADP_LLR_RESEGMENT, llr_resegment.h): the reads it selected [reads of the call], the
    // minibatch states of a GROUPED call (the lanes recycle theirs from group to group: every group leaves a copy here), and
    // whether the last detect call ran the phase (adp_debug_fetch 25)
    DevBuf rs_sel, rs_mbs;
    bool rs_ran = false;
    // the same phase behind the second opinion of adp_detect_cnn (ADP_CNN_SECOND_RESEGMENT, cnn_second_resegment.h): its arrays are
    // pieces of the second opinion's carve; whether the last adp_detect_cnn(_i16) call ran its selection (adp_debug_fetch 26)
    bool sr_ran = false;
    unsigned int op_last_used = 0;
    bool cnn_have_w = false;
    int cnn_Lpad = 0, cnn_L1 = 0, cnn_chunk = 0, n_cu = 256;
    // conv stack: 1 = split float16 MFMA (cnn_conv_split.h, the default), 0 = exact float32 MFMA (cnn_conv.h; ADP_CNN_CONV=f32).
    // cnn_redo_f32: the split kernels met an activation outside the float16 range in this call -- it is being repeated in float32
    int cnn_mode = 1;
    DevBuf cnn_actf[2];                                  // the exact-float32 stack's activations [chunk][64][Lpad] (cnn_rows: the split rows)
    int cnn_f_Lpad = 0, cnn_f_L1 = 0, cnn_f_chunk = 0;
    bool cnn_redo_f32 = false;
    DevBuf cnn_wsp;          // split B fragments of layers 1 and 2
    float cnn_sw[4] = {1.f, 1.f, 1.f, 1.f}; // scales of the split weights: layers 1, 2, 3 (folded into layer 2's kernel) and 0 (into layer 1's)
    // grouped execution of the LLR path (llr_grouped): child handles ("lanes") with their own streams and a workspace for ONE
    // group of minibatches; consecutive groups go to alternating lanes so that the phases of neighbouring groups overlap
    adp_handle *lane[ADP_MAX_LANES] = {};
    adp_handle *owner = nullptr;            // a lane's parent: owns the open-pore arena and collects the profile
    DevBuf sphead;                          // K1 state between k_sp_head, the pooling pass and k_sp_tail
    DevBuf mbstat, mbparams;                // parent: minibatch status / N1 parameters of a grouped call
    std::vector<hipEvent_t> ev_sync;        // parent: phase-done events of the groups (no timing)
    hipEvent_t ev_start = nullptr;          // parent: inputs staged, arena counter reset
    bool last_grouped = false;
    // launch attributes already requested through this handle (hipFuncSetAttribute per kernel instantiation and device; kept per
    // handle -- a handle is used by one thread at a time -- instead of in process-wide statics): the kernels lds_attr_once has
    // seen, and the largest size asked for the two kernels whose need grows with the configuration
    std::vector<const void *> lds_attr_set;
    size_t lds_series_set = 0, lds_series_set_i16 = 0;
#ifdef ADP_ABLATE
    int ablate = 0;   // the mask this handle last copied to its device (sync_ablate)
#endif
};

// ---- a call's pieces of the handle's two carved buffers (carve.h).  A module call completes before it returns, and a phase runs
// to completion before the next starts, so the next one takes the same memory: each buffer holds the largest single need.
// ws: the module entry points' staging and scratch, in 256-byte aligned pieces
template <class F> static int ws_carve(adp_handle *h, F &&pieces) { ALLOCCHK(!carve_pieces(h->ws, 256, pieces)); return ADP_OK; }
// sub_ws: the per-subset arrays of the phase that is running, in 16-byte aligned pieces
template <class F> static int sub_carve(adp_handle *h, F &&pieces) { ALLOCCHK(!carve_pieces(h->sub_ws, 16, pieces)); return ADP_OK; }

// a kernel's dynamic LDS size, requested once per handle and kernel instantiation (`kernel`: its address)
static inline int lds_attr_once(adp_handle *h, const void *kernel, size_t bytes)
{
    for (const void *k : h->lds_attr_set) if (k == kernel) return ADP_OK;
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    h->lds_attr_set.push_back(kernel);
    return ADP_OK;
}

// ---- a call's start and its profiling scopes (adapted_hip.hip) --------------------------
ADP_HIDDEN hipEvent_t next_event(adp_handle *h);
// a call that works on the device: the handle's device current, the profile of the call before it dropped
ADP_HIDDEN int begin_call(adp_handle *h);

struct Scope {
    adp_handle *h; hipEvent_t b = nullptr; hipStream_t st;
    Scope(adp_handle *h_, const char *name, hipStream_t st_ = nullptr) : h(h_), st(st_ ? st_ : h_->stream)
    {
        if (!h->profiling || !name) return;
        hipEvent_t a = next_event(h);
        b = next_event(h);
        (void)hipEventRecord(a, st);
        h->prof.push_back({name, a, b});
    }
    ~Scope() { if (b) (void)hipEventRecord(b, st); }
};

// ---- the front detector of adp_adapter_front(_i16) (modules.hip) for adp_adapter_front_revalidate(_i16) (adapted_hip.hip) ------
// af_check: what every form checks before anything is launched.  af_detect_staged: the signal staged (float32 host signals) and
// k_adapter_front over `rows` (host), which are staged in but NOT patched -- device pointers into the handle's module workspace,
// good until the next module call: the matrix, the rows, the detector's side outputs.  raw != nullptr: the int16 form.
struct AfStaged { const float *sig; adp_row *rows; int32_t *info; int64_t *shift, *cand; double *diff; };
ADP_HIDDEN int af_check(adp_handle *h, const void *sig, int n_reads, int m, const adp_row *rows, const adp_adapter_front_args *args,
                        const int32_t *info_out, const int64_t *shift_out, const int64_t *cand_out, const double *diff_out);
ADP_HIDDEN int af_detect_staged(adp_handle *h, const float *sig, const int16_t *raw, const int32_t *full_len, const float *scale,
                                const float *offset, int n_reads, int m, const adp_row *rows, const adp_adapter_front_args *args,
                                int flags, AfStaged *out);
