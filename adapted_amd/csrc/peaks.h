// peaks.h -- peak picking on the LLR traces, one wave per read.
//
//   T1 LLRTrace._trace_start_end                       reference adapted/detect/llr.py:135-142
//   P1 find_peaks_in_trace                             adapted/detect/llr.py:204-224
//   P2 correct_for_plateau                             adapted/detect/llr.py:145-177
//   P3 correct_for_split_peak                          adapted/detect/llr.py:180-201
//   A1 first candidate -> adapter_end                  adapted/detect/combined.py:180-188
//   P4 detect_full_polya_trace_peak_with_spike         adapted/detect/llr.py:406-479
//
// scipy.signal.find_peaks (third party, not in the reference tree) is restated from its
// published algorithm: strict local maxima with plateau midpoints -> optional minimum
// distance by descending height -> prominence (walk to the next higher sample on each side,
// lowest point on the way) -> width at rel_height by linear interpolation.  Here the 64 lanes
// of a wave evaluate 64 candidate maxima at once; the walks skip whole 64-point blocks using
// the per-block max/min the gains kernel left behind, and the minimum-distance rule is solved
// as its fixed point ("kept iff no kept higher neighbour within the distance") instead of a
// global sort.
#pragma once
#include "common.h"
#include "find_peaks.h"

extern __device__ unsigned long long g_dbg[ADP_NDBG]; // (debug tallies; 16-23: k_polya_peak in a -DADP_PHASE_TIMING build)

// ---------------------------------------------------------------- adapter end (P1 + P2 + P3 + A1)
// One read by one wave: the candidate in pooled units, or -1.  g / bmx / bmn: the read's trace and block summaries, in global memory or
// staged in LDS (P); se = T1's clip; s1 / s2 / nnan: the moments k_gains<1> left.
template <class P>
static __device__ int adapter_peak_read(P g, P bmx, P bmn, int n, int2 se, double s1, double s2, int nnan,
                                        double prominence, double rel_height, int width)
{
    const int ln = lane_id();
    const int cn = se.y - se.x; // clip = g[start:end]
    if (n < 3 || cn < 3) return -1;
    // np.nanstd(clip), clip = g[start:end]: k_gains<1> left the sum, sum of squares and NaN count of the whole
    // trace; the few points outside the clip (all <= 0, never NaN, except possibly g[end]) are taken out here.
    // (One-pass float64 moments instead of numpy's two passes: it only scales a threshold.)
    double o1 = 0.0, o2 = 0.0; int onan = 0;
    // (eight loads in flight per lane: these two sweeps cover most of the trace of a typical read)
    for (int i0 = 0; i0 < se.x; i0 += 512) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int i = i0 + u * 64 + ln; v[u] = i < se.x ? g[i] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; u++) { o1 += v[u]; o2 += v[u] * v[u]; }
    }
    for (int i0 = se.y; i0 < n; i0 += 512) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int i = i0 + u * 64 + ln; v[u] = i < n ? g[i] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; u++) { if (v[u] == v[u]) { o1 += v[u]; o2 += v[u] * v[u]; } else onan++; }
    }
    o1 = wave_sum(o1); o2 = wave_sum(o2); onan = wave_sum(onan);
    const int cnt = cn - (nnan - onan);
    const double sum = s1 - o1, sq = s2 - o2;
    const double mean = sum / (double)cnt;
    double var = (sq - sum * mean) / (double)cnt;
    if (var < 0.0) var = 0.0;
    double sd = sqrt(var);
    TraceViewT<P> tv{g, bmx, bmn, se.x, se.y - 1, 0};
    int peak = wave_first_peak(tv, prominence * sd, (double)width, rel_height);
    if (peak < 0) return -1;
    // P2 correct_for_plateau(trace, peak, s=10, t=0.9, window=500)
    {
        const int wn = min(peak + 500, n) - peak;
        const int nch = wn - 1;
        const double w0 = g[peak];
        int best = -1;
        for (int i = ln; i <= nch - 10; i += 64) {
            bool ok = g[peak + i + 9] > 0.9 * w0;
            for (int j = i; ok && j < i + 9; j++) ok = (g[peak + j + 1] - g[peak + j] >= 0.0);
            if (ok) best = i;
        }
        best = wave_max(best);
        if (best >= 0) peak += best + 9;
    }
    // P3 correct_for_split_peak: find_peaks(window, width=10, prominence=1.0)[0]
    {
        const int wn = min(peak + 500, n) - peak;
        TraceViewT<P> tw{g, nullptr, nullptr, peak, peak + wn - 1, 0};
        int pk = wave_first_peak(tw, 1.0, 10.0, 0.5);
        if (pk >= 0 && g[pk] >= 0.9 * g[peak]) peak = pk;
    }
    return peak;
}

// grid = n_reads waves.  adapter_idx[r] = candidate in pooled units, or -1.
// (Round 4, measured and dropped: traces of at most 2048 points walked from an LDS copy by a launch of their own -- 2.57 against
// 2.68 ms at the 16 k window, 3.2 against 2.65 on heavy-tailed lengths: the walks are bound by their serial steps, not by where
// the samples come from.  tools/experiments/r05_pruned_variants.patch)
__global__ void __launch_bounds__(64) k_adapter_peak(const double *__restrict__ trace, const int32_t *__restrict__ nvalid, int Lp,
                                                     const double *__restrict__ bmax, const double *__restrict__ bmin, int nsum,
                                                     const int2 *__restrict__ t1, int mbsize, const MbState *__restrict__ mbs,
                                                     double prominence, double rel_height, int width,
                                                     int32_t *__restrict__ adapter_idx, const double *__restrict__ gstat)
{
    const int r = blockIdx.x;
    const int ln = lane_id();
    if (mbs[r / mbsize].status != ADP_MB_OK) { if (ln == 0) adapter_idx[r] = -1; return; }
    const int n = nvalid[r];
    int result = -1;
    if (n >= 3) {
        const double *g = trace + (size_t)r * Lp;
        const double *bx = bmax + (size_t)r * nsum, *bn = bmin + (size_t)r * nsum;
        const int2 se = t1[r];
        const double s1 = gstat[3 * r], s2 = gstat[3 * r + 1];
        const int nnan = (int)gstat[3 * r + 2];
        result = adapter_peak_read<const double *>(g, bx, bn, n, se, s1, s2, nnan, prominence, rel_height, width);
    }
    if (ln == 0) adapter_idx[r] = result;
}

// ---------------------------------------------------------------- poly(A) end (P4)
// 2-bit state per local maximum, by ORDINAL in the read's index-ordered list of maxima; transitions only clear
// bits (one LDS atomic and): undecided 3 -> kept 2 / removed 1
#ifndef PK_STEP
#define PK_STEP 16 // kept maxima examined per step of step 4
#endif
#ifndef PK_PREFIX
#define PK_PREFIX 224 // maxima of the first attempt (one round of step 2; 96 000 reads at the 200 k window: 5.2 ms without the prefix, 2.88 with 896, 2.50 with 448, 2.30 with 224, 2.38 with 112); the default of the kernel's `prefix` argument, which the host takes from ADP_PK_PREFIX (0: the whole list at once, as before; same results)
#endif
#define PST_NONE 0u
#define PST_REMOVED 1u
#define PST_KEPT 2u
#define PST_UNDECIDED 3u

// persistent grid of waves.  pk[Lp/2+1] int32 per READ (list of maxima, pre-filled by k_gains; ends up holding
// the kept ones), mk[Lp/2+1] uint32 per SLOT (work list of undecided maxima: ordinal << 8 | neighbour mask);
// the states live in dynamic LDS: ((Lp/2+1) + 8) / 16 + 2 words per wave.  prefix: the first attempt's maxima (0: all).
//
// Strict local maxima are at least two samples apart, so at most four of them lie within the minimum distance
// (|dp| <= 9) on either side of a maximum: the neighbourhood is the ordinals k-4 .. k+4, whatever the positions.
__global__ void __launch_bounds__(64, 8) k_polya_peak(const double *__restrict__ trace, const int32_t *__restrict__ nvalid, int Lp,
                                                   const double *__restrict__ bmax, const double *__restrict__ bmin, int nsum,
                                                   const int32_t *__restrict__ adapter_idx, int n_reads, int mbsize,
                                                   const MbState *__restrict__ mbs, int32_t *__restrict__ pk_all,
                                                   uint32_t *__restrict__ mk_all, int32_t *__restrict__ polya_idx,
                                                   const int32_t *__restrict__ npk_all, const double *__restrict__ pkv_all, int prefix,
                                                   const int32_t *__restrict__ wend_all = nullptr, int32_t *__restrict__ redo = nullptr,
                                                   int redo_pass = 0)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stw_raw[];
    LDS uint32_t *stw = (LDS uint32_t *)stw_raw; // ordinal k is slot k + 4 (slots 0..3 stay PST_NONE)
    const int ln = lane_id();
    const int half = Lp / 2 + 1;
    uint32_t *mk = mk_all + (size_t)blockIdx.x * half;
    // THE WINDOWED PASS 2 (wend_all != nullptr, redo_pass = 0): read r's trace, summaries and maxima are known on [0, wend_all[r])
    // only.  wend == n: the whole-trace code, untouched.  wend < n: t.hi = wend - 1 is the last KNOWN sample, and every step answers "unknown" where
    // the window does not show what the whole trace would say --
    //   distance rule: a maximum at p >= wend - 10 may have an unseen neighbour within 9 samples; it stays undecided for good (not on
    //     the work list), and the prefix machinery does the rest: what depends on it stays undecided, what is decided is final,
    //     survivors are taken in front of the first undecided maximum only;
    //   prominence and width: wave_peak_ok_win (find_peaks.h), three-valued;
    //   the read: an unknown maximum met before the second survivor, fewer than two survivors, or (recount) a plateau that reaches the
    //     window's end leave the read UNDECIDED -- nothing is written for it, its index goes to the redo list (redo[0]: count, zeroed
    //     by the host; redo[1 ..]: reads), and k_gains<2> / this kernel run again over the list with the whole trace (redo_pass = 1).
    //   A decided read's p0 < p1 and g[p0 .. p1] lie inside the window: step 5 is the whole trace's.
    int n_decided = 0, n_listed = 0; // (g_dbg[78] / g_dbg[79]: windowed reads decided in the window / sent to the redo list)
    const int n_work = redo_pass ? redo[0] : n_reads;
    for (int wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
        const int r = redo_pass ? redo[1 + wi] : wi;
        int32_t *pk = pk_all + (size_t)r * half; // per-read list, pre-filled by k_gains
        int result = 0;
        const int n = nvalid[r];
        const bool active = mbs[r / mbsize].status == ADP_MB_OK && adapter_idx[r] >= 0 && n >= 3;
        bool undecided = false;
        if (active) {
            const double *g = trace + (size_t)r * Lp;
            const int wend = (wend_all && !redo_pass) ? min(wend_all[r], n) : n; // the trace is known on [0, wend)
            const bool win = wend < n;
            TraceView tv{g, bmax + (size_t)r * nsum, bmin + (size_t)r * nsum, 0, wend - 1, 1};
            // 1. all local maxima, in index order: normally found by k_gains while the trace tile was in LDS;
            //    recounted here (one load per lane, neighbours by shuffle) when a plateau was met
            int npk = npk_all[r];
            const bool recount = npk < 0;
            // heights of the listed maxima as k_gains wrote them (none after a recount: gathered from the trace then)
            const double *pkv = (pkv_all && !recount) ? pkv_all + (size_t)r * half : nullptr;
            if (recount) npk = 0;
            double carry = 0.0; // value at base - 1
            __syncthreads();
            for (int base0 = 0; recount && base0 < wend; base0 += 256) {
                double vv[4], ee[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { // four tiles in flight
                    const int i = base0 + u * 64 + ln;
                    vv[u] = (i < wend) ? tv_get(tv, i) : 0.0;
                    ee[u] = (ln == 63 && i + 1 < wend) ? tv_get(tv, i + 1) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int base = base0 + u * 64;
                    if (base >= wend) break;
                    const int i = base + ln;
                    const double v = vv[u];
                    double prev = __shfl_up(v, 1);
                    if (ln == 0) prev = carry;
                    double next = __shfl_down(v, 1);
                    if (ln == 63) next = ee[u];
                    carry = __shfl(v, 63);
                    int p = -1;
                    if (i > 0 && i < wend - 1 && prev < v) {
                        if (next < v) p = i;
                        else if (next == v) { // plateau: walk to its end (rare on float64 traces)
                            int j = i + 1;
                            while (j < wend - 1 && tv_get(tv, j) == v) j++;
                            if (tv_get(tv, j) < v) p = (i + j - 1) / 2;
                            else if (win && tv_get(tv, j) == v) undecided = true; // (it reaches the window's end: its midpoint is unknown)
                        }
                    }
                    unsigned long long m = __ballot(p >= 0);
                    if (p >= 0) pk[npk + __popcll(m & ((1ull << ln) - 1ull))] = p;
                    npk += __popcll(m);
                }
            }
            undecided = __any(undecided);
            if (ABLATED(256)) npk = 0;
            // Only the first two survivors in index order are wanted, and they lie near the front of almost every trace: steps 2-4 run
            // on a PREFIX of the list first (the first wn maxima; the maxima behind it read as undecided, so a state that depends on
            // them stays undecided -- whatever is decided is final: the fixed point is unique).  The answer stands when the second
            // survivor was found among maxima in front of the first undecided one; otherwise the steps run again on the whole list.
            int p0 = -1, p1 = -1;
            for (int attempt = 0; attempt < 2; attempt++) {
            const int wn = (attempt == 0 && prefix > 0 && npk > prefix) ? prefix : npk;
            __syncthreads();
            for (int w = ln; w < (wn + 8 + 15) / 16 + 1; w += 64) stw[w] = 0;
            __syncthreads();
            if (ln < 4 && wn + ln < npk) { // (ordinals wn .. wn + 3: neighbours of the prefix's last maxima)
                const uint32_t sl = (uint32_t)(wn + ln + 4);
                __hip_atomic_fetch_or(&stw[sl >> 4], PST_UNDECIDED << ((sl & 15u) * 2u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            // 2. per maximum: which of the up to 8 maxima within +-9 samples have a higher priority
            //    (scipy _select_by_peak_distance, distance = 10 -> |dp| < 10; equal heights: later index first).
            //    56 maxima per step (lanes 4..59), their neighbours by shuffle.  A maximum without any is kept
            //    at once; the others form the work list of step 3.
            int nund = 0;
            // (four steps' positions, then their four trace values, are requested together: a step is two dependent round
            // trips to memory -- the list entry, then the trace value it points at -- and a read has up to 180 steps)
            for (int base4 = 0; base4 < wn; base4 += 56 * 4) {
                int pp[4];
                double vv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = base4 + 56 * u - 4 + ln;
                    const bool valid = k >= 0 && k < npk;
                    pp[u] = valid ? pk[k] : (k < 0 ? -0x40000000 : 0x40000000);
                }
                if (pkv) { // (uniform) positions and heights are independent loads: one round trip per step instead of two
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int k = base4 + 56 * u - 4 + ln;
                        const bool valid = k >= 0 && k < npk;
                        vv[u] = valid ? pkv[k] : 0.0;
                    }
                } else {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = base4 + 56 * u - 4 + ln;
                    const bool valid = k >= 0 && k < npk;
                    vv[u] = valid ? tv_get(tv, pp[u]) : 0.0;
                }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int base = base4 + 56 * u;
                    if (base >= wn) break;
                    const int k = base - 4 + ln;
                    const bool valid = k >= 0 && k < npk;
                    const int p = pp[u];
                    const double v = vv[u];
                    // forward neighbours k+j by shuffle; the backward relation of k to k-j is the forward one seen from
                    // k-j with the comparison reversed (the sanitised values hold no NaN), so it travels as one bit
                    uint32_t mask = 0, lower = 0; // lower bit j-1: k+j lies within 9 samples and is LOWER than k
#pragma unroll
                    for (int j = 1; j <= 4; j++) {
                        const int pf = __shfl_down(p, j); const double vf = __shfl_down(v, j);
                        const bool within = pf - p <= 9;
                        if (within && vf >= v) mask |= 1u << (j - 1);
                        if (within && !(vf >= v)) lower |= 1u << (j - 1);
                    }
#pragma unroll
                    for (int j = 1; j <= 4; j++) {
                        const uint32_t lb = (uint32_t)__shfl_up((int)lower, j);
                        if (lb >> (j - 1) & 1u) mask |= 1u << (4 + j - 1); // k-j is within 9 and k is lower than it
                    }
                    const bool out = valid && ln >= 4 && ln < 60 && k < wn;
                    const bool late = win && p >= wend - 10; // (a neighbour within 9 samples may lie behind the window)
                    if (out) {
                        const uint32_t sl = (uint32_t)(k + 4);
                        __hip_atomic_fetch_or(&stw[sl >> 4], ((mask || late) ? PST_UNDECIDED : PST_KEPT) << ((sl & 15u) * 2u), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    const bool und = out && mask && !late;
                    const unsigned long long m = __ballot(und);
                    if (und) mk[nund + __popcll(m & ((1ull << ln) - 1ull))] = ((uint32_t)k << 8) | mask;
                    nund += __popcll(m);
                }
            }
            __syncthreads();
            // 3. fixed point of "kept iff no kept higher-priority neighbour"
            if (ABLATED(512)) nund = 0;
            while (nund > 0) {
                int w = 0;
                for (int base4 = 0; base4 < nund; base4 += 256) { // (four list loads in flight; the rewritten list stays
                    uint32_t ee[4];                                 //  below what has been read)
#pragma unroll
                    for (int u = 0; u < 4; u++) { const int idx = base4 + 64 * u + ln; ee[u] = (idx < nund) ? mk[idx] : 0u; }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int base = base4 + 64 * u;
                        if (base >= nund) break;
                        const int idx = base + ln;
                        const uint32_t e = ee[u];
                        bool pending = false;
                        if (idx < nund) {
                            const uint32_t k = e >> 8;
                            // states of the ordinals k-4 .. k+4 = slots k .. k+8
                            const unsigned long long W =
                                (((unsigned long long)stw[(k >> 4) + 1] << 32) | stw[k >> 4]) >> ((k & 15u) * 2u);
                            bool kept_nb = false;
                            uint32_t b = e & 255u;
                            while (b) {
                                const int o = __ffs(b) - 1; b &= b - 1;
                                const int f = o < 4 ? 5 + o : 7 - o; // k+1..k+4 -> fields 5..8 ; k-1..k-4 -> fields 3..0
                                const uint32_t sn = (uint32_t)(W >> (2 * f)) & 3u;
                                if (sn == PST_KEPT) kept_nb = true;
                                else if (sn == PST_UNDECIDED) pending = true;
                            }
                            const uint32_t sl = k + 4u;
                            if (kept_nb) {
                                __hip_atomic_fetch_and(&stw[sl >> 4], ~(2u << ((sl & 15u) * 2u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                pending = false;
                            } else if (!pending) {
                                __hip_atomic_fetch_and(&stw[sl >> 4], ~(1u << ((sl & 15u) * 2u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                        const unsigned long long m = __ballot(pending);
                        if (pending) mk[w + __popcll(m & ((1ull << ln) - 1ull))] = e;
                        w += __popcll(m);
                        __syncthreads();
                    }
                }
                if (w == nund) break; // (a prefix: what is left waits for maxima behind it)
                nund = w;
            }
            __syncthreads();
            // kept maxima in front of the first undecided one, in index order, into the work list's place (it is dead by now)
            int32_t *kl = reinterpret_cast<int32_t *>(mk);
            int nkept = 0, first_und = wn;
            for (int base4 = 0; base4 < wn && first_und == wn; base4 += 256) { // (four loads in flight)
                int pq[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const int k = base4 + 64 * u + ln; pq[u] = (k < wn) ? pk[k] : -1; }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = base4 + 64 * u + ln;
                    uint32_t stt = PST_NONE;
                    if (k < wn) {
                        const uint32_t sl = (uint32_t)(k + 4);
                        stt = (stw[sl >> 4] >> ((sl & 15u) * 2u)) & 3u;
                    }
                    const unsigned long long mu = __ballot(stt == PST_UNDECIDED);
                    if (mu && first_und == wn) first_und = base4 + 64 * u + __ffsll((long long)mu) - 1;
                    const bool kp = stt == PST_KEPT && k < first_und;
                    const unsigned long long m = __ballot(kp);
                    if (kp) kl[nkept + __popcll(m & ((1ull << ln) - 1ull))] = pq[u];
                    nkept += __popcll(m);
                }
            }
            __syncthreads();
            // 4. survivors in index order: prominence >= 1, width(rel 0.5) >= 10; first two
            // survivors, compacted in index order (LDS state scan), then 64 candidates per step
            p0 = -1; p1 = -1;
            // (16 candidates per step: the second survivor is among the first 32 kept maxima of almost every read, and
            // every candidate with a long walk costs the whole wave a cooperative scan)
            for (int base = 0; base < nkept && p1 < 0 && !undecided && !ABLATED(1024); base += PK_STEP) {
                int k = base + ln;
                int i = (ln < PK_STEP && k < nkept) ? kl[k] : -1;
                int ok3;
                if (win) ok3 = wave_peak_ok_win(tv, i, 1.0, 10.0, 0.5);
                else ok3 = wave_peak_ok(tv, i, 1.0, 10.0, 0.5) ? PK3_PASS : PK3_FAIL;
                unsigned long long m = __ballot(ok3 != PK3_FAIL);
                const unsigned long long unk = __ballot(ok3 == PK3_UNKNOWN);
                while (m && p1 < 0) {
                    int f = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (unk >> f & 1ull) { undecided = true; break; } // (in index order: an unknown in front of the second survivor)
                    int pi = __shfl(i, f);
                    if (p0 < 0) p0 = pi; else p1 = pi;
                }
            }
            if (p1 >= 0 || first_und >= npk || undecided) break; // (else: the prefix did not settle it)
            }
            if (win && p1 < 0) undecided = true; // (a survivor may lie behind the window)
            // 5. spike heuristics on the UN-sanitised trace
            if (undecided) {
                n_listed++;
                if (ln == 0) redo[1 + atomicAdd(&redo[0], 1)] = r;
            } else if (p0 >= 0 && p1 < 0) result = p0;
            else if (p0 >= 0) {
                double h0 = g[p0], h1 = g[p1];
                if (h1 > h0) result = p1;
                else if (h1 < h0 * 0.5) result = p0;
                else {
                    // idx_min = argmin(g[p0:p1]) (first minimum; a NaN wins)
                    double mv = __builtin_inf(); int mi = 0x7fffffff; int nan_i = 0x7fffffff;
                    for (int i = p0 + ln; i < p1; i += 64) {
                        double v = g[i];
                        if (v != v) nan_i = min(nan_i, i);
                        else if (v < mv) { mv = v; mi = i; }
                    }
                    nan_i = wave_min(nan_i);
                    double gm = wave_min(mv);
                    int cand = (mv == gm) ? mi : 0x7fffffff;
                    cand = wave_min(cand);
                    int idx_min = (nan_i != 0x7fffffff) ? nan_i : cand;
                    if (idx_min == 0x7fffffff) idx_min = p0; // all +inf: np.argmin -> 0
                    int cnt = p1 - idx_min;
                    // scipy.stats.linregress r-value
                    double sx = 0, sy = 0;
                    for (int i = idx_min + ln; i < p1; i += 64) { sx += (double)i; sy += g[i]; }
                    sx = wave_sum(sx); sy = wave_sum(sy);
                    double xm = sx / cnt, ym = sy / cnt;
                    double sxx = 0, sxy = 0, syy = 0;
                    for (int i = idx_min + ln; i < p1; i += 64) {
                        double dx = (double)i - xm, dy = g[i] - ym;
                        sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
                    }
                    sxx = wave_sum(sxx); sxy = wave_sum(sxy); syy = wave_sum(syy);
                    double inv = 1.0 / (double)cnt;
                    double ssxm = sxx * inv, ssxym = sxy * inv, ssym = syy * inv;
                    double rr;
                    if (ssxm == 0.0 || ssym == 0.0) rr = 0.0;
                    else { rr = ssxym / sqrt(ssxm * ssym); if (rr > 1.0) rr = 1.0; else if (rr < -1.0) rr = -1.0; }
                    result = (rr * rr >= 0.99) ? p1 : 0;
                }
            }
            if (win && !undecided) n_decided++;
            __syncthreads();
        }
        if (ln == 0 && !undecided) polya_idx[r] = result;
    }
    if (ln == 0 && n_decided) atomicAdd(&g_dbg[78], (unsigned long long)n_decided);
    if (ln == 0 && n_listed) atomicAdd(&g_dbg[79], (unsigned long long)n_listed);
}
