// find_peaks.h -- scipy.signal.find_peaks on a trace, restated for one wave (the algorithm: peaks.h's header comment): views
// of a trace, strict local maxima, the cooperative walks, prominence and width within a budget of steps.  Used by the fused
// kernels of the detect path (peaks.h) and by the LLR module's kernels (trace_peaks_api.h); no kernels and no device variables here.
#pragma once
#include "common.h"

#define DBLMAX 1.7976931348623157e308

// P: `const double *` (the trace in global memory) or `const LDS double *` (a short trace staged in LDS: every walk below is a chain
// of dependent loads, a memory round trip each from HBM / L2)
template <class P>
struct TraceViewT {
    P x;                 // trace of one read (full-trace coordinates)
    P bmax;              // per-64 block max (NaN -> +inf) or nullptr
    P bmin;              // per-64 block min or nullptr
    int lo, hi;          // inclusive index bounds of the array find_peaks sees
    int sanitize;        // apply np.nan_to_num(nan=0) on load
};
typedef TraceViewT<const double *> TraceView;
typedef TraceViewT<const LDS double *> TraceViewL;

template <class TV>
static __device__ __forceinline__ double tv_get(const TV &t, int i)
{
    double v = t.x[i];
    if (t.sanitize) {
        if (v != v) v = 0.0;
        else if (__builtin_isinf(v)) v = v > 0 ? DBLMAX : -DBLMAX;
    }
    return v;
}

// Is full-trace index i the left edge of a strict local maximum (scipy _local_maxima_1d)?
// Returns the plateau midpoint or -1.
template <class TV>
static __device__ __forceinline__ int tv_peak_at(const TV &t, int i)
{
    if (i <= t.lo || i >= t.hi) return -1;
    double xi = tv_get(t, i);
    if (!(tv_get(t, i - 1) < xi)) return -1;
    int j = i + 1;
    while (j < t.hi && tv_get(t, j) == xi) j++;
    if (tv_get(t, j) < xi) return (i + j - 1) / 2;
    return -1;
}

// scipy's _peak_widths walks from the peak towards each side's prominence BASE -- the first sample, going away from the
// peak, that attains the side's minimum -- and stops there at the latest.  At rel_height = 1 the evaluation height
// x[p] - prominence is that minimum up to rounding, so whether the walk ends by value or at the base is decided by the last
// bit: the walks below carry the two side minima and stop on a sample EQUAL to its side's minimum as well as on one at or
// below the height (equivalent to carrying the base indices).

// ---- long walks, cooperatively ------------------------------------------------------------------------
// The dominant peak of a trace has nothing higher on either side: its prominence walk runs to the ends of the
// trace (hundreds of dependent steps in ONE lane while 63 wait), and its width walk is long too.  A lane whose
// private walk is not done within a budget hands the peak to the whole wave: 64 summary blocks (or the 64 samples
// of one block) are tested per step.
enum { WALK_PROM = 0, WALK_WIDTH = 1 };

template <int KIND>
static __device__ __forceinline__ bool walk_block_clean(double bmx, double bmn, double xp, double height, double smin)
{
    return KIND == WALK_PROM ? (bmx <= xp) : (bmn > height && bmn > smin && bmx <= xp);
}
template <int KIND>
static __device__ __forceinline__ bool walk_hit(double v, double xp, double height, double smin)
{
    return KIND == WALK_PROM ? !(v <= xp) : (!(height < v) || v == smin);
}

// nearest j in [limit, start], searching downwards, with walk_hit(x[j]); limit - 1 if none.  mn (WALK_PROM):
// minimum of the samples passed, i.e. those above j.  Uniform call (all lanes, same arguments).
template <int KIND, class TV>
static __device__ int coop_find_down(const TV &t, int start, int limit, double xp, double height, double &mn, double smin = 0.0)
{
    const int ln = lane_id();
    double lmn = xp;
    int i = start, found = limit - 1;
    while (i >= limit) {
        int b = i / SUMBLK, bstart = b * SUMBLK;
        if (t.bmax && i == bstart + SUMBLK - 1 && bstart >= limit) {
            // up to 64 whole blocks at once: lane l looks at block b - l
            const int bb = b - ln;
            const bool whole = bb >= 0 && bb * SUMBLK >= limit;
            const double bmx = whole ? t.bmax[bb] : 0.0, bmn = whole ? t.bmin[bb] : 0.0;
            const bool dirty = !whole || !walk_block_clean<KIND>(bmx, bmn, xp, height, smin);
            const unsigned long long m = __ballot(dirty);
            const int first = m ? __ffsll((long long)m) - 1 : 64;
            if (KIND == WALK_PROM && ln < first && bmn < lmn) lmn = bmn;
            b -= first; bstart = b * SUMBLK;
            i = bstart + SUMBLK - 1;
            if (first == 64 || i < limit) continue;
        }
        // the samples of block b within [limit, i]
        const int e = bstart + ln;
        const bool in = e >= limit && e <= i;
        const double v = in ? tv_get(t, e) : 0.0;
        const unsigned long long m = __ballot(in && walk_hit<KIND>(v, xp, height, smin));
        if (m) {
            found = bstart + 63 - __clzll((long long)m);
            if (KIND == WALK_PROM && in && e > found && v < lmn) lmn = v;
            break;
        }
        if (KIND == WALK_PROM && in && v < lmn) lmn = v;
        i = bstart - 1;
    }
    if (KIND == WALK_PROM) mn = wave_min(lmn);
    return found;
}

// nearest j in [start, limit], searching upwards; limit + 1 if none
template <int KIND, class TV>
static __device__ int coop_find_up(const TV &t, int start, int limit, double xp, double height, double &mn, double smin = 0.0)
{
    const int ln = lane_id();
    double lmn = xp;
    int i = start, found = limit + 1;
    while (i <= limit) {
        int b = i / SUMBLK, bstart = b * SUMBLK;
        if (t.bmax && i == bstart && bstart + SUMBLK - 1 <= limit) {
            const int bb = b + ln;
            const bool whole = bb * SUMBLK + SUMBLK - 1 <= limit;
            const double bmx = whole ? t.bmax[bb] : 0.0, bmn = whole ? t.bmin[bb] : 0.0;
            const bool dirty = !whole || !walk_block_clean<KIND>(bmx, bmn, xp, height, smin);
            const unsigned long long m = __ballot(dirty);
            const int first = m ? __ffsll((long long)m) - 1 : 64;
            if (KIND == WALK_PROM && ln < first && bmn < lmn) lmn = bmn;
            b += first; bstart = b * SUMBLK;
            i = bstart;
            if (first == 64 || i > limit) continue;
        }
        const int e = bstart + ln;
        const bool in = e >= i && e <= limit;
        const double v = in ? tv_get(t, e) : 0.0;
        const unsigned long long m = __ballot(in && walk_hit<KIND>(v, xp, height, smin));
        if (m) {
            found = bstart + __ffsll((long long)m) - 1;
            if (KIND == WALK_PROM && in && e < found && v < lmn) lmn = v;
            break;
        }
        if (KIND == WALK_PROM && in && v < lmn) lmn = v;
        i = bstart + SUMBLK;
    }
    if (KIND == WALK_PROM) mn = wave_min(lmn);
    return found;
}

// the walks of tv_prominence / tv_width with a step budget.  WALK_CHUNK samples are
// loaded per round trip to memory (the loads do not depend on the comparisons), then examined in walk order.
#ifndef WALK_CHUNK
#define WALK_CHUNK 4
#endif
// Result: PB_DONE (both walks ended: prom exact), PB_REJECT (a COMPLETED side's minimum already shows prominence < pmin: the prominence
// is xp - max(left_min, right_min) <= xp - either minimum, in floating point too, so whatever the other side holds the test
// pmin <= prominence fails -- the noise maxima of a rising or falling stretch, whose walk on the far side would run on to the end of
// the trace, leave here), or PB_LEFT / PB_RIGHT bits: that side's walk was cut short by the budget (its minimum so far is not final).
// WIN (a trace known on [lo, hi] only, the windowed pass 2: wave_peak_ok_win below): PB_OPEN says that the right walk reached hi
// without meeting a higher sample -- its minimum is an upper bound of the side's true one, and shows nothing about the prominence.
enum { PB_DONE = 0, PB_LEFT = 1, PB_RIGHT = 2, PB_REJECT = 4, PB_OPEN = 8 };
template <bool WIN = false, class TV>
static __device__ int tv_prominence_budget(const TV &t, int p, int budget, double pmin, double &prom, double &lmin_out, double &rmin_out)
{
    const double xp = tv_get(t, p);
    double left_min = xp, right_min = xp;
    int more = 0;
    bool stopped = false;
    for (int i0 = p, steps = 0; !stopped && i0 >= t.lo; i0 -= WALK_CHUNK, steps += WALK_CHUNK) {
        if (steps >= budget) { more |= PB_LEFT; break; }
        double v[WALK_CHUNK];
#pragma unroll
        for (int u = 0; u < WALK_CHUNK; u++) v[u] = (i0 - u >= t.lo) ? tv_get(t, i0 - u) : 0.0;
#pragma unroll
        for (int u = 0; u < WALK_CHUNK; u++) {
            if (!stopped) {
                if (i0 - u < t.lo || !(v[u] <= xp)) stopped = true;
                else if (v[u] < left_min) left_min = v[u];
            }
        }
    }
    if (!(more & PB_LEFT) && !(pmin <= xp - left_min)) return PB_REJECT;
    stopped = false;
    bool higher = false; // (WIN) the right walk ended at a higher sample
    for (int i0 = p, steps = 0; !stopped && i0 <= t.hi; i0 += WALK_CHUNK, steps += WALK_CHUNK) {
        if (steps >= budget) { more |= PB_RIGHT; break; }
        double v[WALK_CHUNK];
#pragma unroll
        for (int u = 0; u < WALK_CHUNK; u++) v[u] = (i0 + u <= t.hi) ? tv_get(t, i0 + u) : 0.0;
#pragma unroll
        for (int u = 0; u < WALK_CHUNK; u++) {
            if (!stopped) {
                if (i0 + u > t.hi || !(v[u] <= xp)) { stopped = true; if (WIN && i0 + u <= t.hi) higher = true; }
                else if (v[u] < right_min) right_min = v[u];
            }
        }
    }
    if (WIN && !(more & PB_RIGHT) && !higher) more |= PB_OPEN;
    if (!(more & (WIN ? PB_RIGHT | PB_OPEN : PB_RIGHT)) && !(pmin <= xp - right_min)) return PB_REJECT;
    prom = xp - (left_min > right_min ? left_min : right_min);
    lmin_out = left_min; rmin_out = right_min;
    return more;
}
// WIN: a right walk that ends at hi without a sample at or below the height leaves width = NaN (the crossing lies behind the window)
template <bool WIN = false, class TV>
static __device__ bool tv_width_budget(const TV &t, int p, double prom, double rel, int budget, double &width, double lmin, double rmin)
{
    const double xp = tv_get(t, p);
    const double height = xp - prom * rel;
    // left: the first index i (descending from p, i > lo) with !(height < x[i]); lo if none
    int il = t.lo;
    {
        bool stopped = false;
        for (int i0 = p, steps = 0; !stopped && i0 > t.lo; i0 -= WALK_CHUNK, steps += WALK_CHUNK) {
            if (steps >= budget) return false;
            double v[WALK_CHUNK];
#pragma unroll
            for (int u = 0; u < WALK_CHUNK; u++) v[u] = (i0 - u > t.lo) ? tv_get(t, i0 - u) : 0.0;
#pragma unroll
            for (int u = 0; u < WALK_CHUNK; u++) {
                if (!stopped) {
                    if (i0 - u <= t.lo) { stopped = true; il = t.lo; }
                    else if (!(height < v[u]) || v[u] == lmin) { stopped = true; il = i0 - u; }
                }
            }
        }
    }
    int ir = t.hi;
    bool crossed = false; // (WIN)
    {
        bool stopped = false;
        for (int i0 = p, steps = 0; !stopped && i0 < t.hi; i0 += WALK_CHUNK, steps += WALK_CHUNK) {
            if (steps >= budget) return false;
            double v[WALK_CHUNK];
#pragma unroll
            for (int u = 0; u < WALK_CHUNK; u++) v[u] = (i0 + u < t.hi) ? tv_get(t, i0 + u) : 0.0;
#pragma unroll
            for (int u = 0; u < WALK_CHUNK; u++) {
                if (!stopped) {
                    if (i0 + u >= t.hi) { stopped = true; ir = t.hi; }
                    else if (!(height < v[u]) || v[u] == rmin) { stopped = true; ir = i0 + u; crossed = true; }
                }
            }
        }
    }
    double left_ip = (double)il, right_ip = (double)ir;
    { double xi = tv_get(t, il); if (xi < height) left_ip += (height - xi) / (tv_get(t, il + 1) - xi); }
    { double xi = tv_get(t, ir); if (xi < height) right_ip -= (height - xi) / (tv_get(t, ir - 1) - xi); }
    width = right_ip - left_ip;
    if (WIN && !crossed) width = __builtin_nan("");
    return true;
}

// Per lane: does the local maximum p (or -1: none) pass prominence >= pmin and width(rel) >= wmin?
// Uniform call.  Short walks run privately in each lane, long ones cooperatively, one peak at a time.
// (round 4, with the certain-reject exit of tv_prominence_budget: budget x chunk 48 x 8 -> 8 x 4; 96 000 reads, k_adapter_peak / k_polya_peak:
// 2.2 / 2.25 -> 1.1 / 1.57 ms at the preset's 16 k window, 2.33 / 5.65 -> 1.2 / 5.12 ms at the 200 k window; 8 x 8, 12 x 4, 16 x 8 within 5 %,
// 0 (every walk cooperative) 1.6 / 2.16, 96 x 8 3.4 / 2.9 -- tools/ab_libs.sh)
#ifndef WALK_BUDGET
#define WALK_BUDGET 8
#endif
template <class TV>
static __device__ bool wave_peak_ok(const TV &t, int p, double pmin, double wmin, double rel)
{
    const int ln = lane_id();
    double prom = 0.0, lmn = 0.0, rmn = 0.0; // prominence and the minima of the two sides (the values at the bases)
    bool have = p >= 0, done = true;
    int pb = PB_DONE;
    if (have) pb = tv_prominence_budget(t, p, WALK_BUDGET, pmin, prom, lmn, rmn);
    if (pb == PB_REJECT) have = false;
    unsigned long long todo = __ballot(have && pb != PB_DONE);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int pp = __shfl(p, src), sides = __shfl(pb, src);
        const double xp = tv_get(t, pp);
        double lmin = __shfl(lmn, src), rmin = __shfl(rmn, src); // (a side whose private walk ended keeps its minimum)
        bool rej = false;
        if (sides & PB_LEFT) { coop_find_down<WALK_PROM>(t, pp, t.lo, xp, 0.0, lmin); rej = !(pmin <= xp - lmin); } // (as PB_REJECT; uniform)
        if (!rej && (sides & PB_RIGHT)) coop_find_up<WALK_PROM>(t, pp, t.hi, xp, 0.0, rmin);
        if (ln == src) { if (rej) have = false; else { prom = xp - (lmin > rmin ? lmin : rmin); lmn = lmin; rmn = rmin; } }
    }
    bool cand = have && (pmin <= prom);
    double width = 0.0;
    done = true;
    if (cand) done = tv_width_budget(t, p, prom, rel, WALK_BUDGET, width, lmn, rmn);
    todo = __ballot(cand && !done);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int pp = __shfl(p, src);
        const double pr = __shfl(prom, src);
        const double sl = __shfl(lmn, src), sr = __shfl(rmn, src);
        const double xp = tv_get(t, pp);
        const double height = xp - pr * rel;
        double dummy;
        int il = coop_find_down<WALK_WIDTH>(t, pp, t.lo + 1, xp, height, dummy, sl);
        if (il < t.lo + 1) il = t.lo;
        int ir = coop_find_up<WALK_WIDTH>(t, pp, t.hi - 1, xp, height, dummy, sr);
        if (ir > t.hi - 1) ir = t.hi;
        double left_ip = (double)il, right_ip = (double)ir;
        { double xi = tv_get(t, il); if (xi < height) left_ip += (height - xi) / (tv_get(t, il + 1) - xi); }
        { double xi = tv_get(t, ir); if (xi < height) right_ip -= (height - xi) / (tv_get(t, ir - 1) - xi); }
        if (ln == src) width = right_ip - left_ip;
    }
    return cand && (wmin <= width);
}

// ---- a trace known on a window only ------------------------------------------------------------------------
// The windowed pass 2 (llr_stream.h) computes x[0 .. wend) of a longer trace: t.lo = 0 is the trace's true start, t.hi = wend - 1
// the last KNOWN sample, and what lies behind it is unknown.  wave_peak_ok's question then has three answers per maximum:
// PK3_FAIL / PK3_PASS are what the whole trace would say, PK3_UNKNOWN is everything that cannot be shown from the window (the
// caller computes the whole trace for that read, so an unknown costs time and never a wrong answer).  With h = x[p], lmin the left
// walk's minimum (always exact: the trace is known back to its start) and rp the right walk's minimum:
//   * the right walk met a higher sample inside the window: both minima are exact, and so is everything below.
//   * it reached the window's end (PB_OPEN); the true right minimum is <= rp.
//       rp <= lmin: the prominence is h - max(lmin, true right minimum) = h - lmin, exactly.  The evaluation height h - prom rel
//         must lie above rp (else: unknown); then the right crossing comes no later than the sample that attains rp, inside the
//         window, and a right base stop `v == true minimum` could only fire on a sample <= rp, which is below the height and stops
//         the walk anyway -- the width is exact.
//       rp > lmin: the prominence lies in [h - rp, h - lmin]; h - lmin < pmin was rejected when the left side completed.
//         The width is non-decreasing in the prominence: a lower evaluation height moves the left crossing left and the right one
//         right, whole samples first and within a sample by the interpolation, whose pieces -- h - prom rel, (height - xi) /
//         (x[il+1] - xi), index +- quotient -- are each monotone under rounding.  Lower bound h - rp: its height lies above rp
//         (else: unknown), so the right crossing is inside the window, and both base stops are idle (lmin < rp < height);
//         pmin <= h - rp and wmin <= width(h - rp): PASS.  Upper bound h - lmin, walked with the known left base and NO right
//         base stop (the walk without one goes at least as far): both crossings inside the window and width(h - lmin) < wmin: FAIL.
//         Anything else: unknown.
//   * a width walk that reaches the window's end without a crossing: unknown, whatever the prominence.
enum { PK3_FAIL = 0, PK3_PASS = 1, PK3_UNKNOWN = 2 };

// width at `height` of the maximum pp, cooperatively (uniform call); sl / sr: the base stops (-inf: none).  crossed: the right
// crossing was found in front of t.hi
template <class TV>
static __device__ double coop_width(const TV &t, int pp, double xp, double height, double sl, double sr, bool &crossed)
{
    double dummy;
    int il = coop_find_down<WALK_WIDTH>(t, pp, t.lo + 1, xp, height, dummy, sl);
    if (il < t.lo + 1) il = t.lo;
    int ir = coop_find_up<WALK_WIDTH>(t, pp, t.hi - 1, xp, height, dummy, sr);
    crossed = ir <= t.hi - 1;
    if (!crossed) ir = t.hi;
    double left_ip = (double)il, right_ip = (double)ir;
    { double xi = tv_get(t, il); if (xi < height) left_ip += (height - xi) / (tv_get(t, il + 1) - xi); }
    { double xi = tv_get(t, ir); if (xi < height) right_ip -= (height - xi) / (tv_get(t, ir - 1) - xi); }
    return right_ip - left_ip;
}

// Per lane: PK3_* for the local maximum p (or -1: none, PK3_FAIL).  Uniform call; p + 10 <= t.hi + 1 is the caller's distance rule.
template <class TV>
static __device__ int wave_peak_ok_win(const TV &t, int p, double pmin, double wmin, double rel)
{
    const int ln = lane_id();
    double prom = 0.0, lmn = 0.0, rmn = 0.0;
    bool have = p >= 0;
    int pb = PB_DONE;
    if (have) pb = tv_prominence_budget<true>(t, p, WALK_BUDGET, pmin, prom, lmn, rmn);
    if (pb == PB_REJECT) { have = false; pb = PB_DONE; }
    unsigned long long todo = __ballot(have && (pb & (PB_LEFT | PB_RIGHT)));
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int pp = __shfl(p, src), sides = __shfl(pb, src);
        const double xp = tv_get(t, pp);
        double lmin = __shfl(lmn, src), rmin = __shfl(rmn, src);
        bool rej = false;
        int open = sides & PB_OPEN;
        if (sides & PB_LEFT) { coop_find_down<WALK_PROM>(t, pp, t.lo, xp, 0.0, lmin); rej = !(pmin <= xp - lmin); }
        if (!rej && (sides & PB_RIGHT)) { if (coop_find_up<WALK_PROM>(t, pp, t.hi, xp, 0.0, rmin) > t.hi) open = PB_OPEN; }
        if (ln == src) { if (rej) have = false; else { lmn = lmin; rmn = rmin; pb = open; } }
    }
    const double xpl = have ? tv_get(t, p) : 0.0;
    const bool bounds = have && (pb & PB_OPEN) && rmn > lmn; // the prominence is known as an interval only
    prom = xpl - (lmn > rmn ? lmn : rmn);
    const bool cand = have && !bounds && (pmin <= prom);
    int res = PK3_FAIL;
    double width = 0.0;
    bool done = true;
    if (cand) done = tv_width_budget<true>(t, p, prom, rel, WALK_BUDGET, width, lmn, rmn);
    todo = __ballot(cand && !done);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int pp = __shfl(p, src);
        const double pr = __shfl(prom, src);
        const double sl = __shfl(lmn, src), sr = __shfl(rmn, src);
        const double xp = tv_get(t, pp);
        bool crossed;
        const double w = coop_width(t, pp, xp, xp - pr * rel, sl, sr, crossed);
        if (ln == src) width = crossed ? w : __builtin_nan("");
    }
    if (cand) {
        const double height = xpl - prom * rel;
        if (width != width || ((pb & PB_OPEN) && !(rmn < height))) res = PK3_UNKNOWN;
        else res = (wmin <= width) ? PK3_PASS : PK3_FAIL;
    }
    todo = __ballot(bounds);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int pp = __shfl(p, src);
        const double sl = __shfl(lmn, src), sr = __shfl(rmn, src);
        const double xp = tv_get(t, pp);
        int rs = PK3_UNKNOWN;
        bool crossed;
        const double plo = xp - sr, phi = xp - sl;
        if (pmin <= plo) {
            const double hlo = xp - plo * rel;
            if (sr < hlo) { const double w = coop_width(t, pp, xp, hlo, sl, sr, crossed); if (crossed && wmin <= w) rs = PK3_PASS; }
        }
        if (rs == PK3_UNKNOWN) {
            const double w = coop_width(t, pp, xp, xp - phi * rel, sl, -__builtin_inf(), crossed);
            if (crossed && w < wmin) rs = PK3_FAIL;
        }
        if (ln == src) res = rs;
    }
    return res;
}

// First peak (lowest index) of find_peaks(x[lo..hi], prominence=pmin, width=wmin, rel_height=rel),
// in full-trace coordinates, or -1.  Wave-cooperative: call from uniform control flow.
template <class TV>
static __device__ int wave_first_peak(const TV &t, double pmin, double wmin, double rel)
{
    const int ln = lane_id();
    for (int base = t.lo + 1; base < t.hi; base += 64) {
        int i = base + ln;
        int p = (i < t.hi) ? tv_peak_at(t, i) : -1;
        const bool ok = wave_peak_ok(t, p, pmin, wmin, rel);
        unsigned long long mk = __ballot(ok);
        if (mk) return __shfl(p, __ffsll((long long)mk) - 1);
    }
    return -1;
}
