"""Pass 2 over a window of the trace (llr_stream.h, peaks.h; ADP_G2_WINDOW): the three-valued decision rule of k_polya_peak restated
in numpy, and the batches of tests/test_gpu_polya_window.py with the conditions they were made for (tests/test_polya_window_cpu.py
asserts those without a GPU).

The rule.  x = np.nan_to_num(g) is known on [0, wend), wend <= n = len(x).  wend == n is scipy's find_peaks(distance=10,
prominence=1, width=10) restated; wend < n answers FAIL / PASS per maximum where the whole trace would say the same, and UNKNOWN
otherwise; `decide` returns None (the read is undecided: the GPU computes its whole trace) or the first two survivors.
Geometry "tall" of gains_tile_fast_cases.py: L = 4100, five 1024-point tiles.  Everything returned by the cached functions is shared:
leave it unchanged."""
import functools

import numpy as np

import gains_tile_fast_cases as gc
import llr_stream_cases as lc

GEOM = gc.GEOM
TILE = 1024
N = 64
DBLMAX = float(np.finfo(np.float64).max)
FAIL, PASS, UNKNOWN = 0, 1, 2
DISTANCE, PMIN, WMIN, REL = 10, 1.0, 10.0, 0.5


def wend_of(start, win, n):
    """k_gains<2>'s window end: the tiles that hold [0, start + 1 + win), n for win <= 0"""
    if win <= 0:
        return n
    return min(n, -(-(start + 1 + win) // TILE) * TILE)


def sanitised(g):
    return np.nan_to_num(np.asarray(g, dtype=np.float64), nan=0.0, posinf=DBLMAX, neginf=-DBLMAX)


# ---------------------------------------------------------------- the rule
def maxima(x, wend):
    """-> (positions of the strict local maxima of x[:wend] with plateau midpoints, does a plateau reach the window's end).  The last
    point of the window is never a maximum: it has no known successor (for wend == len(x): scipy's rule for the last sample)"""
    n = len(x)
    v = x[:wend]
    if wend < 3:
        return np.zeros(0, dtype=np.int64), False
    rise = v[1:-1] > v[:-2]
    if not (rise & (v[2:] == v[1:-1])).any():
        return np.flatnonzero(rise & (v[1:-1] > v[2:])) + 1, False
    pos, open_ = [], False
    i, i_max = 1, wend - 1
    while i < i_max:
        if v[i - 1] < v[i]:
            j = i + 1
            while j < i_max and v[j] == v[i]:
                j += 1
            if v[j] < v[i]:
                pos.append((i + j - 1) // 2)
                i = j
            elif v[j] == v[i] and wend < n:
                open_ = True
        i += 1
    return np.array(pos, dtype=np.int64), open_


def distance_states(x, pos, wend):
    """'K' kept / 'R' removed / 'U' undecided per maximum: kept iff no kept neighbour of higher priority (height, then the later
    index) within 9 samples; a maximum at p >= wend - 10 of a windowed trace is undecided for good, and so is what depends on it"""
    n = len(x)
    h = x[pos]
    state = [None] * len(pos)
    for k in np.lexsort((pos, h))[::-1]:
        if wend < n and pos[k] >= wend - 10:
            state[k] = "U"
            continue
        s = "K"
        for j in range(max(0, k - 4), min(len(pos), k + 5)):
            if j != k and state[j] is not None and abs(int(pos[j]) - int(pos[k])) < DISTANCE:   # set already: of higher priority
                if state[j] == "K":
                    s = "R"
                    break
                if state[j] == "U":
                    s = "U"
        state[k] = s
    return state


def _width(x, p, height, lstop, rstop, hi):
    """the walks of tv_width_budget / coop_width -> (width, was the right crossing found in front of hi)"""
    il = p
    while il > 0 and height < x[il] and x[il] != lstop:
        il -= 1
    ir, crossed = p, False
    while ir < hi:
        if not (height < x[ir]) or x[ir] == rstop:
            crossed = True
            break
        ir += 1
    with np.errstate(all="ignore"):
        lip, rip = np.float64(il), np.float64(ir)
        if x[il] < height:
            lip = lip + (height - x[il]) / (x[il + 1] - x[il])
        if x[ir] < height:
            rip = rip - (height - x[ir]) / (x[ir - 1] - x[ir])
        return rip - lip, crossed


def classify(x, p, wend, why=None):
    """FAIL / PASS / UNKNOWN for the maximum p of x, known on [0, wend).  why: a list that takes the branch's name"""
    n, hi = len(x), wend - 1
    win = wend < n
    note = (lambda s: why.append(s)) if why is not None else (lambda s: None)
    with np.errstate(all="ignore"):
        h = x[p]
        i, lmin = p, h
        while i >= 0 and x[i] <= h:
            lmin = min(lmin, x[i])
            i -= 1
        i, rmin = p, h
        while i <= hi and x[i] <= h:
            rmin = min(rmin, x[i])
            i += 1
        is_open = win and i > hi
        if not (PMIN <= h - lmin):
            note("reject_left")
            return FAIL
        if not is_open or rmin <= lmin:
            prom = h - max(lmin, rmin)
            if not (PMIN <= prom):
                note("exact_prom_fail")
                return FAIL
            height = h - prom * REL
            w, crossed = _width(x, p, height, lmin, rmin, hi)
            if win and (not crossed or w != w or (is_open and not (rmin < height))):
                note("exact_prom_width_unknown")
                return UNKNOWN
            note("open_exact" if is_open else "exact")
            return PASS if WMIN <= w else FAIL
        plo, phi = h - rmin, h - lmin
        if PMIN <= plo:
            hlo = h - plo * REL
            if rmin < hlo:
                w, crossed = _width(x, p, hlo, lmin, rmin, hi)
                if crossed and WMIN <= w:
                    note("bounds_pass")
                    return PASS
        w, crossed = _width(x, p, h - phi * REL, lmin, -np.inf, hi)
        if crossed and w < WMIN:
            note("bounds_fail")
            return FAIL
        note("bounds_unknown")
        return UNKNOWN


def decide(g, wend, why=None):
    """-> None (undecided) or (p0, p1), -1 for a survivor that does not exist: the first two survivors of find_peaks(np.nan_to_num(g),
    distance=10, prominence=1, width=10) from what is known on [0, wend)"""
    x = sanitised(g)
    n = len(x)
    wend = min(wend, n)
    pos, open_plateau = maxima(x, wend)
    if open_plateau:
        return None
    state = distance_states(x, pos, wend)
    out = []
    for k, p in enumerate(pos):
        if state[k] == "U":
            break
        if state[k] != "K":
            continue
        c = classify(x, int(p), wend, why)
        if c == UNKNOWN:
            return None
        if c == PASS:
            out.append(int(p))
            if len(out) == 2:
                return out[0], out[1]
    if wend < n:
        return None
    return tuple(out + [-1, -1])[:2]


def step5(g, p0, p1):
    """the spike heuristics of detect_full_polya_trace_peak_with_spike (reference adapted/detect/llr.py:440-479) on the raw trace"""
    if p0 < 0:
        return 0
    if p1 < 0:
        return p0
    with np.errstate(all="ignore"):
        h0, h1 = g[p0], g[p1]
        if h1 > h0:
            return p1
        if h1 < h0 * 0.5:
            return p0
        i = p0 + int(np.argmin(g[p0:p1]))
        xs, ys = np.arange(i, p1, dtype=np.float64), g[i:p1]
        xm, ym = xs.mean(), ys.mean()
        ssxm, ssym, ssxym = ((xs - xm) ** 2).mean(), ((ys - ym) ** 2).mean(), ((xs - xm) * (ys - ym)).mean()
        r = 0.0 if ssxm == 0.0 or ssym == 0.0 else min(1.0, max(-1.0, ssxym / np.sqrt(ssxm * ssym)))
        return p1 if r * r >= 0.99 else 0


def whole(oracle, g):
    """the first two peaks the oracle's find_peaks gives on the whole trace"""
    pk = oracle.find_peaks(sanitised(g), distance=DISTANCE, prominence=PMIN, width=WMIN, rel_height=REL)
    return tuple([int(v) for v in pk[:2]] + [-1, -1])[:2]


# ---------------------------------------------------------------- the batches
def _compose(rng, base_row, a_len, p_len, a_end, p_end, m):
    """a synth read with its adapter stretched to a_end samples and its poly(A) to p_end (adapter-like / poly(A)-like noise)"""
    out = np.empty(m, dtype=np.float32)
    out[:a_len] = base_row[:a_len]
    out[a_len:a_end] = (np.float32(80.0) + np.float32(7.0) * rng.standard_normal(a_end - a_len).astype(np.float32)).astype(np.float32)
    k = min(p_len, p_end - a_end)
    out[a_end: a_end + k] = base_row[a_len: a_len + k]
    out[a_end + k: p_end] = (np.float32(108.0) + np.float32(2.5) * rng.standard_normal(p_end - a_end - k).astype(np.float32)).astype(np.float32)
    out[p_end:] = base_row[a_len + p_len: a_len + p_len + m - p_end]
    return out


KINDS = ("ordinary", "long_polya", "seam1024", "seam2048", "late", "plateau", "holes", "shared", "mixed")
WINDOW = {"seam1024": 512}          # ADP_G2_WINDOW of the case; every other case: 1024
SEAM_OFFSETS = tuple(range(-10, 11))
PLATEAU_LEN = 400


def window_of(name):
    return WINDOW.get(name, 1024)


def _shaped(kind, r, rng, g, base):
    """read r of the pool reshaped for `kind` -> row"""
    from adapted_amd import synth

    a_len, p_len = synth.read_params(41, r)[:2]
    at = lambda k: g.off + k * g.ds   # noqa: E731  the sample at pooled index k
    if kind == "long_polya":          # the poly(A) ends behind the window's end 2048
        return _compose(rng, base[r], a_len, p_len, a_len, at(2300 + 7 * (r % 40)), g.m)
    if kind in ("seam1024", "seam2048"):
        return _compose(rng, base[r], a_len, p_len, a_len, at(int(kind[4:]) + SEAM_OFFSETS[r % len(SEAM_OFFSETS)]), g.m)
    if kind == "late":                # start + 1 + 1024 >= n: the whole trace inside a windowed call
        a_end = at(3200 + 3 * (r % 30))
        return _compose(rng, base[r], a_len, p_len, a_end, a_end + p_len, g.m)
    if kind == "mid":                 # an adapter that ends in tile 1: wend = 3072
        a_end = at(1100 + 5 * (r % 30))
        return _compose(rng, base[r], a_len, p_len, a_end, a_end + p_len, g.m)
    if kind == "plateau":             # saturated samples behind the adapter: equal pooled points, +inf gains side by side
        row = base[r].copy()
        b = g.off + -(-(a_len - g.off) // g.ds) * g.ds
        row[b: b + PLATEAU_LEN] = np.float32(400.0)
        return row
    return base[r].copy()


@functools.lru_cache(maxsize=None)
def ordinary_reads(oracle):
    """-> (the first N reads of the pool's first 96 that the restated rule decides inside the default window, how many of the 96 have
    a candidate, how many of those the rule leaves undecided)"""
    b = lc.make(GEOM, "pw_pool", [lc.geom_of(GEOM).L] * 96)
    ref = lc.reference(oracle, b)
    cand = [r for r, s in enumerate(ref) if s["cand"] >= 0]
    keep = [r for r in cand if decide(ref[r]["g2"], wend_of(ref[r]["cand"], 1024, ref[r]["n_valid"])) is not None]
    return tuple(keep[:N]), len(cand), len(cand) - len(keep)


@functools.lru_cache(maxsize=None)
def batch(name, oracle=None):
    g = lc.geom_of(GEOM)
    base = lc.pool(GEOM)
    rng = np.random.default_rng(1000 + KINDS.index(name))
    if name == "ordinary":
        reads = ordinary_reads(oracle)[0]
        return lc.make(GEOM, "pw_ordinary", [g.L] * len(reads), sig=base[list(reads)])
    sig = base[:N].copy()
    holes, plan, minibatch = (), [g.L] * N, None
    if name == "holes":               # NaN samples inside the window: a NaN pooled point, sanitised to 0 in the trace
        holes = tuple((r, g.off + (500 + 11 * r) * g.ds + 3, 4) for r in range(0, N, 3))
    elif name == "shared":            # per workgroup of four: an ordinary read, one without an adapter, and a dropped minibatch of two
        for r in range(N):
            if r % 4 == 1:
                sig[r, :] = np.float32(70.0 + 0.5 * r)
        plan, minibatch = [g.L, g.L, 0, 0] * (N // 4), 2
    elif name == "mixed":             # per workgroup of four: wend = 2048, 3072, n, and a read that the window does not settle
        for r in range(N):
            sig[r] = _shaped(("ordinary", "mid", "late", "long_polya")[r % 4], r, rng, g, base)
    else:
        for r in range(N):
            sig[r] = _shaped(name, r, rng, g, base)
    return lc.make(GEOM, "pw_" + name, plan, minibatch=minibatch, holes=holes, sig=sig)


def predict(ref, win):
    """per live read with a candidate: (wend, does the restated rule decide it inside the window); None elsewhere"""
    out = []
    for s in ref:
        if s is None or s["cand"] < 0 or s["n_valid"] < 3:
            out.append(None)
            continue
        we = wend_of(s["cand"], win, s["n_valid"])
        out.append((we, decide(s["g2"], we) is not None))
    return out
