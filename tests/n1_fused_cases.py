"""The single-pass N1 median / MAD (adapted_amd/csrc/n1_fused.h) restated in numpy, and the cases that drive each of its outcomes.
Shared by tests/test_n1_fused_cpu.py (no GPU) and tests/test_gpu_n1_fused.py.

The kernels guess two brackets from a sample of the minibatch (k_n1_hist / k_n1_pick<., N1_SAMPLE> / k_n1_fuse_setup), count and
copy in one pass over everything (k_n1_fused) and verify in a finish (k_n1_fused_finish) that either settles median and MAD
exactly or declines and leaves the minibatch to n1_select.h.  Three parts, as in the kernels:

  `brackets`      the sample's positions, both histogram levels and both modes of k_n1_fuse_setup: integer histograms and a few
                  float32 operations, reproduced bit for bit;
  `pass_counts`   what the pass counts and copies, given brackets and a heavy-key list, and whether a staging list overflows;
  `finish`        the caps, the rank tests, the zone of the MAD, the even count's lower value, the status.

`predict` chains them and names the outcome -- not_set_up, settled, decline_overflow (a cap, the staging lists or fewer than four
valid samples: one branch of the finish), decline_median, decline_mad -- with the increments of g_dbg[5, 6, 7, 17, 18, 19, 22, 23].
The choice of heavy keys (k_n1_heavy_scan / _pick: per-block hash tables that drop points when full) is NOT restated: `predict`
takes the key list and the band choice as inputs -- the device's own on the GPU, `standin_heavy` on the CPU.  numpy only."""
import numpy as np

F32 = np.float32
U32 = np.uint32

N1_BINS = 2048
N1_THREADS = 256
N1_WIN = 1 << 21
N1_CB_CAP = 1 << 22
N1_BRACKET_SIGMAS = 6.0
N1F_LDS_M = 768
N1F_LDS_B = 2304
N1F_MCAP = N1_CB_CAP // 4
N1F_BCAP = N1_CB_CAP - N1F_MCAP
N1H_MAX = 32
PDIV = 32
OUTCOMES = ("not_set_up", "settled", "decline_overflow", "decline_median", "decline_mad")
COUNTERS = (5, 6, 7, 17, 18, 19, 22, 23)
THRESH = 5.0  # RNA004's core.sig_norm_outlier_thresh (make_spc): enters lo / hi only


# ------------------------------------------------------------------------------------------- keys (common.h f2key / key2f)
def f2key(x):
    u = np.asarray(x, dtype=F32).view(U32)
    return u ^ (((u >> U32(31)) * U32(0xFFFFFFFF)) | U32(0x80000000))


def key2f(k):
    k = np.asarray(k, dtype=U32)
    u = np.where(k & U32(0x80000000), k & U32(0x7FFFFFFF), ~k).astype(U32)
    return u.view(F32)


def _k2f(k):
    return key2f(np.array([k & 0xFFFFFFFF], dtype=U32))[0]


def _f2k(x):
    return int(f2key(np.array([x], dtype=F32))[0])


# --------------------------------------------------------------------------------------------------- (a) sample and brackets
def geometry(T, minibatch):
    """launch_n1's sample: col_div pieces of Tp samples per read, one in every Rg samples, or every row_step-th read whole"""
    col_div = 1
    if T >= 8192:
        col_div = min(64, max(2, T // (PDIV * 96)))
    row_step = 1 if col_div > 1 else max(1, minibatch // 32)
    s0 = 8 if (col_div > 1 and minibatch >= 64) else 1  # ADP_N1_S0: the first level reads an eighth of the sampled rows
    Rg = ((T // col_div) & ~3) if col_div > 1 else 0
    Tp = ((T // (col_div * PDIV)) & ~3) if col_div > 1 else T
    return dict(col_div=col_div, row_step=row_step, s0=s0, Rg=Rg, Tp=Tp)


def row_ends(lens, T, tails):
    """Te per read: the whole window, or the read's own end under ADP_TAILS_NAN"""
    lens = np.asarray(lens, dtype=np.int64)
    return np.clip(lens, 0, T) if tails else np.full(lens.size, T, dtype=np.int64)


def sample_mask(rows, T, minibatch, Te, level, vec):
    """bool [rows, T]: the positions k_n1_hist reads at `level` (0: the window, 1: the bracket) of a minibatch of `rows` reads"""
    g = geometry(T, minibatch)
    step = g["row_step"] * (g["s0"] if level == 0 else 1)
    mask = np.zeros((rows, T), dtype=bool)
    for rr in range(0, rows, step):
        te = int(Te[rr])
        if g["col_div"] > 1:
            rot = (rr // step) % PDIV
            for pc in range(g["col_div"]):
                a = pc * g["Rg"] + rot * g["Tp"]
                pos = np.arange(a, a + g["Tp"])
                # (vector path: a float4 is read whole when its first sample lies in front of the end)
                keep = ((pos & ~3) < te) if vec else (pos < te)
                mask[rr, pos[keep]] = True
        else:
            mask[rr, :te] = True
    return mask


def _find(hist, k):
    """n1_find: (bin holding rank k or -1, samples before it, total)"""
    cum = np.cumsum(hist.astype(np.int64))
    tot = int(cum[-1])
    if k >= tot:
        return -1, 0, tot
    b = int(np.searchsorted(cum, k, side="right"))
    return b, int(cum[b] - hist[b]), tot


def _clamp_window(c):
    lo = c - (N1_WIN >> 1) if c > (N1_WIN >> 1) else 0
    lo &= ~1023
    if lo > 0xFFFFFFFF - N1_WIN:
        lo = (0xFFFFFFFF - N1_WIN) & ~1023
    return lo


def sample_bracket(v0, v1):
    """both levels of a statistic's sample: v0 / v1 the float32 values of level 0 / 1 (NaN dropped here) -> (cklo, ckw)"""
    k0 = f2key(v0[v0 == v0])
    hist = np.bincount((k0 >> U32(21)).astype(np.int64), minlength=N1_BINS)
    k = int(hist.sum()) // 2
    b, before, _ = _find(hist, k)
    c = 0
    if b >= 0:
        cnt = int(hist[b])
        frac = float(k - before) / float(cnt) if cnt else 0.5
        c = (b << 21) + int(frac * 2097152.0)
    kbase = _clamp_window(c)
    k1 = f2key(v1[v1 == v1]).astype(np.int64)
    Ms = k1.size
    d = (k1 - kbase) & 0xFFFFFFFF
    inwin = d < N1_WIN
    c_below = int((k1 < kbase).sum())
    hist = np.bincount((d[inwin] >> 10), minlength=N1_BINS)
    k = Ms // 2
    miss = k < c_below
    krel = 0 if miss else k - c_below
    b, before, tot = _find(hist, krel)
    if b < 0:
        miss = True
    D = int(N1_BRACKET_SIGMAS * np.sqrt(float(Ms))) + 16
    D = min(D, (N1_CB_CAP // 4) * 7 // 10 // 64)
    cut = miss or krel < D or krel + D >= tot
    rlo = krel - D if krel > D else 0
    rhi = krel + D
    if tot and rhi > tot - 1:
        rhi = tot - 1
    blo = _find(hist, rlo)[0]
    bhi = _find(hist, rhi)[0]
    if tot and not cut and blo >= 0 and bhi >= blo:
        return (kbase + (blo << 10)) & 0xFFFFFFFF, ((bhi + 1 - blo) << 10) & 0xFFFFFFFF
    return 0, 0


def zero_brackets():
    z = F32(0.0)
    return dict(med_s=z, A0=z, A1=z, D0=z, D1=z, eps=z, ok=0, wide_ok=0, D0w=z, D1w=z)


def setup_median(cklo, ckw):
    """k_n1_fuse_setup, mode 0"""
    f = zero_brackets()
    if ckw and ((cklo + ckw) & 0xFFFFFFFF) > cklo:
        a_lo, a_hi, ms = _k2f(cklo), _k2f(cklo + ckw), _k2f(cklo + (ckw >> 1))
        with np.errstate(all="ignore"):
            f["med_s"], f["A0"], f["A1"] = ms, F32(a_lo - ms), F32(a_hi - ms)
            f["eps"] = F32(np.fmax(-f["A0"], f["A1"]))
        f["ok"] = int(f["A0"] <= 0 and f["A1"] > 0 and f["eps"] < np.inf)
    return f


def setup_mad(f, cklo, ckw):
    """k_n1_fuse_setup, mode 1 (in place)"""
    if not f["ok"]:
        return f
    if ckw and ((cklo + ckw) & 0xFFFFFFFF) > cklo:
        d_lo, d_hi = _k2f(cklo), _k2f(cklo + ckw)
        with np.errstate(all="ignore"):
            tail = F32(F32(1e-6) * np.abs(f["med_s"]))
            e = F32(F32(F32(f["eps"] * F32(1.01)) + tail) + F32(1e-30))
            f["D0"], f["D1"] = F32(d_lo - e), F32(d_hi + e)
            f["ok"] = int(f["D0"] > f["eps"] and f["D1"] > f["D0"] and f["D1"] < np.inf)
            e2 = F32(F32(F32(f["eps"] * F32(2.02)) + tail) + F32(1e-30))
            f["D0w"], f["D1w"] = F32(d_lo - e2), F32(d_hi + e2)
            f["wide_ok"] = int(bool(f["ok"]) and f["D0w"] > f["eps"] and f["D1w"] > f["D0w"] and f["D1w"] < np.inf)
    else:
        f["ok"] = 0
    return f


def brackets(x, Te, T, minibatch, vec=True):
    """x: the minibatch's rows [rows, >= T] float32 -> the N1Fused struct as k_n1_fuse_setup leaves it (narrow band in D0 / D1)"""
    rows = x.shape[0]
    xs = x[:, :T]
    m0 = sample_mask(rows, T, minibatch, Te, 0, vec)
    m1 = sample_mask(rows, T, minibatch, Te, 1, vec)
    v0, v1 = xs[m0], xs[m1]
    f = setup_median(*sample_bracket(v0, v1))
    with np.errstate(invalid="ignore"):
        ms = f["med_s"]  # (mode 0 leaves med_s in MbState.med: the MAD's sample measures |x - med_s|)
        t0, t1 = np.abs(v0 - ms, dtype=F32), np.abs(v1 - ms, dtype=F32)
    return setup_mad(f, *sample_bracket(t0, t1))


def use_band(f, wide):
    """the struct as k_n1_heavy_pick leaves it: the wide band moved into D0 / D1 when it chose it"""
    g = dict(f)
    if wide:
        g["D0"], g["D1"] = f["D0w"], f["D1w"]
    return g


# -------------------------------------------------------------------------------------------------------------- (b) the pass
def _segments_overflow(take_m, take_b, Te, vec):
    """does any (row, segment) put more than N1F_LDS_M / N1F_LDS_B copied samples into a staging list?"""
    cm, cb = take_m.sum(axis=1), take_b.sum(axis=1)
    for r in np.nonzero((cm > N1F_LDS_M) | (cb > N1F_LDS_B))[0]:
        te = int(Te[r])
        pos = np.arange(te)
        if vec:
            T4 = te >> 2
            if T4 == 0:
                seg = np.zeros(te, dtype=np.int64)
            else:
                q4 = ((T4 + 7) // 8 + 2 * N1_THREADS - 1) // (2 * N1_THREADS) * (2 * N1_THREADS)
                seg = np.minimum(pos >> 2, T4 - 1) // q4  # (the samples behind the last float4 go with the last segment)
        else:
            seg = np.zeros(te, dtype=np.int64)
        if (np.bincount(seg, weights=take_m[r, :te]).max(initial=0) > N1F_LDS_M
                or np.bincount(seg, weights=take_b[r, :te]).max(initial=0) > N1F_LDS_B):
            return True
    return False


def pass_counts(x, Te, T, f, hkeys=(), vec=True):
    """k_n1_fused over one minibatch: counts, the two lists (copied values) and the heavy keys' counts"""
    xs = np.array(x[:, :T], dtype=F32)
    xs[np.arange(T)[None, :] >= np.asarray(Te)[:, None]] = np.nan
    hkeys = np.asarray(hkeys, dtype=U32)
    with np.errstate(invalid="ignore"):
        u = xs - f["med_s"]
        t = np.abs(u)
        valid = t == t
        ge0, lt1, ged, led = u >= f["A0"], u < f["A1"], t >= f["D0"], t <= f["D1"]
    take = (ge0 & lt1) | (ged & led)
    out = dict(valid=int(valid.sum()), below=int((valid & ~ge0).sum()), inner=int((valid & ~ged).sum()))
    inner = take & ~ged  # n1f_copy: fabsf(x - med_s) < D0
    heavy = np.zeros_like(take)
    hcnt = np.zeros(hkeys.size, dtype=np.int64)
    if hkeys.size:
        kt = f2key(xs[take])
        idx = np.searchsorted(hkeys, kt)
        hit = (idx < hkeys.size) & (hkeys[np.minimum(idx, hkeys.size - 1)] == kt)
        heavy[take] = hit
        hcnt = np.bincount(idx[hit], minlength=hkeys.size)
    cm, cb = take & inner & ~heavy, take & ~inner & ~heavy
    out.update(list_m=xs[cm], list_b=xs[cb], hcnt=hcnt, heavy_m=int((heavy & inner).sum()), heavy_b=int((heavy & ~inner).sum()),
               overflow=_segments_overflow(cm, cb, Te, vec))
    return out


# ------------------------------------------------------------------------------------------------------------ (c) the finish
def _select(vals, wts, keys, klo, khi, rank_in_zone, need_prev):
    """n1f_select: -> (ok, key of the rank, key of the rank before it, c_lo, c_hi)"""
    keys = keys.astype(np.int64)
    c_lo, c_hi = int(wts[keys < klo].sum()), int(wts[keys > khi].sum())
    kz = rank_in_zone(c_lo)
    if kz < (1 if need_prev else 0):
        return False, 0, 0, c_lo, c_hi
    z = (keys >= klo) & (keys <= khi)
    zk, zw = keys[z], wts[z]
    o = np.argsort(zk, kind="stable")
    zk, cum = zk[o], np.cumsum(zw[o])
    if zk.size == 0 or kz >= cum[-1]:
        return False, 0, 0, c_lo, c_hi
    i = int(np.searchsorted(cum, kz, side="right"))
    k1 = int(zk[i])
    first = int(np.searchsorted(zk, k1, side="left"))  # items with a smaller key: cum[first - 1]
    before = int(cum[first - 1]) if first else 0
    k0 = k1
    if kz == before:
        if first == 0:
            return (not need_prev), k1, k1, c_lo, c_hi
        k0 = int(zk[first - 1])
    return True, k1, k0, c_lo, c_hi


def finish(f, p, hkeys=(), thresh=THRESH):
    """k_n1_fused_finish on the pass's result p -> dict(outcome, counters, why[, med, mad, lo, hi, mad_zero])"""
    cnt = {c: 0 for c in COUNTERS}
    if not f["ok"]:
        return dict(outcome="not_set_up", counters=cnt, why="no brackets")
    hkeys = np.asarray(hkeys, dtype=U32)
    nh = hkeys.size
    hval = key2f(hkeys) if nh else np.zeros(0, dtype=F32)
    hc = np.asarray(p["hcnt"], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        h_inner = np.abs(hval - f["med_s"], dtype=F32) < f["D0"] if nh else np.zeros(0, dtype=bool)
    hwm, hwb = np.where(h_inner, hc, 0), np.where(h_inner, 0, hc)
    cnt[5], cnt[22], cnt[23] = 1, nh, int(hc.sum())
    l_cm, l_cb = p["list_m"].size, p["list_b"].size
    n_valid, n_below, n_inner = p["valid"], p["below"], p["inner"]
    why = []
    if p["overflow"]:
        # (a flush that overflows adds nothing to the lists, so the caps see what is left: not restated, not asserted)
        cnt[19], cnt[18], cnt[17] = 1, None, None
        why.append("staging")
    else:
        if l_cm > N1F_MCAP:
            cnt[18] = 1
            why.append("median list cap")
        if l_cb > N1F_BCAP:
            cnt[17] = 1
            why.append("band cap")
    if n_valid < 4:
        why.append("n_valid < 4")
    if why:
        cnt[6] = 1
        return dict(outcome="decline_overflow", counters=cnt, why=", ".join(why))
    n_cm = l_cm + int(hwm.sum())
    even = n_valid % 2 == 0
    k = n_valid // 2
    one = np.ones(l_cm, dtype=np.int64)
    with np.errstate(all="ignore"):
        ka, kb = _f2k(F32(f["med_s"] + f["A0"])), _f2k(F32(f["med_s"] + f["A1"]))
    klo = ka - 64 if ka > 64 else 0
    khi = kb + 64 if kb < 0xFFFFFFFF - 64 else 0xFFFFFFFF
    hm = hwm > 0
    ok, kk, km1, c_lo, c_hi = _select(np.concatenate([p["list_m"], hval[hm]]), np.concatenate([one, hwm[hm]]),
                                      f2key(np.concatenate([p["list_m"], hval[hm]])), klo, khi,
                                      lambda _c: (k - n_below) if (k >= n_below and k - n_below < n_cm) else -1, even)
    if not ok or c_lo or c_hi:
        cnt[6] = 1
        return dict(outcome="decline_median", counters=cnt, why="rank outside the median bracket")
    med, med_key, med_lower_key = _k2f(kk), kk, km1
    if even:
        med = F32(F32(_k2f(km1) + med) / F32(2.0))
    delta = abs(float(med) - float(f["med_s"]))
    tlo, thi = (float(f["D0"]) + delta) * (1.0 + 1e-12), (float(f["D1"]) - delta) * (1.0 - 1e-12)
    vlo = F32(tlo)
    if float(vlo) < tlo:
        vlo = (np.array([vlo]).view(U32) + U32(1)).view(F32)[0]
    vhi = F32(thi)
    if float(vhi) > thi:
        vhi = (np.array([vhi]).view(U32) - U32(1)).view(F32)[0]
    if not (thi > 0.0) or not (vhi > vlo) or ((_f2k(vhi) - _f2k(vlo)) & 0xFFFFFFFF) < 2:
        cnt[7] = 1
        return dict(outcome="decline_mad", counters=cnt, why="no zone left", med=med)
    hb = hwb > 0
    xb = np.concatenate([p["list_b"], hval[hb]])
    with np.errstate(invalid="ignore"):
        kb_ = f2key(np.abs(xb - med, dtype=F32))
    ok, kk, km1, _, _ = _select(xb, np.concatenate([np.ones(l_cb, dtype=np.int64), hwb[hb]]), kb_, _f2k(vlo) + 1, _f2k(vhi) - 1,
                                lambda c: (k - (n_inner + c)) if k >= n_inner + c else -1, even)
    if not ok:
        cnt[7] = 1
        return dict(outcome="decline_mad", counters=cnt, why="rank outside the zone", med=med)
    mad = _k2f(kk)
    if even:
        mad = F32(F32(_k2f(km1) + mad) / F32(2.0))
    lo, hi = F32(float(med) - float(mad) * thresh), F32(float(med) + float(mad) * thresh)
    med_heavy = bool(nh and (hkeys[hm].astype(np.int64) == med_key).any())  # the upper middle value is a counted one
    return dict(outcome="settled", counters=cnt, why="", med=med, mad=mad, lo=lo, hi=hi, mad_zero=bool(mad == 0), n_valid=n_valid,
                med_heavy=med_heavy, med_key=med_key, med_lower_key=med_lower_key)


def predict(x, Te, T, minibatch, hkeys=(), wide=False, f=None, vec=True, thresh=THRESH):
    """one minibatch (x: its rows) -> finish()'s dict plus `brackets` (as the sample gives them) and `pass` (the counts)"""
    fs = brackets(x, Te, T, minibatch, vec) if f is None else f
    fu = use_band(fs, wide)
    if not fu["ok"]:
        r = finish(fu, None)
        r.update(brackets=fs)
        return r
    p = pass_counts(x, Te, T, fu, hkeys, vec)
    r = finish(fu, p, hkeys, thresh)
    r.update(brackets=fs, used=fu, **{"pass": p})
    return r


def zone_counts(x, Te, T, f):
    """numpy's count of every distinct value among the samples the pass takes (median bracket or band): key -> count"""
    p = pass_counts(x, Te, T, f)
    k, c = np.unique(f2key(np.concatenate([p["list_m"], p["list_b"]])), return_counts=True)
    return dict(zip(k.tolist(), c.tolist()))


def standin_heavy(x, Te, T, fs):
    """A stand-in for k_n1_heavy_scan / _pick where no device is at hand -- NOT a restatement (the device's tables drop points):
    the up to 32 most frequent taken values when they carry at least half of the taken samples, and the wide band when they
    carry nine tenths (the rules of k_n1_heavy_pick applied to all samples instead of the sample's)."""
    if not fs["ok"]:
        return np.zeros(0, dtype=U32), False
    zc = zone_counts(x, Te, T, use_band(fs, bool(fs["wide_ok"])))
    tot = sum(zc.values())
    top = sorted(zc.items(), key=lambda kv: -kv[1])[:N1H_MAX]
    top = [(k, c) for k, c in top if c >= max(16, tot // 128)]
    hs = sum(c for _, c in top)
    if not top or hs * 2 < tot:
        return np.zeros(0, dtype=U32), False
    return np.array(sorted(k for k, _ in top), dtype=U32), bool(fs["wide_ok"] and hs * 10 >= tot * 9)


def oracle_params(oracle_mod, x, T, thresh=THRESH):
    """(med, mad, lo, hi) float64 of the oracle (np.nanmedian and the float32 MAD)"""
    rc, want = oracle_mod.norm_params(np.ascontiguousarray(x), T, thresh)
    return want


# ------------------------------------------------------------------------------------------------------------------ the cases
# geometries: T (core.max_obs_trace), m (samples per row), reads, minibatch -- all a few MB of float32
GEOM = {
    "g4000": dict(T=4000, m=4000, n=128, mb=128),      # col_div 1: every (n / 32)-th read whole
    "g8192": dict(T=8192, m=8192, n=96, mb=96),        # col_div 2
    "g16000": dict(T=16000, m=16000, n=64, mb=64),     # col_div 5, Tp 100, Rg 3200
    "scalar": dict(T=8192, m=8194, n=96, mb=96),       # m & 3 != 0: every kernel's scalar path
    "two_mb": dict(T=8192, m=8192, n=136, mb=96),      # two minibatches, the last one short (40 reads)
    # The median list's cap (2^20 copied samples) cannot be met at 8192 x 160: a staging list takes 768 samples per flush and a
    # row of 8192 has four flushes, 160 x 4 x 768 < 2^20 -- the staging overflow always comes first.  Rows of 1024 samples (one
    # flush each) with 768 values inside the bracket reach it at 1440 reads, 5.9 MB.
    "cap": dict(T=1024, m=1024, n=1440, mb=1440),
}
# band_cap is left out: the band list holds 3 * 2^20 samples, so more than 3.1 M samples (12.6 MB of float32) have to lie inside
# the band alone -- beyond the 8 MB a case may take.


def make_spc(T):
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.core.max_obs_trace = T
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


def sampled_positions(g, tails_Te=None):
    """bool [mb rows, T]: every position any sampling kernel of the first minibatch reads (both levels of k_n1_hist and
    k_n1_heavy_scan, which takes every fourth sampled row and rotates by its own row count)"""
    T, rows = g["T"], min(g["n"], g["mb"])
    Te = np.full(rows, T) if tails_Te is None else tails_Te
    vec = g["m"] % 4 == 0
    mask = sample_mask(rows, T, g["mb"], Te, 0, vec) | sample_mask(rows, T, g["mb"], Te, 1, vec)
    gg = geometry(T, g["mb"])
    step = gg["row_step"] * 4
    for rr in range(0, rows, step):
        if gg["col_div"] > 1:
            rot = (rr // step) % PDIV
            for pc in range(gg["col_div"]):
                a = pc * gg["Rg"] + rot * gg["Tp"]
                mask[rr, a:a + gg["Tp"]] = True
        else:
            mask[rr, :] = True
    return mask


def _base(rng, shape, g, centre=100.0, scale=1.0):
    """The signal of a case.  A bracket only exists where k_n1_pick's 2^21-key window holds the sample ranks +-D: for the
    MAD of N(100, 8) that takes a sample of about 10^5 points (window +-0.5 round 5.4, ranks +-D within +-0.2), which only the
    4000-sample geometry's whole-row sample has.  The others get a density that is high at both statistics: a narrow centre
    (40 % N(c, 1)) between two shoulders (60 % c +- N(6, 0.5))."""
    if g["T"] == 4000:
        return (centre + scale * rng.normal(0.0, 8.0, shape)).astype(F32)
    core = rng.random(shape) < 0.4
    x = np.where(core, rng.normal(0.0, 1.0, shape), rng.choice([-1.0, 1.0], shape) * rng.normal(6.0, 0.5, shape))
    return (centre + scale * x).astype(F32)


def _grid(x, step):
    return (np.round(x / F32(step)) * F32(step)).astype(F32)


def _middle_two(sig, T):
    """flat indices (into sig[:, :T]) of the lower and the upper middle sample of an even count without NaN"""
    flat = sig[:, :T].ravel()
    k = flat.size // 2
    part = np.argpartition(flat, [k - 1, k])
    return part[k - 1], part[k]


CASE_GEOM = {
    "plain": "g8192", "odd_count": "g4000", "nan_rows": "g16000", "negatives": "g8192", "centred_zero": "g8192",
    "adc_grid": "g8192", "adc_grid_odd": "g16000", "coarse_grid": "g4000", "half_grid": "g8192",
    "even_lower_copied": "g4000", "even_lower_heavy": "g8192", "even_lower_one_key": "g16000",
    "constant": "g8192", "two_values": "g4000", "median_outside": "g8192", "mad_outside": "g16000",
    "median_list_cap": "cap", "staging_overflow": "g8192", "fewer_than_four": "g4000", "tails": "g8192",
    "scalar_path": "scalar", "two_minibatches": "two_mb",
}
# what each case was built for, per minibatch (None: whatever the device chose -- exactness only)
EXPECT = {
    "plain": ["settled"], "odd_count": ["settled"], "nan_rows": ["settled"], "negatives": ["settled"],
    # N(0, 10): the issue hoped for a bracket whose keys span the sign.  The sample's second level works inside a window of
    # 2^21 keys, and round zero that window is 3e-39 wide: no sample of such data ever gets a bracket (k_n1_pick's `cut`), and
    # data that fit the window (denormals) fail k_n1_fuse_setup's D0 > eps through its 1e-30 term.  A bracket that spans zero
    # therefore exists only as a hand-made one: tests/test_n1_fused_cpu.py settles those; the device case is not_set_up.
    "centred_zero": ["not_set_up"],
    "adc_grid": ["settled"], "adc_grid_odd": ["settled"], "coarse_grid": ["settled"], "half_grid": [None],
    "even_lower_copied": ["settled"], "even_lower_heavy": ["settled"], "even_lower_one_key": ["settled"],
    # one value (and one outlier) / two values 40 apart: the MAD's sample bracket lies inside eps, the two values do not fit one
    # window -- no brackets.  (mad == 0 cannot come out of the finish at all: its zone starts above vlo > 0.)
    "constant": ["not_set_up"], "two_values": ["not_set_up"],
    "median_outside": ["decline_median"], "mad_outside": ["decline_mad"], "median_list_cap": ["decline_overflow"],
    "staging_overflow": ["decline_overflow"], "fewer_than_four": ["not_set_up"], "tails": ["settled"],
    "scalar_path": ["settled"], "two_minibatches": ["settled", "settled"],
}
CONTROLS = ["plain", "odd_count", "nan_rows", "negatives", "adc_grid", "adc_grid_odd", "coarse_grid", "even_lower_copied",
            "even_lower_heavy", "even_lower_one_key", "tails", "scalar_path", "two_minibatches"]
HEAVY = ["adc_grid", "adc_grid_odd", "coarse_grid", "even_lower_heavy"]  # nh > 0, the wide band, a counted median
NAMES = list(CASE_GEOM)
_cache = {}


def case(name):
    """-> dict(name, geom, sig float32 [n, m], lens int32 [n], T, m, n, mb, tails, expect, ...)"""
    if name in _cache:
        return _cache[name]
    g = dict(GEOM[CASE_GEOM[name]])
    T, m, n = g["T"], g["m"], g["n"]
    rng = np.random.default_rng(1000 + NAMES.index(name))
    sig = _base(rng, (n, m), g)
    lens = np.full(n, m, dtype=np.int32)
    tails = False
    extra = {}
    if name == "odd_count":
        sig[3, 17] = np.nan
    elif name == "nan_rows":
        sig[0::3] = np.nan
        lens[0::3] = 0
    elif name == "negatives":
        sig *= F32(-1.0)
    elif name == "centred_zero":
        sig = _base(rng, (n, m), g, centre=0.0)
    elif name in ("adc_grid", "adc_grid_odd"):
        sig = _grid(sig, 0.18)
        if name == "adc_grid_odd":
            sig[3, 17] = np.nan
    elif name == "coarse_grid":
        sig = _grid(sig, 3.0)
    elif name == "half_grid":
        sig[0::2] = _grid(sig[0::2], 0.18)
    elif name == "even_lower_copied":  # (i) the value under the upper middle one is another copied sample
        lo, hi = _middle_two(sig, T)
        extra["middle"] = (float(sig[:, :T].flat[lo]), float(sig[:, :T].flat[hi]))
        assert extra["middle"][0] < extra["middle"][1]
    elif name == "even_lower_one_key":  # (iii) ... lies one key under it
        lo, hi = _middle_two(sig, T)
        up = sig[:, :T].flat[hi]
        sig[:, :T].flat[lo] = np.nextafter(up, F32(-np.inf))
        extra["middle"] = (float(sig[:, :T].flat[lo]), float(up))
    elif name == "even_lower_heavy":  # (ii) ... is a counted (heavy) value: grid data, ONE sample off the grid as the upper middle
        sig = _grid(sig, 0.18)
        flat = sig.ravel()  # (m == T)
        vals = np.unique(flat)
        g1 = vals[np.searchsorted(vals, F32(100.0))]
        u = F32(g1 + F32(0.07))
        free = np.nonzero(~sampled_positions(g).ravel())[0]  # touch no position a sampling kernel reads
        flat[free[0]] = u
        k = flat.size // 2
        diff = int((flat < u).sum()) - k  # > 0: that many samples have to move from below to above
        pool = free[1:]  # mirror that many samples at g1: from (g1 - 4, g1 - 1.5) to the other side, or back
        d = flat[pool] - g1
        src = pool[(d < -1.5) & (d > -4.0)] if diff > 0 else pool[(d > 1.5) & (d < 4.0)]
        src = src[:abs(diff)]
        assert src.size == abs(diff)
        mirrored = (g1 - (flat[src] - g1)).astype(F32)
        flat[src] = vals[np.clip(np.searchsorted(vals, mirrored - F32(0.09)), 0, vals.size - 1)]
        assert int((flat < u).sum()) == k and flat[flat < u].max() == g1
        extra["middle"] = (float(g1), float(u))
    elif name == "constant":
        sig[:, :] = F32(77.25)
        sig[1, 5] = F32(80.0)
    elif name == "two_values":
        sig[:, :] = F32(50.0)
        sig[:, 1::2] = F32(90.0)
    elif name == "median_outside":  # the sample sees the signal round 100, everything else lies round 120
        s = sampled_positions(g)
        sig[:, :T][~s] = _base(rng, int((~s).sum()), g, centre=120.0)
    elif name == "mad_outside":  # the median agrees, the spread of what the sample does not see is three times wider
        s = sampled_positions(g)
        sig[:, :T][~s] = _base(rng, int((~s).sum()), g, scale=3.0)
    elif name == "median_list_cap":  # every unsampled read: 768 distinct values inside the median bracket, 256 far outside the band
        s = sampled_positions(g)
        for r in np.nonzero(~s.any(axis=1))[0]:
            row = np.concatenate([rng.uniform(99.8, 100.2, 768), rng.normal(40.0, 2.0, 128), rng.normal(160.0, 2.0, 128)])
            sig[r] = rng.permutation(row).astype(F32)
    elif name == "staging_overflow":  # read 5, second quarter: what the sample does not see lies inside the median bracket
        s = sampled_positions(g)[5, 2048:4096]
        seg = sig[5, 2048:4096]
        seg[~s] = rng.uniform(99.9, 100.1, int((~s).sum())).astype(F32)
        assert (~s).sum() > N1F_LDS_M
    elif name == "fewer_than_four":
        keep = [(0, 0), (64, 1999), (127, 3999)]
        v = [sig[r, c] for r, c in keep]
        sig[:, :] = np.nan
        for (r, c), x in zip(keep, v):
            sig[r, c] = x
    elif name == "tails":  # Pareto lengths, NaN behind every read's end
        tails = True
        ln = np.minimum(3 * T, (1500 * (1.0 + rng.pareto(1.2, n))).astype(np.int64))
        ln[:8] = [0, 1, 3, 4 * 500 + 1, T, T - 1, 2, 3 * T]
        lens = ln.astype(np.int32)
        sig[np.arange(m)[None, :] >= lens[:, None]] = np.nan
    elif name == "scalar_path":
        sig[:, T:] = F32(1e6)  # behind the window: never read by N1
    elif name == "two_minibatches":
        sig[g["mb"]:] = _base(rng, (n - g["mb"], m), g, centre=80.0, scale=0.7)
        sig[g["mb"] + 7, 33] = np.nan
    c = dict(name=name, sig=np.ascontiguousarray(sig), lens=lens, tails=tails, expect=EXPECT[name], vec=(m % 4 == 0), **g)
    c.update(extra)
    assert c["sig"].nbytes <= 8 << 20
    _cache[name] = c
    return c


def minibatches(c):
    """[(rows of the minibatch, Te per row)]"""
    Te = row_ends(c["lens"], c["T"], c["tails"])
    return [(c["sig"][r0:r0 + c["mb"]], Te[r0:r0 + c["mb"]]) for r0 in range(0, c["n"], c["mb"])]


def predict_case(c, heavy=None):
    """the predictions per minibatch; heavy: [(keys, wide)] per minibatch (the device's), default the CPU stand-in"""
    out = []
    for i, (x, Te) in enumerate(minibatches(c)):
        fs = brackets(x, Te, c["T"], c["mb"], c["vec"])
        keys, wide = heavy[i] if heavy is not None else standin_heavy(x, Te, c["T"], fs)
        out.append(predict(x, Te, c["T"], c["mb"], keys, wide, f=fs, vec=c["vec"]))
    return out
