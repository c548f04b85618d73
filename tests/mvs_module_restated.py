"""A CPU restatement of the reference's MVS poly(A) module (adapted/detect/mvs.py) with numpy only, under numpy 1.x's rules
whatever numpy runs it: the array range checks compare float32 series against float32 bounds (value-based casting), the
scalar ones in float64; np.median / np.percentile propagate NaN, np.nanmedian skips it.  bottleneck's move_mean / move_var are
restated here as bottleneck/src/move_template.c runs them, NaN-aware, in the input dtype (np.float32 scalars, or Python floats
for float64); tests/test_mvs_module_cpu.py pins the float32 form to oracle/bn_shim.py and the whole module to the fixture the
real reference wrote (tests/golden/mvs_module.npz).  Integer input is widened to float64.  TEST INFRASTRUCTURE."""
import math

import numpy as np

PCTLS = (85, 15)
NAN = float("nan")


class RefIndexError(IndexError):
    pass


def work(x):
    x = np.asarray(x)
    if x.dtype == np.float32 or x.dtype == np.float64:
        return x
    if np.issubdtype(x.dtype, np.integer):
        return x.astype(np.float64)
    raise TypeError(x.dtype)


def _scal(x):
    """the samples as scalars of the arithmetic: np.float32 for float32, Python float (IEEE double) for float64"""
    return list(x) if x.dtype == np.float32 else x.tolist()


def _bn_check(n, w):
    if w < 1 or w > n:
        raise ValueError("Moving window (=%d) must between 1 and %d, inclusive" % (w, n))


def move_mean(x, w):
    x = work(x)
    _bn_check(x.size, w)
    F = np.float32 if x.dtype == np.float32 else float
    a = _scal(x)
    out = [NAN] * len(a)
    asum, count = F(0), 0
    inv = F(0)
    for i in range(w):
        ai = a[i]
        if ai == ai:
            asum = asum + ai
            count += 1
    if count >= w:
        out[w - 1] = asum / F(count)
    inv = F(1.0 / count) if count else F(math.inf)
    for i in range(w, len(a)):
        ai, aold = a[i], a[i - w]
        if ai == ai:
            if aold == aold:
                asum = asum + (ai - aold)
            else:
                asum = asum + ai
                count += 1
                inv = F(1.0 / count)
        elif aold == aold:
            asum = asum - aold
            count -= 1
            inv = F(1.0 / count) if count else F(math.inf)
        if count >= w:
            out[i] = asum * inv
    return np.array(out, dtype=x.dtype)


def move_var(x, w):
    x = work(x)
    _bn_check(x.size, w)
    F = np.float32 if x.dtype == np.float32 else float
    a = _scal(x)
    out = [NAN] * len(a)
    amean, assqdm, count = F(0), F(0), 0
    for i in range(w):
        ai = a[i]
        if ai == ai:
            count += 1
            delta = ai - amean
            amean = amean + delta / F(count)
            assqdm = assqdm + delta * (ai - amean)
    if count >= w:
        if assqdm < 0:
            assqdm = F(0)
        out[w - 1] = assqdm / F(count)
    inv = F(1.0 / count) if count else F(math.inf)
    for i in range(w, len(a)):
        ai, aold = a[i], a[i - w]
        if ai == ai:
            if aold == aold:
                delta = ai - aold
                aold = aold - amean
                amean = amean + delta * inv
                ai = ai - amean
                assqdm = assqdm + (ai + aold) * delta
            else:
                count += 1
                inv = F(1.0 / count)
                delta = ai - amean
                amean = amean + delta * inv
                assqdm = assqdm + delta * (ai - amean)
        elif aold == aold:
            count -= 1
            inv = F(1.0 / count) if count else F(math.inf)
            if count > 0:
                delta = aold - amean
                amean = amean - delta * inv
                assqdm = assqdm - delta * (aold - amean)
            else:
                amean, assqdm = F(0), F(0)
        if count >= w:
            if assqdm < 0:
                assqdm = F(0)
            out[i] = assqdm * inv
    return np.array(out, dtype=x.dtype)


def median(x):
    """np.median: NaN for an empty slice or one with a NaN; an even count averages in the dtype"""
    if x.size == 0 or np.isnan(x).any():
        return x.dtype.type(NAN)
    s = np.sort(x)
    n = s.size
    if n & 1:
        return s[n // 2]
    return (s[n // 2 - 1] + s[n // 2]) / x.dtype.type(2)


def nanmedian(x):
    return median(x[~np.isnan(x)])


def percentile_pair(x, integer=False):
    """np.percentile(x, (85, 15)) (linear): the rank arithmetic in float64, the difference of the neighbours in the dtype,
    the interpolation in float64; NaN anywhere: NaN; an empty slice: numpy's IndexError (its index reads 0 for integer input)"""
    n = x.size
    if n == 0:
        raise RefIndexError("index %d is out of bounds for axis 0 with size 0" % (0 if integer else -1))
    if np.isnan(x).any():
        return NAN, NAN
    s = np.sort(x)
    res = []
    for q in PCTLS:
        vi = float(n - 1) * (q / 100.0)
        lo = min(max(int(math.floor(vi)), 0), n - 1)
        hi = min(lo + 1, n - 1)
        g = vi - lo
        a, b = s[lo], s[hi]
        diff = float(b - a)
        r = float(a) + diff * g
        if g >= 0.5:
            r = float(b) - diff * (1.0 - g)
        res.append(r)
    return res[0], res[1]


def rng(r):
    lo, hi = (None, None) if r is None else r
    return (-math.inf if lo is None else float(lo), math.inf if hi is None else float(hi))


def in_range_scalar(v, r):
    lo, hi = rng(r)
    return bool(lo <= float(v) <= hi)


def in_range_arr(v, r):
    lo, hi = rng(r)
    if v.dtype == np.float32:
        with np.errstate(over="ignore"):
            lo, hi = np.float32(lo), np.float32(hi)
    return (lo <= v) & (v <= hi)


def check(x, adapter_end, polya_end, params, return_values=False, less_signal_ok=False, windowed_stats=True):
    """mvs.py:45-158"""
    integer = np.issubdtype(np.asarray(x).dtype, np.integer)
    x = work(x)
    sig_size = x.size
    failed = (False, np.zeros(5).astype(bool), 0.0, 0.0, 0.0, 0.0, 0.0) if return_values else False
    ae, pe = adapter_end, polya_end
    if pe == 0 or ae == 0 or pe < ae or pe - ae <= 2:
        return failed
    if not less_signal_ok and sig_size < ae + params.median_shift_window:
        return failed
    seg = x[ae:pe]
    if windowed_stats:
        if pe - ae <= params.pA_var_window + 2:
            var = np.var(seg)
        else:
            var = nanmedian(move_var(seg, params.pA_var_window))
        if pe - ae <= params.pA_mean_window + 2:
            mean = np.mean(seg)
        else:
            mean = nanmedian(move_mean(seg, params.pA_mean_window))
    else:
        mean = np.mean(seg)
        var = np.var(seg)
    med = median(seg)
    p85, p15 = percentile_pair(seg, integer)
    lr = p85 - p15
    shift = median(x[ae:min(ae + params.median_shift_window, sig_size)]) - median(x[max(ae - params.median_shift_window, 0):ae])
    vals = (float(mean), float(var), float(med), float(lr), float(shift))
    vec = np.array([in_range_scalar(vals[0], params.pA_mean_range), in_range_scalar(vals[1], params.pA_var_range),
                    in_range_scalar(vals[2], params.polyA_med_range), in_range_scalar(vals[3], params.polyA_local_range),
                    in_range_scalar(vals[4], params.median_shift_range)])
    return (vec.all(), vec) + vals if return_values else vec.all()


def detect_at_loc(x, loc, params, return_values=False, less_signal_ok=True):
    """mvs.py:181-338"""
    integer = np.issubdtype(np.asarray(x).dtype, np.integer)
    x = work(x)
    sig_size = x.size
    fail = (False, 0, 0.0, 0.0, 0.0, 0.0, 0.0) if return_values else False
    if not less_signal_ok and sig_size < loc + params.search_window + max(params.median_shift_window, params.polyA_window):
        return fail
    if loc < max(params.pA_mean_window, params.pA_var_window):
        return fail
    offset = max(params.pA_mean_window, params.pA_var_window)
    seg = x[loc - offset:loc + params.search_window]
    mm = move_mean(seg, params.pA_mean_window)
    mv = move_var(seg, params.pA_var_window)
    match = in_range_arr(mm, params.pA_mean_range) & in_range_arr(mv, params.pA_var_range)
    idx = int(np.argmax(match))
    if idx > 0:
        mean, var = mm[idx], mv[idx]
        idx += loc - offset
    else:
        if 2 * offset >= mm.size:
            raise RefIndexError("index %d is out of bounds for axis 0 with size %d" % (2 * offset, mm.size))
        mean, var = mm[2 * offset], mv[2 * offset]
    loc_ = max(loc, idx)
    pa = x[loc_:min(loc_ + params.polyA_window, sig_size)]
    med = median(pa)
    p85, p15 = percentile_pair(pa, integer)
    shift = median(x[loc_:min(loc_ + params.median_shift_window, sig_size)]) - median(x[:loc_])
    vals = (float(mean), float(var), float(med), float(p85 - p15), float(shift))
    ok = (idx > 0 and in_range_scalar(vals[2], params.polyA_med_range) and in_range_scalar(vals[3], params.polyA_local_range)
          and in_range_scalar(vals[4], params.median_shift_range))
    ok = bool(ok)
    return (ok, idx) + vals if return_values else ok


def detect(x, params):
    """mvs.py:341-426"""
    x = work(x)
    sig_size = x.size
    mo = params.min_obs_adapter
    if sig_size < mo + max(params.pA_mean_window, params.pA_var_window, params.min_obs_post_loc, params.polyA_window):
        return 0
    mm = move_mean(x[mo:], params.pA_mean_window)
    mv = move_var(x[mo:], params.pA_var_window)
    match = np.asarray(in_range_arr(mm, params.pA_mean_range) & in_range_arr(mv, params.pA_var_range))
    offset = max(params.pA_mean_window, params.pA_var_window)
    while offset < sig_size - mo:
        rest = match[offset:]
        j = int(np.argmax(rest))
        if j > 0 or rest[0]:
            idx = mo + offset + j
            if sig_size - idx < params.min_obs_post_loc:
                return 0
            pa = x[idx:min(idx + params.polyA_window, sig_size)]
            shift = median(x[idx:min(idx + params.median_shift_window, sig_size)]) - median(x[max(idx - params.median_shift_window, 0):idx])
            p85, p15 = percentile_pair(pa)
            if (in_range_scalar(median(pa), params.polyA_med_range) and in_range_scalar(p85 - p15, params.polyA_local_range)
                    and in_range_scalar(float(shift), params.median_shift_range)):
                return np.int64(idx)
            offset = idx - mo + params.search_increment_step
            continue
        return 0
    return 0


def run(fn, *a, **k):
    """the result, or the exception as ("raise", type name, message)"""
    try:
        return fn(*a, **k)
    except (IndexError, ValueError) as e:
        return ("raise", "IndexError" if isinstance(e, IndexError) else "ValueError", str(e))
