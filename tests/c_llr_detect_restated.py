"""The best-split segmenters of the reference's `_c_llr` (adapted/detect/_c_llr.pyx:40-64, :239-433) restated on the CPU oracle's
gains (``oracle.c_llr_trace``: the reference's formula with the same libm, so its gains are the reference's bit for bit) plus
numpy's own arg-max and median: the yardstick of the GPU tests beyond the fixture's cases.  ``orc`` is the oracle module."""
import warnings

import numpy as np


def best_split_gains(orc, start, end, c, c2, offset_head, offset_tail):
    """_best_split (:40-64) -> (x, split_gain, gains): the loop's winner is the first index of the maximum among gains > 0"""
    g = orc.c_llr_trace(None, start, end, offset_head, offset_tail, sums=(c, c2))
    lo, hi = start + offset_head, end - offset_tail
    if hi <= lo:
        return -1, 0.0, g
    seg = g[lo:hi]
    ok = seg > 0  # (NaN compares false)
    if not ok.any():
        return -1, 0.0, g
    k = int(np.argmax(np.where(ok, seg, -np.inf)))
    return lo + k, float(seg[k]), g


def best_split(orc, start, end, c, c2, offset_head, offset_tail):
    return best_split_gains(orc, start, end, c, c2, offset_head, offset_tail)[:2]


def median(x):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (numpy warns on an empty segment and returns NaN)
        return float(np.median(x))


def detect(orc, raw, min_obs_adapter, border_trim, min_obs_polya=None):
    """c_llr_detect_adapter (min_obs_polya None) / c_llr_detect_adapter_polya -> dict: `result` (the reference's tuple), `splits`
    [x_first, x_head, x_tail, x_polya] as the searches returned them, `gains` (their split gains), `gain_arrays` (the four gain
    arrays, None where not searched), `medians`, `branch` and `flags` (which paths of the reference the read took)"""
    raw = np.asarray(raw, dtype=np.float64)
    c = np.cumsum(raw)
    c2 = np.cumsum(np.multiply(raw, raw))
    length = len(raw) - 1
    mo, bt = min_obs_adapter, border_trim
    out = dict(splits=[-1, -1, -1, -1], gains=[0.0] * 4, gain_arrays=[None] * 4, medians=[np.nan] * 4, flags=set())
    xf, gf, a0 = best_split_gains(orc, 0, length, c, c2, mo + bt, bt)
    out["splits"][0], out["gains"][0], out["gain_arrays"][0] = xf, gf, a0
    if xf == -1:
        out.update(result=(0, 0), branch="no_first_split")
        return out
    xh, gh, a1 = best_split_gains(orc, 0, xf, c, c2, bt, mo)
    xt, gt, a2 = best_split_gains(orc, xf, length, c, c2, mo, bt)
    out["splits"][1:3], out["gains"][1:3], out["gain_arrays"][1:3] = [xh, xt], [gh, gt], [a1, a2]
    if xh == -1:
        xh = 1
        out["flags"].add("head_fallback")
    if xt == -1:
        xt = xf + 1
        out["flags"].add("tail_fallback")
    m = np.zeros(4)
    m[0] = median(raw[:xh])
    m[1] = median(raw[xh:xf])
    m[2] = median(raw[xf:xt])
    m[3] = median(raw[xt:])
    out["medians"] = [float(v) for v in m]
    diffs = np.diff(m)
    if diffs[1] > 0:
        if m[0] >= m.mean():
            s, e, br = xh, xf, "full_adapter"
        else:
            s, e, br = 0, xf, "partial_adapter"
    elif gt > gh:
        s, e, br = xf, xt, "first_split_is_adapter_start"
    else:
        s, e, br = 0, 0, "none_by_decision"
    out["branch"] = br
    if min_obs_polya is None:
        out["result"] = (s, e)
        return out
    if e == 0:
        out["result"] = (0, 0, 0)
        return out
    xp, gp, a3 = best_split_gains(orc, e, length, c, c2, min_obs_polya, bt)
    out["splits"][3], out["gains"][3], out["gain_arrays"][3] = xp, gp, a3
    if xp == -1:
        out["flags"].add("polya_not_found")
        xp = 0
    out["result"] = (s, e, xp)
    return out


def traces(orc, raw, min_obs_adapter, border_trim, min_obs_polya=None):
    """c_llr_detect_adapter_trace / c_llr_boundary_traces (:368-385, :415-433), with min_obs_polya
    c_llr_detect_adapter_polya_trace (:388-412): each level starts at np.argmax of the one before"""
    raw = np.asarray(raw, dtype=np.float64)
    c = np.cumsum(raw)
    c2 = np.cumsum(np.multiply(raw, raw))
    length = len(raw) - 1
    mo, bt = min_obs_adapter, border_trim
    g1 = orc.c_llr_trace(None, 0, length, mo + bt, bt, sums=(c, c2))
    xf = int(np.argmax(g1))
    g2 = orc.c_llr_trace(None, 0, xf, bt, mo, sums=(c, c2))
    g3 = orc.c_llr_trace(None, xf, length, mo, bt, sums=(c, c2))
    if min_obs_polya is None:
        return g1, g2, g3
    xl = int(np.argmax(g3))
    return g1, g2, g3, orc.c_llr_trace(None, xl, length, min_obs_polya, bt, sums=(c, c2))
