"""The reference's LLR trace module (adapted/detect/llr.py) restated on the CPU oracle: scipy's find_peaks as ``oracle.find_peaks``,
np.nanstd in numpy's summation order as ``orc_np_nanstd_f64``, the traces as ``oracle.c_llr_trace``, the rest in numpy (np.interp,
np.argmin).  The yardstick of the GPU tests beyond the fixture's cases.  ``orc`` is the oracle module."""
import ctypes as C

import numpy as np


def nanstd(orc, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return float(orc.lib().orc_np_nanstd_f64(x.ctypes.data_as(C.POINTER(C.c_double)), C.c_long(x.size)))


def trace_state(sig, stride, min_obs, tail_trim):
    """LLRTrace (llr.py:53-142) -> dict(signal, start, end, early_stop); ValueError as numpy raises it"""
    sig = np.asarray(sig, dtype=np.float64)
    start = int(np.argmin(sig <= 0))
    end = int(sig.size - np.argmin(sig[::-1] <= 0) - 1)
    r = np.arange(min_obs, sig.size - 1 - tail_trim, stride)
    mlnes = r[-1] if r.size else sig.size - 1 - tail_trim
    out = dict(start=start, end=end, early_stop=bool(end < mlnes), signal=sig)
    if stride > 1:
        nz = np.where(sig[start:end] != 0)[0]
        out["signal"] = np.interp(np.arange(sig.size), nz + start, sig[nz + start], left=0, right=0)
    return out


def clip_bounds(size, start, end):
    a, b, _ = slice(start, end).indices(size)
    return a, max(a, b)


def find_peaks_in_trace(orc, sig, start, end, width=100, prominence=1.0, rel_height=0.5):
    a, b = clip_bounds(sig.size, start, end)
    clip = sig[a:b]
    sd = nanstd(orc, clip) if clip.size else float("nan")
    return orc.find_peaks(clip, prominence=prominence * sd, width=width, rel_height=rel_height).astype(np.int64) + a


def correct_for_plateau(sig, peak, s=10, t=0.9, window=500):
    tr = sig[peak: min(peak + window, sig.size)]
    changes = np.diff(tr)
    n = len(changes)
    plateau_end = -1
    for i in range(n - s, -1, -1):
        if (changes[i: i + (s - 1)] >= 0).all() and tr[i + (s - 1)] > t * tr[0]:
            plateau_end = i + (s - 1)
            break
    return peak + plateau_end if plateau_end > 0 else peak


def correct_for_split_peak(orc, sig, peak, s=10, t=0.9, window=500, prominence=1.0):
    w = sig[peak: min(peak + window, sig.size)]
    pk = orc.find_peaks(w, prominence=prominence, width=s, cap=1) if w.size >= 3 else np.zeros(0, dtype=np.int64)
    if pk.size and sig[pk[0] + peak] >= t * sig[peak]:
        return int(pk[0]) + peak
    return peak


def adapter_end_from_trace(orc, sig, start, end, prominence=1.0, rel_height=1.0, width=2000, fix_plateau=True, split=True,
                           plateau_args=(10, 0.9, 500), split_args=(10, 0.9, 500, 1.0)):
    peaks = find_peaks_in_trace(orc, sig, start, end, width, prominence, rel_height)
    if fix_plateau:
        peaks = np.array([correct_for_plateau(sig, int(p), *plateau_args) for p in peaks])
    if split:
        peaks = np.array([correct_for_split_peak(orc, sig, int(p), *split_args) for p in peaks])
    return peaks


def spike(orc, y, d=10, prom=1.0, width=10, ratio=0.5, r2=0.99):
    """detect_full_polya_trace_peak_with_spike (llr.py:406-479); ties under the distance: the later index first"""
    y = np.asarray(y, dtype=np.float64)
    pk = orc.find_peaks(np.nan_to_num(y, nan=0), distance=d, prominence=prom, width=width, rel_height=0.5)
    if pk.size == 0:
        return 0
    if pk.size == 1:
        return int(pk[0])
    h = y[pk]
    if h[1] > h[0]:
        return int(pk[1])
    if h[1] < h[0] * ratio:
        return int(pk[0])
    i = int(y[pk[0]:pk[1]].argmin()) + int(pk[0])
    x = np.arange(i, pk[1], dtype=np.float64)
    s = y[i:pk[1]]
    c = np.cov(x, s, bias=True)
    ssxm, ssxym, ssym = c[0, 0], c[0, 1], c[1, 1]
    r = 0.0 if (ssxm == 0.0 or ssym == 0.0) else float(np.clip(ssxym / np.sqrt(ssxm * ssym), -1.0, 1.0))
    return int(pk[1]) if r ** 2 >= r2 else 0

