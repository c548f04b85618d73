"""The event segmentation of adp_segment_events (include/adapted_hip_events.h) in numpy + scipy: its exact oracle.  Every
operation is float64 in the order the header writes it, so device results are compared bit for bit."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy.signal import find_peaks


def clip(signal_row, length, start, end):
    """signal[row, start:end] as adp_seg clips it: to the read's length; start < 0 or end <= start gives an empty slice"""
    if start < 0 or end <= start:
        return np.asarray(signal_row)[:0]
    return np.asarray(signal_row)[:length][start:end]


def scores(x, w, var_floor):
    """the squared two-window t-statistic of every position of x (float64 [n]); 0.0 outside [w, n - w]"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    out = np.zeros(n)
    if n < 2 * w:
        return out
    win = sliding_window_view(x, w)  # [n - w + 1, w]
    s = np.zeros(win.shape[0])
    for k in range(w):
        s = s + win[:, k]
    mean = s / w
    q = np.zeros(win.shape[0])
    for k in range(w):
        d = win[:, k] - mean
        q = q + d * d
    var = q / w
    i = np.arange(w, n - w + 1)
    d = mean[i - w] - mean[i]
    den = var[i - w] + var[i]
    den = np.where(den < var_floor, var_floor, den)
    out[i] = ((d * d) * w) / den
    return out


def segment(x, w=8, D=8, thr=16.0, var_floor=1e-3):
    """-> (boundaries int64, status, median gap, MAD of the gaps)"""
    x = np.asarray(x, dtype=np.float64)
    nan = float("nan")
    none = np.zeros(0, dtype=np.int64)
    if np.isnan(x).any():
        return none, 1, nan, nan
    if x.size < 2 * w:
        return none, 2, nan, nan
    b = find_peaks(scores(x, w, var_floor), height=thr, distance=D)[0].astype(np.int64)
    if b.size < 2:
        return b, 0, nan, nan
    gaps = np.diff(b)
    med = np.median(gaps)
    return b, 0, float(med), float(np.median(np.abs(gaps - med)))


def candidates(x, w, thr, var_floor):
    """the maxima the distance rule chooses among, and their heights"""
    sc = scores(x, w, var_floor)
    c = find_peaks(sc, height=thr)[0]
    return c, sc[c]


def has_close_ties(x, w, D, thr, var_floor):
    """do two candidates closer than D have equal scores (where scipy's order and the library's may part)?"""
    x = np.asarray(x, dtype=np.float64)
    if x.size < 2 * w or np.isnan(x).any():
        return False
    c, h = candidates(x, w, thr, var_floor)
    for a in range(c.size):
        b = a + 1
        while b < c.size and c[b] - c[a] < D:
            if h[a] == h[b]:
                return True
            b += 1
    return False


def staircase(rng, n, level_sd=12.0, level_mean=85.0, dwell=(5, 40), noise_sd=2.0, dtype=np.float32):
    """a staircase of n samples: levels N(level_mean, level_sd^2), a dwell drawn per event, Gaussian noise"""
    if n == 0:
        return np.zeros(0, dtype=dtype)
    dw = rng.integers(dwell[0], dwell[1] + 1, size=n // dwell[0] + 2)
    lv = rng.normal(level_mean, level_sd, size=dw.size)
    x = np.repeat(lv, dw)[:n] + rng.normal(0.0, noise_sd, size=n)
    return x.astype(dtype)
