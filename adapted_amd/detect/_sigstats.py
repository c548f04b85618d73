"""What the signal statistics drop-ins share (partition/signal_partitions.py, detect/normalize.py, downscale.py, real_range.py,
anomalies.py): the dtype rule, the [n, L] input, positions and segments."""
from __future__ import annotations

import numpy as np

from ._c_llr import _engine  # noqa: F401  (the modules' engine)
from ._rows import as_rows


def work_dtype(dt) -> np.dtype:
    """float32 computes in float32, float64 in float64, integers are widened to float64"""
    dt = np.dtype(dt)
    if dt == np.float32 or dt == np.float64:
        return dt
    if np.issubdtype(dt, np.integer):
        return np.dtype(np.float64)
    raise TypeError("signals must be float32, float64 or integer, not %s" % dt)


def as_work(signal) -> np.ndarray:
    """a host array in its working dtype, C-contiguous"""
    x = np.asarray(signal)
    return np.ascontiguousarray(x, dtype=work_dtype(x.dtype))


def rows_in(signals, lens, n, L, dtype):
    """host signals -> (C-contiguous float32 / float64 [n, L] array, lens, f64, n); a device pointer passes through"""
    x, lens = as_rows(signals, lens, n, L, work_dtype, "signals")
    if isinstance(x, int):
        dt = np.dtype(dtype)
        if dt not in (np.float32, np.float64):
            raise TypeError("device signals must be float32 or float64")
        if lens.size != int(n):
            raise ValueError("need one length per read")
        return x, lens, dt == np.float64, int(n)
    if x.shape[1] == 0:  # (the library wants L >= 1: every read is empty)
        x = np.zeros((x.shape[0], 1), dtype=x.dtype)
    return x, lens, x.dtype == np.float64, x.shape[0]


def positions(v, nn, what, none_ok=False):
    """one position per read -> int64 [n]; -1 stands for the reference's None where that is allowed"""
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    if v.size != nn:
        raise ValueError("%s needs one entry per read" % what)
    if v.size and v.min() < (-1 if none_ok else 0):
        raise ValueError("%s must be >= 0%s (negative positions are not supported)" % (what, ", or -1 for None" if none_ok else ""))
    return v


def position(v, what, none_ok=False):
    if v is None and none_ok:
        return -1
    v = int(v)
    if v < 0:
        raise ValueError("%s must be >= 0 (negative positions are not supported)" % what)
    return v


def bounds(r):
    """a (min, max) range with None for an open end -> (float, float)"""
    lo, hi = (None, None) if r is None else r
    lo, hi = (-np.inf if lo is None else float(lo), np.inf if hi is None else float(hi))
    if lo != lo or hi != hi:
        raise ValueError("a range bound must be a number or None")
    return lo, hi
