"""The reference's anomalies module ``adapted.detect.anomalies`` on the HIP library: `find_open_pores` with the same arguments,
defaults and return shapes, and `find_open_pores_batch` for the slices ``signals[r, starts[r]:ends[r]]`` of a padded [n, L] batch
(a host array with ``lens``, or a device pointer with ``n``, ``L`` and ``dtype``).  One call of adp_open_pores (adapted_amd/csrc/
sigstats_api.h), repeated with a larger cap when a list did not fit; there is no CPU path.

What the reference returns, and this returns alike: the positions in range whose distance to the PRECEDING position in range
(kept or not) is at least ``min_obs_diff``, as an int64 array of shape (k, 1); when there are none of those, the LAST position in
range alone, with shape (1,); when at most one position is in range, ``np.argwhere``'s own result, with shape (0, 1) or (1, 1).
float32 samples are compared with the bounds rounded to float32, as numpy compares a float32 array with Python floats; integer
input is widened to float64.  Differences: the signal must be 1-D; negative positions raise ValueError.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from ._rows import _engine, as_work, bounds, positions, rows_in
from .utils import in_range  # noqa: F401  (the reference module imports it from here)


def _raw(signals, lens, starts, ends, sig_range, min_obs_diff, cap, device, n, L, dtype):
    """adp_open_pores as it comes: (pos int64 [n, cap'], counts int64 [n, 3]: kept, in range, the last in range)"""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    s, e = positions(starts, nn, "starts"), positions(ends, nn, "ends")
    lo, hi = bounds(sig_range)
    if nn == 0:
        return np.full((0, max(int(cap), 1)), -1, dtype=np.int64), np.zeros((0, 3), dtype=np.int64)
    return _engine(device).open_pores(x, lens, np.arange(nn, dtype=np.int32), s, e, lo, hi, float(min_obs_diff), cap, n=n, L=L, f64=f64)


def find_open_pores_batch(signals, lens, starts, ends, sig_range: Tuple[Optional[float], Optional[float]] = (200.0, None),
                          min_obs_diff: int = 10, cap: int = 16, device=0, n: Optional[int] = None, L: Optional[int] = None,
                          dtype=np.float32):
    """`find_open_pores` of ``signals[r, starts[r]:ends[r]]`` for many reads -> (positions int64 [n, cap'] from the slice's start,
    padded with -1; counts int64 [n]: the length of the reference's result; in_range int64 [n]: how many positions are in
    range).  cap' is ``cap`` or, when a read has more, the largest count: no list is cut short"""
    pos, cnt = _raw(signals, lens, starts, ends, sig_range, min_obs_diff, cap, device, n, L, dtype)
    kept, inr, last = cnt[:, 0].copy(), cnt[:, 1], cnt[:, 2]
    alone = (kept == 0) & (inr > 0)  # (nothing far enough from its predecessor: the last position in range)
    pos[alone, 0] = last[alone]
    kept[alone] = 1
    return pos, kept, inr.copy()


def find_open_pores(signal: np.ndarray, sig_range: Tuple[Optional[float], Optional[float]] = (200.0, None), min_obs_diff: int = 10):
    x = as_work(signal)
    if x.ndim != 1:
        raise ValueError("signal must be 1-D")
    if x.size == 0:
        return np.zeros((0, 1), dtype=np.int64)
    pos, cnt = _raw(x.reshape(1, -1), [x.size], [0], [x.size], sig_range, min_obs_diff, 16, 0, None, None, None)
    kept, inr, last = (int(v) for v in cnt[0])
    if inr <= 1:  # (np.argwhere's own result)
        return np.full((inr, 1), last, dtype=np.int64)
    if kept == 0:
        return np.array([last], dtype=np.int64)
    return pos[0, :kept].reshape(-1, 1).copy()


__all__ = ["find_open_pores", "find_open_pores_batch"]
