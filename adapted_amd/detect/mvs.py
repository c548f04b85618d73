"""The reference's MVS poly(A) module ``adapted.detect.mvs`` (adapted/detect/mvs.py) on the HIP library: its three functions with
the same arguments, defaults and return types, so that ``from adapted.detect.mvs import ...`` can become
``from adapted_amd.detect.mvs import ...``.  Next to them sit their batch forms (``*_batch``): padded [n, L] signals with per-read
lengths (read r is ``signals[r, :lens[r]]``), or a device pointer (int) with ``n``, ``L`` and ``dtype``, so that resident signals
never cross PCIe.

Every per-read function is one batch call with n = 1 (adp_mvs_check, adp_mvs_detect_at_loc, adp_mvs_detect: adapted_amd/csrc/
mvs_api.h).  There is no CPU path: without the HIP library every function raises ``HipLibraryError``.

Dtypes follow bottleneck and numpy: float32 input computes in float32 (bottleneck's recurrences, numpy's medians and sums),
float64 in float64; integer input is widened to float64 (what bottleneck's native integer path computes; the reference's
bottleneck 1.3.2 sends int8 / int16 / unsigned input to a pure-Python fallback that fails under numpy >= 1.24, int32 / int64 to
the native path); anything else raises TypeError.  Where the reference raises -- IndexError when nothing matches and the moving
series is shorter than 2 * offset + 1, or for np.percentile of an empty slice; bottleneck's ValueError when a slice is shorter
than its window -- the per-read functions raise the same exception type and message, and the batch forms mark the read in
``status`` (1 IndexError, 2 ValueError).

Differences from the reference: negative positions (adapter_end, polya_end, loc) raise ValueError (the reference gives them
Python's slice wrap-around meaning); windows below 1 and a search_increment_step below 1 raise ValueError (the reference fails
inside bottleneck, or never returns).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import lib
from ..config.schema import MVSPolyAConfig, StreamingConfig
from ._rows import _engine, bounds, position, positions, rows_in
from ._rows import work_dtype as _work_dtype  # noqa: F401  (the module's dtype rule under its name here)
from .utils import LOCAL_RANGE_PCTLS, in_range  # noqa: F401  (the reference module imports both from here)

ST_INDEX, ST_VALUE = 1, 2  # `status` of the batch forms (0: the reference returns)


def _args(params=None, stream=None, less_signal_ok=False, windowed_stats=True) -> "lib.AdpMvsArgs":
    a = lib.AdpMvsArgs()
    if params is not None:
        for k in ("pA_mean_range", "pA_var_range", "median_shift_range", "polyA_med_range", "polyA_local_range"):
            getattr(a, k)[:] = bounds(getattr(params, k), nan_ok=True)
        for k in ("search_window", "pA_mean_window", "pA_var_window", "median_shift_window", "polyA_window"):
            setattr(a, k, int(getattr(params, k)))
    else:
        a.pA_mean_window = a.pA_var_window = 1
    if stream is not None:
        for k in ("pA_mean_range", "pA_var_range", "median_shift_range", "polyA_med_range", "polyA_local_range"):
            getattr(a, "s_" + k)[:] = bounds(getattr(stream, k), nan_ok=True)
        for k in ("pA_mean_window", "pA_var_window", "median_shift_window", "polyA_window"):
            setattr(a, "s_" + k, int(getattr(stream, k)))
        a.min_obs_adapter, a.min_obs_post_loc = int(stream.min_obs_adapter), int(stream.min_obs_post_loc)
        a.search_increment_step = int(stream.search_increment_step)
    else:
        a.s_pA_mean_window = a.s_pA_var_window = a.search_increment_step = 1
    a.less_signal_ok, a.windowed_stats = int(bool(less_signal_ok)), int(bool(windowed_stats))
    if min(a.pA_mean_window, a.pA_var_window, a.s_pA_mean_window, a.s_pA_var_window) < 1:
        raise ValueError("pA_mean_window and pA_var_window must be >= 1")
    if a.search_increment_step < 1:
        raise ValueError("search_increment_step must be >= 1 (the reference never returns otherwise)")
    if min(a.min_obs_adapter, a.min_obs_post_loc) < 0:
        raise ValueError("min_obs_adapter and min_obs_post_loc must be >= 0")
    return a


def _check_raw(signals, lens, adapter_ends, polya_ends, params, less_signal_ok=False, windowed_stats=True, n=None, L=None,
                    dtype=np.float32, device=0):
    """adp_mvs_check as it comes: (info int32 [n, 8], vals float64 [n, 5]) -- include/adapted_hip.h"""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype, count_lens=False)
    ae, pe = positions(adapter_ends, nn, "adapter_ends"), positions(polya_ends, nn, "polya_ends")
    a = _args(params, None, less_signal_ok, windowed_stats)
    if nn == 0:
        return np.zeros((0, 8), dtype=np.int32), np.zeros((0, 5))
    return _engine(device).mvs_check(x, lens, ae, pe, a, n=n, L=L, f64=f64)


def mean_var_shift_polyA_check_batch(signals, lens, adapter_ends, polya_ends, params, less_signal_ok=False, windowed_stats=True,
                                     device=0, n: Optional[int] = None, L: Optional[int] = None, dtype=np.float32,
                                     return_status: bool = False):
    """`mean_var_shift_polyA_check` for many reads -> (ok bool [n], check_vector bool [n, 5], values float64 [n, 5]) and, with
    ``return_status``, status int32 [n] (1: the reference raises IndexError, 2: ValueError).  values: mean, var, poly(A) median,
    local range, median shift (0.0 where the reference returns its failed result)"""
    info, vals = _check_raw(signals, lens, adapter_ends, polya_ends, params, less_signal_ok, windowed_stats, n, L, dtype, device)
    ok = info[:, 0] != 0
    vec = ((info[:, 1:2] >> np.arange(5)) & 1).astype(bool)
    return (ok, vec, vals, info[:, 2].copy()) if return_status else (ok, vec, vals)


def mean_var_shift_polyA_detect_at_loc_batch(signals, lens, locs, params, less_signal_ok=True, device=0, n: Optional[int] = None,
                                             L: Optional[int] = None, dtype=np.float32):
    """`mean_var_shift_polyA_detect_at_loc` for many reads -> (ok bool [n], idx int64 [n], values float64 [n, 5], status int32 [n])"""
    ok, idx, vals, info = _at_loc_raw(signals, lens, locs, params, less_signal_ok, n, L, dtype, device)
    return ok, idx, vals, info[:, 2].copy()


def _at_loc_raw(signals, lens, locs, params, less_signal_ok, n, L, dtype, device):
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype, count_lens=False)
    lo = positions(locs, nn, "locs")
    a = _args(params, None, less_signal_ok, True)
    if nn == 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64), np.zeros((0, 5)), np.zeros((0, 8), dtype=np.int32)
    info, idx, vals = _engine(device).mvs_detect_at_loc(x, lens, lo, a, n=n, L=L, f64=f64)
    return info[:, 0] != 0, idx, vals, info


def mean_var_shift_polyA_detect_batch(signals, lens, params=None, device=0, n: Optional[int] = None, L: Optional[int] = None,
                                      dtype=np.float32):
    """`mean_var_shift_polyA_detect` for many reads -> int64 [n] (0: none found)"""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype, count_lens=False)
    a = _args(None, StreamingConfig() if params is None else params)
    if nn == 0:
        return np.zeros(0, dtype=np.int64)
    return _engine(device).mvs_detect(x, lens, a, n=n, L=L, f64=f64)


def _raise(info_row, integer=False):
    st, a, b = int(info_row[2]), int(info_row[3]), int(info_row[4])
    if st == ST_INDEX:
        if a == -1 and integer:  # (numpy's percentile of an empty integer slice reports index 0)
            a = 0
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (a, b))
    if st == ST_VALUE:
        raise ValueError("Moving window (=%d) must between 1 and %d, inclusive" % (a, b))


def _one(calibrated_signal):
    x = np.asarray(calibrated_signal).reshape(1, -1)
    return x, [x.shape[1]], np.issubdtype(x.dtype, np.integer)


def mean_var_shift_polyA_check(calibrated_signal, adapter_end, polya_end, params, return_values=False, less_signal_ok=False,
                               windowed_stats=True):
    """mvs.py:45-158 -> check_vector.all() (np.bool_; False on the early outs), or with ``return_values`` the tuple
    (ok, check_vector bool [5], mean, var, polya_med, polya_local_range, med_shift)"""
    x, lens, integer = _one(calibrated_signal)
    info, vals = _check_raw(x, lens, [position(adapter_end, "adapter_end")], [position(polya_end, "polya_end")], params,
                                 less_signal_ok, windowed_stats)
    _raise(info[0], integer)
    if not info[0, 5]:
        return (False, np.zeros(5).astype(bool), 0.0, 0.0, 0.0, 0.0, 0.0) if return_values else False
    vec = ((int(info[0, 1]) >> np.arange(5)) & 1).astype(bool)
    ok = vec.all()
    if not return_values:
        return ok
    return (ok, vec) + tuple(float(v) for v in vals[0])


def mean_var_shift_polyA_detect_at_loc(calibrated_signal, loc=0, params=MVSPolyAConfig(), return_values=False, less_signal_ok=True):
    """mvs.py:181-338 -> bool, or with ``return_values`` (found, idx, mean, var, polya_med, polya_local_range, med_shift)"""
    x, lens, integer = _one(calibrated_signal)
    ok, idx, vals, info = _at_loc_raw(x, lens, [position(loc, "loc")], params, less_signal_ok, None, None, np.float32, 0)
    _raise(info[0], integer)
    res = bool(ok[0])
    if not return_values:
        return res
    return (res, int(idx[0])) + tuple(float(v) for v in vals[0])


def mean_var_shift_polyA_detect(calibrated_signal, params=StreamingConfig()):
    """mvs.py:341-426: the streaming detector -> the poly(A) start (np.int64), or the int 0"""
    x, lens, _ = _one(calibrated_signal)
    r = int(mean_var_shift_polyA_detect_batch(x, lens, params)[0])
    return np.int64(r) if r else 0


__all__ = ["mean_var_shift_polyA_check", "mean_var_shift_polyA_detect_at_loc", "mean_var_shift_polyA_detect",
           "mean_var_shift_polyA_check_batch", "mean_var_shift_polyA_detect_at_loc_batch", "mean_var_shift_polyA_detect_batch"]
