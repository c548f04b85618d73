"""The reference's adapter-start module ``adapted.detect.adapter_start`` on the HIP library: `moving_mean_adapter_start_detect`
with the same arguments and return types, so that ``from adapted.detect.adapter_start import ...`` can become
``from adapted_amd.detect.adapter_start import ...``.  Next to it sits `moving_mean_adapter_start_detect_batch`: padded [n, L]
signals with per-read lengths (read r is ``signals[r, :lens[r]]``), or a device pointer (int) with ``n``, ``L`` and ``dtype``.

Both are one call of adp_adapter_start (k_adapter_start: adapted_amd/csrc/startmods_api.h).  There is no CPU path: without the
HIP library every function raises ``HipLibraryError``.  It is the package's only detector of the adapter's FRONT boundary; the
detect pipeline does not call it (nor does the reference's): ``DetectResults.adapter_start`` stays 0.

Dtypes follow bottleneck and numpy: float32 input runs move_mean and both cumulative sums in float32, float64 in float64, and the
means of those sums and their difference in float64 either way; integer input is widened to float64 (bottleneck's own rule);
anything else raises TypeError.  Where the reference raises -- bottleneck's ValueError when ``len - min_obs_adapter`` is shorter
than the window -- the per-read function raises the same exception type and message, and the batch form marks the read in
``status`` (2).

Differences from the reference: a negative min_obs_adapter raises ValueError (the reference gives it Python's slice wrap-around
meaning); the batch form refuses a window below 1 on the host.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import lib
from ..config.schema import MMAdapterStartConfig  # noqa: F401  (the reference module imports it from its configuration)
from ._rows import _engine, rows_in
from ._rows import work_dtype as _work_dtype  # noqa: F401  (the module's dtype rule under its name here)

ST_VALUE = 2  # `status` of the batch form (0: the reference returns)


def _args(params) -> "lib.AdpAdapterStartArgs":
    a = lib.AdpAdapterStartArgs()
    a.min_shift, a.min_pA_current = float(params.min_shift), float(params.min_pA_current)
    a.window, a.min_obs_adapter = int(params.window), int(params.min_obs_adapter)
    if a.window < 1:
        raise ValueError("window must be >= 1")
    if a.min_obs_adapter < 0:
        raise ValueError("min_obs_adapter must be >= 0 (negative positions are not supported)")
    return a


def _raw(signals, lens, params, n, L, dtype, device):
    """adp_adapter_start as it comes: (info int32 [n, 4], adapter_start, cand int64 [n], difference[cand] float64 [n])"""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    a = _args(params)
    if nn == 0:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    return _engine(device).adapter_start(x, lens, a, n=n, L=L, f64=f64)


def moving_mean_adapter_start_detect_batch(signals, lens, params, device=0, n: Optional[int] = None, L: Optional[int] = None,
                                           dtype=np.float32, details: bool = False):
    """`moving_mean_adapter_start_detect` for many reads -> (adapter_start int64 [n] (0: none accepted), status int32 [n]
    (2: the reference raises bottleneck's ValueError)) and, with ``details``, cand int64 [n] (np.argmin(difference); -1 where
    difference is empty or the reference raises) and difference[cand] float64 [n]"""
    info, out, cand, diff = _raw(signals, lens, params, n, L, dtype, device)
    status = info[:, 0].copy()
    return (out, status, cand, diff) if details else (out, status)


def moving_mean_adapter_start_detect(calibrated_signal: np.ndarray, params):
    """adapter_start.py:14-54 -> the adapter's start (np.int64), or the int 0"""
    x = np.asarray(calibrated_signal).reshape(1, -1)
    if int(params.window) < 1:  # (bottleneck's own check, on the slice the reference hands it)
        raise ValueError("Moving window (=%d) must between 1 and %d, inclusive" %
                         (int(params.window), max(x.shape[1] - max(int(params.min_obs_adapter), 0), 0)))
    info, out, _, _ = _raw(x, [x.shape[1]], params, None, None, np.float32, 0)
    if info[0, 0] == ST_VALUE:
        raise ValueError("Moving window (=%d) must between 1 and %d, inclusive" % (int(info[0, 1]), int(info[0, 2])))
    return np.int64(out[0]) if info[0, 3] else 0


__all__ = ["moving_mean_adapter_start_detect", "moving_mean_adapter_start_detect_batch"]
