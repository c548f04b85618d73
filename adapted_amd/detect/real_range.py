"""The reference's real-range module ``adapted.detect.real_range`` on the HIP library: `real_range_check` with the same
arguments, defaults and return types, and `real_range_check_batch` for the slices ``signals[r, starts[r]:ends[r]]`` of a padded
[n, L] batch (a host array with ``lens``, or a device pointer with ``n``, ``L`` and ``dtype``) -- the reference calls the check
on ``signal[adapter_start:adapter_end]``.  One call of adp_real_range (adapted_amd/csrc/sigstats_api.h); there is no CPU path.

The two means come back in the input's type (np.float32 / np.float64; integers are widened to float64), the local range as
np.float64 -- numpy's percentile interpolates in float64 also for float32 input.  Differences from the reference: negative
positions, a ``mean_window`` below 1 and a ``max_obs_local_range`` below 1 raise ValueError.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import lib
from ..config.schema import RealRangeConfig
from ._rows import _engine, as_work, bounds, positions, rows_in
from .utils import LOCAL_RANGE_PCTLS, in_range  # noqa: F401  (the reference module imports both from here)

STAGE_SHORT, STAGE_MEANS, STAGE_LOCAL_RANGE = 0, 1, 2  # `stage` of the batch form


def _args(params: RealRangeConfig) -> "lib.AdpRealRangeArgs":
    a = lib.AdpRealRangeArgs()
    for k in ("mean_start_range", "mean_end_range", "local_range"):
        getattr(a, k)[:] = bounds(getattr(params, k))
    a.mean_window, a.max_obs_local_range = int(params.mean_window), int(params.max_obs_local_range)
    if a.mean_window < 1 or a.max_obs_local_range < 1:
        raise ValueError("mean_window and max_obs_local_range must be >= 1")
    return a


def real_range_check_batch(signals, lens, starts, ends, params: RealRangeConfig, device=0, n: Optional[int] = None,
                           L: Optional[int] = None, dtype=np.float32):
    """`real_range_check` of ``signals[r, starts[r]:ends[r]]`` for many reads -> (ok bool [n]; values float64 [n, 3]: mean_start,
    mean_end, local range; stage int32 [n]: 0 -- fewer than 2 * mean_window samples, the reference returns no values (NaN here);
    1 -- a mean is out of range, no local range (NaN); 2 -- all three)"""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    s, e = positions(starts, nn, "starts"), positions(ends, nn, "ends")
    a = _args(params)
    if nn == 0:
        return np.zeros(0, dtype=bool), np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
    info, vals = _engine(device).real_range(x, lens, np.arange(nn, dtype=np.int32), s, e, a, n=n, L=L, f64=f64)
    stage = info[:, 1].copy()
    vals[stage < STAGE_MEANS, :2] = np.nan
    vals[stage < STAGE_LOCAL_RANGE, 2] = np.nan
    return info[:, 0] != 0, vals, stage


def real_range_check(calibrated_signal: np.ndarray, params: RealRangeConfig, return_values=False):
    """Checks that signal start with adapter, ends with polyA tail and has a sufficient local range."""
    x = as_work(calibrated_signal).reshape(1, -1)
    if x.shape[1] < 2 * params.mean_window:
        _args(params)
        return (False, None, None, None) if return_values else False
    ok, vals, stage = real_range_check_batch(x, [x.shape[1]], [0], [x.shape[1]], params)
    if not return_values:
        return bool(ok[0])
    m0, m1 = x.dtype.type(vals[0, 0]), x.dtype.type(vals[0, 1])
    if stage[0] < STAGE_LOCAL_RANGE:
        return (False, m0, m1, None)
    return (bool(ok[0]), m0, m1, np.float64(vals[0, 2]))


__all__ = ["real_range_check", "real_range_check_batch"]
