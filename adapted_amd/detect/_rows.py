"""What the module drop-ins' batch forms share (_c_llr, llr, mvs, normalize, downscale, real_range, anomalies, partition/
signal_partitions): their engine, the [n, L] input -- a host array, or a device pointer (int) with n and L, and one length per
read --, the dtype rule, positions and ranges.  Each caller keeps its own exceptions beyond these."""
from __future__ import annotations

import numpy as np

from .. import lib
from ..lib import bounds  # noqa: F401  (a (min, max) range -> floats: the same conversion the engine's configuration takes)

_ENGINE = None


def _engine(device: int = 0):
    """the modules' engine (their entry points read nothing from the configuration)"""
    global _ENGINE
    if _ENGINE is None or _ENGINE.device != device:
        from ..config import get_chemistry_specific_config

        spc = get_chemistry_specific_config("RNA004")
        _ENGINE = lib.Engine(spc, 1, spc.sig_preload_size, device=device)
    return _ENGINE


def as_rows(x, lens, n, L, work_dtype, what, min_len=0, lens_msg=None):
    """-> (x as a C-contiguous [n, L] array of work_dtype(x.dtype) -- a device pointer passes through --, lens int64 [n]).
    ValueError: a device pointer without n and L, a host array that is not 2-D, lens not one per read in [min_len, L]"""
    if isinstance(x, int):
        if n is None or L is None:
            raise ValueError("a device pointer needs n and L")
        return x, np.asarray(lens, dtype=np.int64).reshape(-1)
    x = np.asarray(x)
    x = np.ascontiguousarray(x, dtype=work_dtype(x.dtype))
    if x.ndim != 2:
        raise ValueError("%s must be [n, L]" % what)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if lens.size != x.shape[0] or (lens.size and (lens.min() < min_len or lens.max() > x.shape[1])):
        raise ValueError(lens_msg or "need one length per read, %d <= lens <= L" % min_len)
    return x, lens


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


def rows_in(signals, lens, n, L, dtype, count_lens=True):
    """host signals -> (C-contiguous float32 / float64 [n, L] array, lens, f64, n); a device pointer passes through, its lens
    counted here unless ``count_lens`` is off (the MVS forms: the engine counts them, behind their return for n == 0)"""
    x, lens = as_rows(signals, lens, n, L, work_dtype, "signals")
    if isinstance(x, int):
        dt = np.dtype(dtype)
        if dt not in (np.float32, np.float64):
            raise TypeError("device signals must be float32 or float64")
        if count_lens and lens.size != int(n):
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
