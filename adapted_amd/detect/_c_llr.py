"""The reference's native module ``adapted.detect._c_llr`` (Cython, adapted/detect/_c_llr.pyx; imported at
adapted/detect/llr.py:18 as ``_gains, c_llr_trace, c_llr_trace_gains``) on the HIP library: every Python-visible name, with the
same arguments and return values.  The traces are computed by ``adp_c_llr_trace`` (adapted_amd/csrc/trace_api.h), `_best_split`
and the segmenters ``c_llr_detect_adapter`` / ``c_llr_detect_adapter_polya`` by ``adp_c_llr_best_split`` / ``adp_c_llr_detect``
(adapted_amd/csrc/llr_detect_api.h); their trace functions chain ``adp_c_llr_trace`` calls with numpy's arg-max in between.

A call per read pays a launch and two copies per trace -- the product path does not come through here (``adp_detect_llr`` runs
a whole minibatch in fused passes); these functions are the API-level drop-in, and ``c_llr_trace_batch`` is the form to use
for many reads.  There is no CPU path: without the HIP library every function raises ``HipLibraryError``.

Differences from the Cython module: values agree to ~1e-15 relative (the device logarithm is correctly rounded, glibc's is
not: DESIGN.md section 4) -- a split index can differ only where two gains tie to ~1e-15; index arguments outside
``0 <= start <= end <= len(signal)``, negative offsets and empty signals raise ``ValueError`` where the reference reads outside
its arrays (bounds checks are off there, _c_llr.pyx:21).
"""
from __future__ import annotations

import numpy as np

from .. import lib
from ._rows import _engine, as_rows  # noqa: F401  (_engine: the modules' engine, reached through this module too)


def _args(min_obs, border_trim, stride, adapter_early_stopping, adapter_early_stop_window, adapter_early_stop_stride,
          polya_early_stopping, polya_early_stop_window, polya_early_stop_stride) -> "lib.AdpTraceArgs":
    # the reference's asserts (_c_llr.pyx:102, :137-138)
    if polya_early_stopping > 0:
        assert adapter_early_stop_stride % stride == 0
        assert polya_early_stop_stride % stride == 0
    elif adapter_early_stopping > 0:
        assert adapter_early_stop_stride % stride == 0
    return lib.AdpTraceArgs(int(min_obs), int(border_trim), int(stride), int(adapter_early_stopping), int(adapter_early_stop_window),
                            int(adapter_early_stop_stride), int(polya_early_stopping), int(polya_early_stop_window),
                            int(polya_early_stop_stride))


def _check_range(start, end, n):
    if not (0 <= start <= end <= n):
        raise ValueError("need 0 <= start <= end <= len(signal) (got start=%d, end=%d, len=%d)" % (start, end, n))


def c_llr_trace_batch(raw_signals, lens, starts, ends, min_obs, border_trim, stride=1, adapter_early_stopping=0,
                      adapter_early_stop_window=500, adapter_early_stop_stride=100, polya_early_stopping=0,
                      polya_early_stop_window=50, polya_early_stop_stride=10, return_c_c2=0, sums=None, device: int = 0):
    """`c_llr_trace` for many reads in one call: raw_signals float64 [n, L] (read r valid in [0, lens[r])), per-read starts /
    ends -> gains float64 [n, L] (zeros beyond lens[r]), with ``return_c_c2`` also the cumulative sums.  ``sums=(c, c2)``:
    the form of `c_llr_trace_gains`."""
    a = _args(min_obs, border_trim, stride, adapter_early_stopping, adapter_early_stop_window, adapter_early_stop_stride,
              polya_early_stopping, polya_early_stop_window, polya_early_stop_stride)
    lens = np.asarray(lens, dtype=np.int64)
    for s, e, n in zip(np.asarray(starts).tolist(), np.asarray(ends).tolist(), lens.tolist()):
        _check_range(s, e, n)
    return _engine(device).c_llr_trace(raw_signals, lens, starts, ends, a, sums=sums, return_c_c2=bool(return_c_c2))


def c_llr_trace(raw_signal, start, end, min_obs, border_trim, stride=1, adapter_early_stopping=0, adapter_early_stop_window=500,
                adapter_early_stop_stride=100, polya_early_stopping=0, polya_early_stop_window=50, polya_early_stop_stride=10,
                return_c_c2=0):
    """_c_llr.pyx:202-236 -> gain, or (gain, c, c2) with ``return_c_c2``"""
    x = np.ascontiguousarray(raw_signal, dtype=np.float64).reshape(1, -1)
    n = x.shape[1]
    if n == 0:
        z = np.zeros(0)
        return (z, z.copy(), z.copy()) if return_c_c2 else z
    res = c_llr_trace_batch(x, [n], [start], [end], min_obs, border_trim, stride, adapter_early_stopping, adapter_early_stop_window,
                            adapter_early_stop_stride, polya_early_stopping, polya_early_stop_window, polya_early_stop_stride,
                            return_c_c2)
    if return_c_c2:
        return res[0][0], res[1][0], res[2][0]
    return res[0]


def c_llr_trace_gains(c, c2, start, end, min_obs, border_trim, stride=1, adapter_early_stopping=0, adapter_early_stop_window=500,
                      adapter_early_stop_stride=100, polya_early_stopping=0, polya_early_stop_window=50, polya_early_stop_stride=10):
    """_c_llr.pyx:176-199: the gains from given cumulative sums"""
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(1, -1)
    c2 = np.ascontiguousarray(c2, dtype=np.float64).reshape(1, -1)
    n = c.shape[1]
    if n == 0:
        return np.zeros(0)
    return c_llr_trace_batch(None, [n], [start], [end], min_obs, border_trim, stride, adapter_early_stopping, adapter_early_stop_window,
                             adapter_early_stop_stride, polya_early_stopping, polya_early_stop_window, polya_early_stop_stride,
                             sums=(c, c2))[0]


def _gains(start, end, c, c2, offset_head, offset_tail, stride=1):
    """_c_llr.pyx:67-88"""
    return c_llr_trace_gains(c, c2, start, end, offset_head, offset_tail, stride)


# -- the best-split segmenters (_c_llr.pyx:40-64, :239-433) ------------------------------------------------------------------

def _check_offsets(**kw):
    for k, v in kw.items():
        if v < 0:
            raise ValueError("%s must be >= 0 (got %d)" % (k, v))


def best_split_batch(c, c2, lens, starts, ends, offset_heads, offset_tails, device: int = 0):
    """`_best_split` for many rows in one call: sums float64 [n, L] (row r valid in [0, lens[r])), per-row start / end /
    offsets -> (x int64 [n], split_gain float64 [n]); x = -1 and gain 0.0 where no split point has a gain > 0"""
    lens = np.asarray(lens, dtype=np.int64)
    for s, e, n, oh, ot in zip(*(np.asarray(a).tolist() for a in (starts, ends, lens, offset_heads, offset_tails))):
        _check_range(s, e, n)
        _check_offsets(offset_head=oh, offset_tail=ot)
    return _engine(device).c_llr_best_split(c, c2, lens, starts, ends, offset_heads, offset_tails)


def _best_split(start, end, c, c2, offset_head, offset_tail):
    """_c_llr.pyx:40-64 -> (x, split_gain)"""
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(1, -1)
    c2 = np.ascontiguousarray(c2, dtype=np.float64).reshape(1, -1)
    n = c.shape[1]
    _check_range(start, end, n)
    _check_offsets(offset_head=offset_head, offset_tail=offset_tail)
    if n == 0:
        return -1, 0.0
    x, g = best_split_batch(c, c2, [n], [start], [end], [offset_head], [offset_tail])
    return int(x[0]), float(g[0])


def _gains_w_early_stop(start, end, c, c2, offset_head, offset_tail, stride=1, early_stop_window=500, early_stop_stride=100):
    """_c_llr.pyx:91-122"""
    return c_llr_trace_gains(c, c2, start, end, offset_head, offset_tail, stride, adapter_early_stopping=1,
                             adapter_early_stop_window=early_stop_window, adapter_early_stop_stride=early_stop_stride)


def _gains_w_polya_early_stop(start, end, c, c2, offset_head, offset_tail, stride=1, adapter_early_stop_window=1000,
                              adapter_early_stop_stride=500, polya_early_stop_window=50, polya_early_stop_stride=10):
    """_c_llr.pyx:126-173"""
    return c_llr_trace_gains(c, c2, start, end, offset_head, offset_tail, stride, adapter_early_stop_window=adapter_early_stop_window,
                             adapter_early_stop_stride=adapter_early_stop_stride, polya_early_stopping=1,
                             polya_early_stop_window=polya_early_stop_window, polya_early_stop_stride=polya_early_stop_stride)


def _detect_batch(raw_signals, lens, min_obs_adapter, border_trim, min_obs_polya, polya, details, device):
    x, lens = as_rows(np.asarray(raw_signals), lens, None, None, lambda dt: dt if dt == np.float32 else np.dtype(np.float64), "raw_signals",
                      1, "need one length per read, 1 <= lens <= L (an empty read: the reference indexes outside its arrays)")
    _check_offsets(min_obs_adapter=min_obs_adapter, border_trim=border_trim, min_obs_polya=min_obs_polya)
    if x.shape[0] == 0:
        z = np.zeros((0, 4), dtype=np.int64)
        return (z, z.copy(), np.zeros((0, 8))) if details else z
    return _engine(device).c_llr_detect(x, lens, min_obs_adapter, border_trim, min_obs_polya, polya=polya, details=details)


def c_llr_detect_adapter_batch(raw_signals, lens, min_obs_adapter, border_trim, details=False, device: int = 0):
    """`c_llr_detect_adapter` for many reads in one call: raw_signals float64 or float32 [n, L] (read r valid in [0, lens[r]),
    1 <= lens[r]; float32 rows give the results of ``x.astype(float64)``; what lies beyond lens[r] is never read) ->
    int64 [n, 4]: adapter_start, adapter_end, 0, 2 (the last column is the length of the reference's tuple).
    ``details``: also (splits int64 [n, 4]: x_first, x_head, x_tail, -1 -- the searches' results before the fallbacks;
    stats float64 [n, 8]: their gains, then the four segment medians)."""
    return _detect_batch(raw_signals, lens, min_obs_adapter, border_trim, 0, False, details, device)


def c_llr_detect_adapter_polya_batch(raw_signals, lens, min_obs_adapter, border_trim, min_obs_polya, details=False, device: int = 0):
    """`c_llr_detect_adapter_polya` for many reads: as `c_llr_detect_adapter_batch`, rows adapter_start, adapter_end, polya_end,
    k -- k = 3 for the reference's 3-tuple, k = 2 where it returns the 2-tuple (0, 0) (the first split found nothing,
    _c_llr.pyx:310-312; polya_end is 0 there).  splits[:, 3]: the poly(A) search's x (-1: none, or not searched)."""
    return _detect_batch(raw_signals, lens, min_obs_adapter, border_trim, min_obs_polya, True, details, device)


def _one_read(raw_signal):
    x = np.asarray(raw_signal)
    x = (x if x.dtype == np.float32 else np.asarray(x, dtype=np.float64)).reshape(1, -1)
    if x.shape[1] == 0:
        raise ValueError("empty signal: the reference indexes outside its arrays (_c_llr.pyx:247, len - 1 = -1)")
    return x


def c_llr_detect_adapter(raw_signal, min_obs_adapter, border_trim):
    """_c_llr.pyx:239-287 -> (adapter_start, adapter_end)"""
    x = _one_read(raw_signal)
    row = c_llr_detect_adapter_batch(x, [x.shape[1]], min_obs_adapter, border_trim)[0]
    return int(row[0]), int(row[1])


def c_llr_detect_adapter_polya(raw_signal, min_obs_adapter, border_trim, min_obs_polya):
    """_c_llr.pyx:290-365 -> (adapter_start, adapter_end, polya_end), or (0, 0) when the first split finds nothing"""
    x = _one_read(raw_signal)
    row = c_llr_detect_adapter_polya_batch(x, [x.shape[1]], min_obs_adapter, border_trim, min_obs_polya)[0]
    return tuple(int(v) for v in row[: int(row[3])])


def _traces(raw_signal, min_obs_adapter, border_trim):
    # the first level and the two below it; the next level starts at np.argmax of the previous gains (the first NaN, else the
    # first maximum: 0 when no gain is > 0) -- not _best_split's rule
    x = np.asarray(raw_signal, dtype=np.float64).reshape(-1)
    if x.size == 0:
        raise ValueError("empty signal: the reference indexes outside its arrays (_c_llr.pyx:373, len - 1 = -1)")
    _check_offsets(min_obs_adapter=min_obs_adapter, border_trim=border_trim)
    length = x.size - 1
    g_first, c, c2 = c_llr_trace(x, 0, length, min_obs_adapter + border_trim, border_trim, return_c_c2=1)
    x_first = int(np.argmax(g_first))
    g_head = _gains(0, x_first, c, c2, border_trim, min_obs_adapter)
    g_tail = _gains(x_first, length, c, c2, min_obs_adapter, border_trim)
    return g_first, g_head, g_tail, c, c2, length


def c_llr_detect_adapter_trace(raw_signal, min_obs_adapter, border_trim):
    """_c_llr.pyx:368-385 -> (gains_first, gains_head, gains_tail)"""
    return _traces(raw_signal, min_obs_adapter, border_trim)[:3]


def c_llr_boundary_traces(raw_signal, min_obs_adapter, border_trim):
    """_c_llr.pyx:415-433 -> (gains_first, gains_head, gains_tail)"""
    return _traces(raw_signal, min_obs_adapter, border_trim)[:3]


def c_llr_detect_adapter_polya_trace(raw_signal, min_obs_adapter, border_trim, min_obs_polya):
    """_c_llr.pyx:388-412 -> (gains_first, gains_head, gains_tail, gains_polya)"""
    _check_offsets(min_obs_polya=min_obs_polya)
    g_first, g_head, g_tail, c, c2, length = _traces(raw_signal, min_obs_adapter, border_trim)
    x_last = int(np.argmax(g_tail))
    return g_first, g_head, g_tail, _gains(x_last, length, c, c2, min_obs_polya, border_trim)
