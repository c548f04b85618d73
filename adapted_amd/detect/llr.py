"""The reference's LLR trace module ``adapted.detect.llr`` (adapted/detect/llr.py) on the HIP library: every name it defines, with
the same arguments and return types, so that ``from adapted.detect.llr import ...`` can become
``from adapted_amd.detect.llr import ...``.  Next to the drop-ins sit their batch forms (``*_batch``): padded float64 [n, L] traces
with per-read lengths, or a device pointer (int) with ``n`` and ``L``, so that resident traces never cross PCIe.

Every per-read function is one batch call with n = 1 on the engine `_rows._engine` caches; the traces come from `_c_llr`, the
derived state of `LLRTrace` from ``adp_llr_trace_bounds``, the peaks from ``adp_llr_trace_peaks`` and the poly(A) end from
``adp_llr_spike_peak`` (adapted_amd/csrc/trace_peaks_api.h).  There is no CPU path: without the HIP library every function raises
``HipLibraryError``.  Only numpy is needed (no scipy, no attrs).

Differences from the reference: the traces' values agree to ~1e-15 relative (the device logarithm is correctly rounded,
glibc's is not: DESIGN.md section 4), so a peak can move only where two trace values tie to that precision; linregress's r is
summed in another order (the r**2 test can flip only within ~1e-15 of its threshold); equal heights under the minimum distance
are resolved in favour of the later index (scipy's unstable argsort leaves that case undefined); `correct_for_plateau` takes
s >= 1 and a peak inside the trace (the reference indexes from the end otherwise).
"""
from __future__ import annotations

import logging
from typing import Optional, Tuple

import numpy as np

from .. import lib
from . import _c_llr
from ._c_llr import _gains, c_llr_trace, c_llr_trace_gains
from ._rows import _engine, as_rows

##############################
# LLR-based adapter detection
##############################


class LLRBoundariesLog:
    too_little_signal: bool = False
    no_adapter_end_found: bool = False
    min_obs_adapter_first_candidate: bool = False
    min_obs_adapter_only_candidate: bool = False
    recalc_adapter_trace_with_start_offset: bool = False
    recalc_adapter_trace_with_start_offset_too_short: bool = False
    second_try_no_adapter_end_found: bool = False
    second_try_min_obs_adapter_first_candidate: bool = False
    second_try_min_obs_adapter_only_candidate: bool = False
    truncated_polya: bool = False
    adapter_end_too_close_to_trace_end: bool = False
    no_polya_end_found: bool = False
    refine_too_few_extrema: bool = False
    refine_adapter_end_adjusted_within_atol: bool = False
    refine_polya_not_poi: bool = False
    refine_region_too_short: bool = False
    refine_possible_noisy_polya: bool = False
    refine_adapter_end_adjusted: bool = False

    def to_string(self):
        return " ".join([f"{k}" for k, v in self.__dict__.items() if v])


_EMPTY_KNOTS = "array of sample points is empty"  # (numpy's np.interp message)


class LLRTrace:
    """llr.py:53-142 (an attrs class there; keyword-only fields): the trace, its bounds, the early-stop flag and the stride
    interpolation, derived on the device (adp_llr_trace_bounds)"""

    __slots__ = ("signal", "c", "c2", "trace_start", "trace_end", "stride", "min_obs", "tail_trim", "start", "end", "early_stop",
                 "stride_interp", "start_interp", "end_interp")

    def __init__(self, *, signal: np.ndarray, c: Optional[np.ndarray] = None, c2: Optional[np.ndarray] = None, trace_start: int = 0,
                 trace_end: Optional[int] = None, stride: int, min_obs: int, tail_trim: int):
        self.signal, self.c, self.c2 = signal, c, c2
        self.trace_start, self.trace_end = trace_start, trace_end
        self.stride, self.min_obs, self.tail_trim = stride, min_obs, tail_trim
        self.start = self.end = None
        self.early_stop = self.stride_interp = self.start_interp = self.end_interp = None
        self.__attrs_post_init__()

    def __repr__(self):
        return "LLRTrace(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)

    @property
    def max_len_no_early_stop(self):
        r = np.arange(self.min_obs, self.signal.size - 1 - self.tail_trim, self.stride)
        if r.size:
            return r[-1]
        logging.error("ERROR %s %s %s %s", self.min_obs, self.signal.size, self.tail_trim, self.stride)
        return self.signal.size - 1 - self.tail_trim

    @property
    def zero_tail_length(self):
        return self.signal.size - self.end

    def __attrs_post_init__(self):
        if self.signal is None:
            msg = "signal is None"
            logging.error(msg)
            raise ValueError(msg)
        sig = np.asarray(self.signal)
        if sig.size == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        interp = self.stride > 1
        row = np.array(sig, dtype=np.float64).reshape(1, -1)  # (a copy: the stride interpolation works in place)
        st, en, es = _engine().llr_trace_bounds(row, [row.shape[1]], [self.min_obs], [self.tail_trim], max(int(self.stride), 1), interp)
        if es[0] & 2:
            raise ValueError(_EMPTY_KNOTS)
        self.start, self.end = int(st[0]), int(en[0])
        self.early_stop = bool(es[0] & 1)
        if interp:
            self.signal = row[0]
            self.stride_interp = True

    def interp_start(self):
        y_val = self.signal[self.start]
        self.signal[np.arange(self.start)] = np.interp(np.arange(self.start), [0, self.start], [0, y_val], left=0)
        self.start_interp = True

    def interp_end(self):
        y_val = self.signal[self.end]
        self.signal[-1 * np.arange(self.zero_tail_length)] = np.interp(np.arange(self.zero_tail_length), [self.zero_tail_length, 0],
                                                                       [y_val, 0], left=0)
        self.end_interp = True

    def interp_stride(self):
        row = np.array(self.signal, dtype=np.float64).reshape(1, -1)
        _, _, es = _engine().llr_trace_bounds(row, [row.shape[1]], [self.min_obs], [self.tail_trim], max(int(self.stride), 2), True)
        if es[0] & 2:
            raise ValueError(_EMPTY_KNOTS)
        self.signal = row[0]
        self.stride_interp = True

    def _trace_start_end(self) -> Tuple[int, int]:
        sig = np.array(self.signal, dtype=np.float64).reshape(1, -1)
        if sig.size == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        st, en, _ = _engine().llr_trace_bounds(sig, [sig.shape[1]], [0], [0], 1, False)
        return int(st[0]), int(en[0])


# -- peaks -------------------------------------------------------------------------------------------------------------------

_PLATEAU = (10, 0.9, 500)        # correct_for_plateau's defaults (s, t, window)
_SPLIT = (10, 0.9, 500, 1.0)     # correct_for_split_peak's (s, t, window, prominence)


def _peak_args(prominence=1.0, width=0.0, rel_height=0.5, fix_plateau=False, plateau=_PLATEAU, split_peaks=False, split=_SPLIT):
    ps, pt, pw = plateau
    ss, st, sw, sp = split
    if fix_plateau and int(ps) < 1:
        raise ValueError("correct_for_plateau needs s >= 1 (got %r)" % (ps,))
    return lib.AdpPeakArgs(prominence=float(prominence), width=float(width), rel_height=float(rel_height), plateau_t=float(pt),
                           split_t=float(st), split_prominence=float(sp), plateau_on=int(bool(fix_plateau)), plateau_s=int(ps),
                           plateau_window=int(pw), split_on=int(bool(split_peaks)), split_s=int(ss), split_window=int(sw))


def _as_rows(traces, lens, n, L):
    """host traces -> (float64 C-contiguous [n, L] array, lens int64 [n]); a device pointer passes through"""
    return as_rows(traces, lens, n, L, lambda dt: np.dtype(np.float64), "traces")


def _peaks_batch(x, lens, lo, hi, args, cap, n, L, device, given=False):
    """adp_llr_trace_peaks, then the reads whose count exceeded cap again, one by one with a cap that fits"""
    eng = _engine(device)
    if isinstance(x, int):
        n, L = int(n), int(L)
    else:
        n, L = x.shape
    if n == 0:
        return np.full((0, cap), -1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    pk, cnt = eng.llr_trace_peaks(x, lens, lo, hi, args, cap=cap, n=n, L=L, given_peak=given)
    over = np.nonzero(cnt > cap)[0]
    if over.size:
        wide = np.full((n, int(cnt.max())), -1, dtype=np.int64)
        wide[:, :cap] = pk
        for r in over.tolist():
            row = (x + r * L * 8) if isinstance(x, int) else x[r:r + 1]
            k = int(cnt[r])
            p2, c2 = eng.llr_trace_peaks(row, lens[r:r + 1], lo[r:r + 1], hi[r:r + 1], args, cap=k, n=1, L=L)
            assert int(c2[0]) == k
            wide[r, :k] = p2[0]
        pk = wide
    return pk, cnt


def _clip_of(trace: LLRTrace) -> Tuple[int, int]:
    # trace.signal[trace.start if not trace.start_interp else 0 : (trace.end if not trace.end_interp else -1)] (llr.py:210-215)
    size = np.asarray(trace.signal).size
    a, b, _ = slice(trace.start if not trace.start_interp else 0, trace.end if not trace.end_interp else -1).indices(size)
    return a, max(a, b)


def _one_row(sig):
    return np.ascontiguousarray(sig, dtype=np.float64).reshape(1, -1)


def correct_for_plateau(trace_sig: np.ndarray, peak: int, s: int = 10, t: float = 0.9, window: int = 500, verbose: bool = False):
    """llr.py:145-177: the end of the last increase or plateau of length s within `window` after `peak` whose end is above
    t * trace[peak]; `peak` when there is none"""
    x = _one_row(trace_sig)
    if not 0 <= int(peak) < x.shape[1]:
        raise ValueError("peak must lie inside the trace (got %d, size %d)" % (int(peak), x.shape[1]))
    args = _peak_args(fix_plateau=True, plateau=(s, t, window))
    pk, _ = _peaks_batch(x, [x.shape[1]], np.array([int(peak)]), np.array([int(peak)]), args, 1, None, None, 0, given=True)
    new = int(pk[0, 0])
    if new == int(peak):
        return peak
    if verbose:
        logging.info(f"plateau end found! {new}")
    return peak + (new - int(peak))


def correct_for_split_peak(trace_sig: np.ndarray, peak: int, s: int = 10, t: float = 0.9, window: int = 500, prominence: float = 1.0,
                           verbose: bool = False):
    """llr.py:180-201: the first peak of find_peaks(trace[peak:peak + window], width=s, prominence) when it reaches t * trace[peak]"""
    x = _one_row(trace_sig)
    if not 0 <= int(peak) < x.shape[1]:
        raise ValueError("peak must lie inside the trace (got %d, size %d)" % (int(peak), x.shape[1]))
    args = _peak_args(split_peaks=True, split=(s, t, window, prominence))
    pk, _ = _peaks_batch(x, [x.shape[1]], np.array([int(peak)]), np.array([int(peak)]), args, 1, None, None, 0, given=True)
    new = int(pk[0, 0])
    if new == int(peak):
        return peak
    if verbose:
        logging.info(f"split peak accepted! {new - int(peak)}")
    return np.int64(new)


def find_peaks_in_trace(trace: LLRTrace, width: int = 100, prominence: float = 1.0, rel_height=0.5) -> np.ndarray:
    """llr.py:204-224: find_peaks(clip, width, prominence=prominence * np.nanstd(clip), rel_height), in full-trace indices"""
    x = _one_row(trace.signal)
    a, b = _clip_of(trace)
    pk, cnt = _peaks_batch(x, [x.shape[1]], np.array([a]), np.array([b]), _peak_args(prominence, width, rel_height), 16, None, None, 0)
    return pk[0, :int(cnt[0])].copy()


def adapter_end_from_trace(trace: LLRTrace, prominence: float = 1.0, rel_height: float = 1.0, width: int = 2000, fix_plateau: bool = True,
                           correct_for_split_peaks: bool = True) -> np.ndarray:
    """llr.py:227-263: every peak of find_peaks_in_trace, each plateau- and split-corrected as the flags ask (an empty result
    with either flag set is np.array([]), float64, as in the reference)"""
    x = _one_row(trace.signal)
    a, b = _clip_of(trace)
    args = _peak_args(prominence, width, rel_height, fix_plateau, _PLATEAU, correct_for_split_peaks, _SPLIT)
    pk, cnt = _peaks_batch(x, [x.shape[1]], np.array([a]), np.array([b]), args, 16, None, None, 0)
    peaks = pk[0, :int(cnt[0])].copy()
    if (fix_plateau or correct_for_split_peaks) and peaks.size == 0:
        return np.array([])
    return peaks


# -- traces ------------------------------------------------------------------------------------------------------------------

def calc_adapter_trace(signal: np.ndarray, offset_head: int, offset_tail: int, stride: int, early_stop1_window: int, early_stop1_stride: int,
                       early_stop2_window: int, early_stop2_stride: int, return_c_c2: bool, trace_start: int = 0,
                       trace_end: Optional[int] = None, adapter_early_stopping: int = 0, polya_early_stopping: int = 1,
                       c: Optional[np.ndarray] = None, c2: Optional[np.ndarray] = None) -> LLRTrace:
    """llr.py:266-354"""
    if (c is not None) != (c2 is not None):
        msg = "c and c2 need to be both provided or not provided"
        logging.error(msg)
        raise ValueError(msg)
    if trace_end is None:
        trace_end = int(signal.size - 1)
    if c is not None and c2 is not None:
        if c.size != c2.size:
            msg = "c and c2 need to have the same size"
            logging.error(msg)
            raise ValueError(msg)
        if c.size != signal.size:
            msg = "c and c2 need to have the same size as signal"
            logging.error(msg)
            raise ValueError(msg)
        llr_trace = c_llr_trace_gains(c=c.astype(np.float64), c2=c2.astype(np.float64), start=trace_start, end=trace_end,
                                      min_obs=offset_head, border_trim=offset_tail, stride=stride,
                                      adapter_early_stopping=adapter_early_stopping, adapter_early_stop_window=early_stop1_window,
                                      adapter_early_stop_stride=early_stop1_stride, polya_early_stopping=polya_early_stopping,
                                      polya_early_stop_window=early_stop2_window, polya_early_stop_stride=early_stop2_stride)
        if not return_c_c2:
            c, c2 = None, None
    else:
        res = c_llr_trace(signal.astype(np.float64), trace_start, trace_end, offset_head, offset_tail, stride, adapter_early_stopping,
                          early_stop1_window, early_stop1_stride, polya_early_stopping, early_stop2_window, early_stop2_stride,
                          int(return_c_c2))
        if return_c_c2:
            llr_trace, c, c2 = res
        else:
            llr_trace = res
            c, c2 = None, None
    return LLRTrace(signal=llr_trace, c=c, c2=c2, trace_start=trace_start, trace_end=trace_end, stride=stride, min_obs=offset_head,
                    tail_trim=offset_tail)


def calc_polya_trace(c: np.ndarray, c2: np.ndarray, adapter_end: int, trace_early_stop_end: int, min_obs_polya: int,
                     stride: int = 1) -> LLRTrace:
    """llr.py:357-382 (the two tail expressions as there: c.size - trace_early_stop_end to _gains, c.size - 1 - ... to LLRTrace)"""
    trace_sig = _gains(adapter_end, c.size - 1, c.astype(np.float64), c2.astype(np.float64), min_obs_polya, c.size - trace_early_stop_end,
                       stride)
    return LLRTrace(signal=trace_sig, c=c, c2=c2, stride=stride, min_obs=min_obs_polya + adapter_end,
                    tail_trim=c.size - 1 - trace_early_stop_end)


def calc_full_polya_trace(signal, adapter_end):
    """llr.py:385-403"""
    llr_trace, c, c2 = c_llr_trace(signal.astype(np.float64), adapter_end, signal.size - 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1)
    return LLRTrace(signal=llr_trace, c=c, c2=c2, trace_start=adapter_end, stride=1, min_obs=1, tail_trim=1)


def _spike_args(min_peak_distance, prominence_threshold, min_width, threshold_prominence_ratio, threshold_r_squared):
    if not min_peak_distance >= 1:
        raise ValueError("`distance` must be greater or equal to 1")
    return lib.AdpSpikeArgs(float(min_peak_distance), float(prominence_threshold), float(min_width), float(threshold_prominence_ratio),
                            float(threshold_r_squared))


def detect_full_polya_trace_peak_with_spike(llr_trace: np.ndarray, min_peak_distance: int = 10, prominence_threshold: float = 1.0,
                                            min_width: int = 10, threshold_prominence_ratio: float = 0.5, threshold_r_squared: float = 0.99):
    """llr.py:406-479: the poly(A) end in the full poly(A) trace, a spike allowed for; 0 when no peak is found"""
    x = _one_row(llr_trace)
    args = _spike_args(min_peak_distance, prominence_threshold, min_width, threshold_prominence_ratio, threshold_r_squared)
    if x.shape[1] == 0:
        return 0
    r = int(_engine().llr_spike_peak(x, [x.shape[1]], args)[0])
    return np.int64(r) if r else 0


# -- batch forms ---------------------------------------------------------------------------------------------------------------

def calc_adapter_trace_batch(signals, lens, offset_head: int, offset_tail: int, stride: int, early_stop1_window: int,
                             early_stop1_stride: int, early_stop2_window: int, early_stop2_stride: int, return_c_c2: bool = False,
                             trace_starts=None, trace_ends=None, adapter_early_stopping: int = 0, polya_early_stopping: int = 1,
                             device: int = 0):
    """`calc_adapter_trace` for many reads: signals float64 [n, L] (read r valid in [0, lens[r]), 1 <= lens[r]) ->
    (signal float64 [n, L] -- interpolated when stride > 1 --, start int64 [n], end int64 [n], early_stop bool [n]) and with
    ``return_c_c2`` also (c, c2).  No per-read host work: the traces (adp_c_llr_trace) and their bounds, early-stop flags and
    interpolation (adp_llr_trace_bounds) stay on the device between the two calls' kernels."""
    x = np.ascontiguousarray(signals, dtype=np.float64)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    n = x.shape[0]
    if lens.size != n or (n and (lens.min() < 1 or lens.max() > x.shape[1])):
        raise ValueError("need one length per read, 1 <= lens <= L")
    starts = np.zeros(n, dtype=np.int64) if trace_starts is None else np.asarray(trace_starts, dtype=np.int64).reshape(-1)
    ends = lens - 1 if trace_ends is None else np.asarray(trace_ends, dtype=np.int64).reshape(-1)
    res = _c_llr.c_llr_trace_batch(x, lens, starts, ends, offset_head, offset_tail, stride, adapter_early_stopping, early_stop1_window,
                                   early_stop1_stride, polya_early_stopping, early_stop2_window, early_stop2_stride, int(return_c_c2),
                                   device=device)
    g = res[0] if return_c_c2 else res
    st, en, es = _engine(device).llr_trace_bounds(g, lens, np.full(n, offset_head), np.full(n, offset_tail), max(int(stride), 1),
                                                  stride > 1)
    bad = np.nonzero(es & 2)[0]
    if bad.size:
        raise ValueError("%s (reads %s)" % (_EMPTY_KNOTS, bad[:8].tolist()))
    out = (g, st.astype(np.int64), en.astype(np.int64), (es & 1).astype(bool))
    return out + (res[1], res[2]) if return_c_c2 else out


def find_peaks_in_trace_batch(traces, lens, starts, ends, width: int = 100, prominence: float = 1.0, rel_height: float = 0.5,
                              cap: int = 16, n: Optional[int] = None, L: Optional[int] = None, device: int = 0):
    """`find_peaks_in_trace` for many reads: traces float64 [n, L] or a device pointer with n, L; the clip of read r is
    [starts[r], ends[r]) -> (peaks int64 [n, >= cap] padded with -1, counts int64 [n]); reads with more than cap peaks are run again
    with a cap that fits, so nothing is cut off"""
    return adapter_end_from_trace_batch(traces, lens, starts, ends, prominence, rel_height, width, False, False, cap=cap, n=n, L=L,
                                        device=device)


def adapter_end_from_trace_batch(traces, lens, starts, ends, prominence: float = 1.0, rel_height: float = 1.0, width: int = 2000,
                                 fix_plateau: bool = True, correct_for_split_peaks: bool = True, plateau=_PLATEAU, split=_SPLIT,
                                 cap: int = 16, n: Optional[int] = None, L: Optional[int] = None, device: int = 0):
    """`adapter_end_from_trace` for many reads (clips [starts[r], ends[r])) -> (peaks int64 [n, >= cap] padded with -1, counts
    int64 [n]).  plateau = (s, t, window), split = (s, t, window, prominence): the corrections' parameters"""
    x, lens = _as_rows(traces, lens, n, L)
    nn = int(n) if isinstance(x, int) else x.shape[0]
    lo = np.asarray(starts, dtype=np.int64).reshape(-1)
    hi = np.asarray(ends, dtype=np.int64).reshape(-1)
    if lo.size != nn or hi.size != nn:
        raise ValueError("starts / ends need one entry per read")
    hi = np.maximum(hi, lo)  # (an empty clip, as the reference's slice)
    args = _peak_args(prominence, width, rel_height, fix_plateau, plateau, correct_for_split_peaks, split)
    return _peaks_batch(x, lens, lo, hi, args, int(cap), n, L, device)


def detect_full_polya_trace_peak_with_spike_batch(traces, lens, min_peak_distance: int = 10, prominence_threshold: float = 1.0,
                                                  min_width: int = 10, threshold_prominence_ratio: float = 0.5,
                                                  threshold_r_squared: float = 0.99, n: Optional[int] = None, L: Optional[int] = None,
                                                  device: int = 0):
    """`detect_full_polya_trace_peak_with_spike` for many reads (read r: traces[r, :lens[r]]) -> int64 [n] (0: no peak)"""
    x, lens = _as_rows(traces, lens, n, L)
    args = _spike_args(min_peak_distance, prominence_threshold, min_width, threshold_prominence_ratio, threshold_r_squared)
    nn = int(n) if isinstance(x, int) else x.shape[0]
    if nn == 0:
        return np.zeros(0, dtype=np.int64)
    return _engine(device).llr_spike_peak(x, lens, args, n=n, L=L)


__all__ = ["LLRBoundariesLog", "LLRTrace", "correct_for_plateau", "correct_for_split_peak", "find_peaks_in_trace", "adapter_end_from_trace",
           "calc_adapter_trace", "calc_polya_trace", "calc_full_polya_trace", "detect_full_polya_trace_peak_with_spike",
           "calc_adapter_trace_batch", "find_peaks_in_trace_batch", "adapter_end_from_trace_batch",
           "detect_full_polya_trace_peak_with_spike_batch"]
