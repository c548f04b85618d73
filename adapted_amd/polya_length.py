"""Poly(A) tail length in bases (an extension: the reference's README, "Poly(A) tail length estimation", describes the step and
leaves it to its users and to another tool's event segmentation).

The boundaries of a detect call are lengths in samples.  The adapter has a fixed length in bases, so its signal gives the
read's translocation speed in samples per base, either as ``(adapter_end - adapter_start) / adapter_nt`` or -- the more robust
form -- as the median length of the events an event segmentation finds in the adapter signal.  The poly(A) length in bases is
its length in samples divided by that speed.

``segment_events`` / ``segment_events_batch`` run the segmentation on the GPU (adp_segment_events,
include/adapted_hip_events.h: a squared two-window t-statistic, then ``scipy.signal.find_peaks(score, height, distance)``);
``estimate_polya_length`` is the division, plain float64 numpy on the host.

The defaults of ``EventParams`` are UNTUNED: they were chosen on synthetic staircases, not on real pod5 data.  This module is
not part of ``adapted_amd.detect``, which mirrors the reference's package name for name.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import lib
from .detect._rows import _engine, as_work, rows_in


@dataclass
class EventParams:
    """window: samples per side of the two-window t-statistic (2 .. 64); min_distance: the least distance between two
    boundaries; threshold: the least squared t-statistic of a boundary (16.0: |t| = 4); var_floor: the least pooled variance
    the statistic divides by.  Untuned defaults."""
    window: int = 8
    min_distance: int = 8
    threshold: float = 16.0
    var_floor: float = 1e-3

    def args(self) -> "lib.AdpEventArgs":
        a = lib.AdpEventArgs()
        a.window, a.min_distance = int(self.window), int(self.min_distance)
        a.threshold, a.var_floor = float(self.threshold), float(self.var_floor)
        return a

    @classmethod
    def parse(cls, text: str) -> "EventParams":
        """"WINDOW,MIN_DISTANCE,THRESHOLD" (the command line's --event_params)"""
        parts = [p.strip() for p in str(text).split(",")]
        if len(parts) != 3:
            raise ValueError("event parameters are WINDOW,MIN_DISTANCE,THRESHOLD")
        p = cls(window=int(parts[0]), min_distance=int(parts[1]), threshold=float(parts[2]))
        p.check()
        return p

    def check(self):
        """what the library refuses, said without a GPU"""
        if not 2 <= int(self.window) <= 64:
            raise ValueError("window must lie in [2, 64]")
        if int(self.min_distance) < 1:
            raise ValueError("min_distance must be >= 1")
        for name in ("threshold", "var_floor"):
            v = float(getattr(self, name))
            if not (np.isfinite(v) and v > 0):
                raise ValueError("%s must be finite and > 0" % name)


def _segs(segs):
    """(rows, starts, ends), or an array [n_seg, 3] of them -> three int64 arrays"""
    if isinstance(segs, np.ndarray) and segs.dtype == lib.SEG_DTYPE:
        return segs["row"].astype(np.int64), segs["start"].astype(np.int64), segs["end"].astype(np.int64)
    if not isinstance(segs, (tuple, list)) or len(segs) != 3 or np.ndim(segs[0]) == 0:
        a = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
        segs = (a[:, 0], a[:, 1], a[:, 2])
    rows, starts, ends = (np.asarray(v, dtype=np.int64).reshape(-1) for v in segs)
    if not rows.size == starts.size == ends.size:
        raise ValueError("segs: one row, start and end per segment")
    return rows, starts, ends


def segment_events_batch(signals, lens, segs, params: Optional[EventParams] = None, cap: Optional[int] = None, device=0,
                         n: Optional[int] = None, L: Optional[int] = None, dtype=np.float32, engine=None):
    """The event boundaries of ``signals[row, start:end]`` for many segments.  signals: a padded host array [n, L] (float32,
    float64; integers are widened to float64), or a device pointer (int) with ``n``, ``L`` and ``dtype``; lens: one length per
    read; segs: (rows, starts, ends) or an array [n_seg, 3].  A segment is clipped to its read as a Python slice is; a negative
    start or end <= start gives an empty one.
    -> (pos int64 [n_seg, cap]: positions from the clipped segment's start, ascending, then -1; count int64 [n_seg]: the
    number of boundaries, also past cap; status int64 [n_seg]: 0, 1 -- a NaN in the slice, 2 -- the slice is shorter than two
    windows; stats float64 [n_seg, 2]: the median and the median absolute deviation of the gaps between boundaries, NaN with
    fewer than two).  cap None: as wide as the longest list (the call is made twice)."""
    params = params or EventParams()
    params.check()
    rows, starts, ends = _segs(segs)
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    ns = rows.size
    if ns == 0 or nn == 0:
        if ns:
            raise ValueError("segments of no reads")
        return np.zeros((0, int(cap or 0)), dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 2))
    eng = engine or _engine(device)
    a = params.args()
    pos, info, stats = eng.segment_events(x, lens, rows, starts, ends, a, cap=0 if cap is None else int(cap), n=n, L=L, f64=f64)
    if cap is None and info[:, 0].max() > 0:
        pos, info, stats = eng.segment_events(x, lens, rows, starts, ends, a, cap=int(info[:, 0].max()), n=n, L=L, f64=f64)
    return pos, info[:, 0].copy(), info[:, 1].copy(), stats


def segment_events_packed(packed, offsets, params: Optional[EventParams] = None, cap: Optional[int] = None, scale=None, offset=None,
                          device=0, engine=None):
    """segment_events_batch of segments that lie back to back in one array (adp_segment_events_packed,
    include/adapted_hip_events_packed.h): segment g is ``packed[offsets[g]:offsets[g + 1]]`` -- float32 pA, or raw int16 ADC
    samples with ``scale`` / ``offset``, one calibration per segment (pA = scale * (float32(adc) + offset), rounded to float32
    twice).  packed: a host array, or a device pointer (int; int16 when ``scale`` and ``offset`` are given, device pointers
    too); offsets: int64 [n_seg + 1] on the host.  -> segment_events_batch's (pos, count, status, stats), the same bytes as that
    call gives for the same samples inside a padded matrix.  The int16 form's parity with pod5's own signal_pa is unpinned."""
    params = params or EventParams()
    params.check()
    if np.asarray(offsets).size < 2:
        return np.zeros((0, int(cap or 0)), dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 2))
    eng = engine or _engine(device)
    a = params.args()
    pos, info, stats = eng.segment_events_packed(packed, offsets, a, cap=0 if cap is None else int(cap), scale=scale, offset=offset)
    if cap is None and info[:, 0].max() > 0:
        pos, info, stats = eng.segment_events_packed(packed, offsets, a, cap=int(info[:, 0].max()), scale=scale, offset=offset)
    return pos, info[:, 0].copy(), info[:, 1].copy(), stats


def segment_events(signal, params: Optional[EventParams] = None, device=0) -> np.ndarray:
    """The event boundaries of one signal (int64, ascending); none for a signal with a NaN or shorter than two windows"""
    x = as_work(signal).reshape(1, -1)
    if x.shape[1] == 0:
        (params or EventParams()).check()
        return np.zeros(0, dtype=np.int64)
    pos, count, _, _ = segment_events_batch(x, [x.shape[1]], ([0], [0], [x.shape[1]]), params, device=device)
    return pos[0, : int(count[0])].copy()


def _column(v, n=None):
    """a column of positions or lengths with None / NaN for a missing value -> float64 array"""
    a = np.asarray([np.nan if q is None else q for q in np.atleast_1d(np.asarray(v, dtype=object)).ravel()], dtype=np.float64)
    if n is not None and a.size == 1 and n != 1:
        a = np.full(n, a[0])
    return a


def estimate_polya_length(adapter_start, adapter_end, polya_end, *, method, event_len_med=None, adapter_nt=None):
    """-> (polya_nt, samples_per_nt), float64 arrays with one entry per read.
    method "events": samples_per_nt = event_len_med (the median event length of the adapter, segment_events_batch's stats[:, 0]);
    method "adapter": samples_per_nt = (adapter_end - adapter_start) / adapter_nt (the adapter's length in bases).
    polya_nt = (polya_end - adapter_end) / samples_per_nt.  NaN where an input is missing (None or NaN) or samples_per_nt is
    not > 0.  A poly(A) cut off by the preload window (polya_truncated) gives a lower bound."""
    if method not in ("events", "adapter"):
        raise ValueError('method must be "events" or "adapter"')
    a_s, a_e, p_e = _column(adapter_start), _column(adapter_end), _column(polya_end)
    if not a_s.size == a_e.size == p_e.size:
        raise ValueError("one adapter_start, adapter_end and polya_end per read")
    if method == "events":
        if event_len_med is None:
            raise ValueError('method "events" needs event_len_med')
        spn = _column(event_len_med, a_e.size)
    else:
        if adapter_nt is None:
            raise ValueError('method "adapter" needs adapter_nt')
        with np.errstate(divide="ignore", invalid="ignore"):
            spn = (a_e - a_s) / _column(adapter_nt, a_e.size)
    if spn.size != a_e.size:
        raise ValueError("one speed per read")
    spn = np.where((spn > 0) & np.isfinite(spn), spn, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        polya_nt = (p_e - a_e) / spn
    return polya_nt, spn


__all__ = ["EventParams", "segment_events", "segment_events_batch", "segment_events_packed", "estimate_polya_length"]
