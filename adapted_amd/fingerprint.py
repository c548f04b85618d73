"""Adapter event fingerprints and barcode assignment by dynamic time warping (an extension: the reference's README sends its
users to a sister tool that segments the adapter signal into events and compares the events' levels by DTW to tell barcoded
adapters apart; ``adapted detect`` is that tool's first step).

``event_levels`` / ``event_levels_batch`` run the event segmentation of adapted_amd/polya_length.py on the GPU and return, per
segment, the event table (lengths and mean levels of at most ``max_events`` events -- with more, the boundaries of the highest
scores stay) and its fingerprint: the levels minus their median, over their median absolute deviation (adp_event_levels,
include/adapted_hip_fingerprint.h).  ``dtw_distances`` / ``assign_barcodes`` compare fingerprints with a small set of templates
(adp_dtw_assign: squared differences, the three classic steps, an optional Sakoe-Chiba band) and name the nearest.
``medoid_templates`` makes templates from labelled fingerprints; ``save_templates`` / ``load_templates`` keep them in an .npz.

The parameters are UNTUNED and no real pod5 data has been through any of this: whether such fingerprints separate real
barcodes is NOT claimed.  This module is not part of ``adapted_amd.detect``, which mirrors the reference's package name for name.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import lib
from .detect._rows import _engine, as_work, rows_in
from .polya_length import EventParams, _segs


@dataclass
class FingerprintParams:
    """max_events: the width of a fingerprint (2 .. 512); events: the segmentation's parameters; band: the DTW's band (0: none).
    Untuned defaults."""
    max_events: int = 110
    events: EventParams = field(default_factory=EventParams)
    band: int = 0

    def check(self):
        """what the library refuses, said without a GPU"""
        if not 2 <= int(self.max_events) <= lib.FINGERPRINT_MAX_EVENTS:
            raise ValueError("max_events must lie in [2, %d]" % lib.FINGERPRINT_MAX_EVENTS)
        if int(self.band) < 0:
            raise ValueError("band must be >= 0")
        self.events.check()


@dataclass
class EventLevels:
    """event_levels_batch's answer, one entry (row) per segment: count int32 (events), status int32 (0; 1 a NaN in the slice; 2 the
    slice is shorter than two windows; 4 the MAD of the levels is 0, or median / MAD are not finite -- then the fingerprint is
    NaN), lengths int32 / levels / fingerprints float64 [n_seg, max_events] (0 / NaN at and beyond count), norm float64
    [n_seg, 2] (median and MAD of the levels), event_len_med / event_len_mad float64 (segment_events_batch's stats)"""
    count: np.ndarray
    status: np.ndarray
    lengths: np.ndarray
    levels: np.ndarray
    fingerprints: np.ndarray
    norm: np.ndarray
    event_len_med: np.ndarray
    event_len_mad: np.ndarray


def event_levels_batch(signals, lens, segs, params: Optional[FingerprintParams] = None, device=0, n: Optional[int] = None,
                       L: Optional[int] = None, dtype=np.float32, engine=None) -> EventLevels:
    """The event tables and fingerprints of ``signals[row, start:end]`` for many segments; signals, lens and segs as
    polya_length.segment_events_batch takes them (a padded host array, or a device pointer with ``n``, ``L`` and ``dtype``)."""
    params = params or FingerprintParams()
    params.check()
    rows, starts, ends = _segs(segs)
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    E, ns = int(params.max_events), rows.size
    if ns == 0 or nn == 0:
        if ns:
            raise ValueError("segments of no reads")
        return EventLevels(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, E), dtype=np.int32), np.zeros((0, E)),
                           np.zeros((0, E)), np.zeros((0, 2)), np.zeros(0), np.zeros(0))
    eng = engine or _engine(device)
    r = eng.event_levels(x, lens, rows, starts, ends, params.events.args(), E, n=n, L=L, f64=f64)
    return EventLevels(r["count"], r["status"], r["lengths"], r["levels"], r["fingerprints"], r["norm"], r["stats"][:, 0].copy(),
                       r["stats"][:, 1].copy())


def event_levels_packed(packed, offsets, params: Optional[FingerprintParams] = None, scale=None, offset=None, device=0,
                        engine=None) -> EventLevels:
    """event_levels_batch of segments that lie back to back in one array (adp_event_levels_packed,
    include/adapted_hip_events_packed.h); packed, offsets, scale and offset as polya_length.segment_events_packed takes them.
    The same bytes as event_levels_batch gives for the same samples inside a padded matrix."""
    params = params or FingerprintParams()
    params.check()
    E = int(params.max_events)
    if np.asarray(offsets).size < 2:
        return EventLevels(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, E), dtype=np.int32), np.zeros((0, E)),
                           np.zeros((0, E)), np.zeros((0, 2)), np.zeros(0), np.zeros(0))
    eng = engine or _engine(device)
    r = eng.event_levels_packed(packed, offsets, params.events.args(), E, scale=scale, offset=offset)
    return EventLevels(r["count"], r["status"], r["lengths"], r["levels"], r["fingerprints"], r["norm"], r["stats"][:, 0].copy(),
                       r["stats"][:, 1].copy())


def event_levels(signal, params: Optional[FingerprintParams] = None, device=0) -> EventLevels:
    """The event table and fingerprint of one signal (arrays without the leading axis; count and status are numbers)"""
    params = params or FingerprintParams()
    x = as_work(signal).reshape(1, -1)
    if x.shape[1] == 0:
        x = np.zeros((1, 1), dtype=x.dtype)
        r = event_levels_batch(x, [0], ([0], [0], [0]), params, device=device)
    else:
        r = event_levels_batch(x, [x.shape[1]], ([0], [0], [x.shape[1]]), params, device=device)
    return EventLevels(int(r.count[0]), int(r.status[0]), r.lengths[0], r.levels[0], r.fingerprints[0], r.norm[0],
                       float(r.event_len_med[0]), float(r.event_len_mad[0]))


def _sequences(v, counts, what):
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.ndim != 2 or not 1 <= v.shape[1] <= lib.FINGERPRINT_MAX_EVENTS:
        raise ValueError("%s: a float64 [n, E] array, 1 <= E <= %d" % (what, lib.FINGERPRINT_MAX_EVENTS))
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if counts.size != v.shape[0]:
        raise ValueError("%s: one count per row" % what)
    return v, counts


def _templates(t, t_count):
    t, t_count = _sequences(t, t_count, "templates")
    if not 1 <= t.shape[0] <= lib.DTW_MAX_TEMPLATES:
        raise ValueError("1 to %d templates" % lib.DTW_MAX_TEMPLATES)
    if t_count.min() < 1 or t_count.max() > t.shape[1]:
        raise ValueError("every template needs 1 <= count <= its width")
    if not all(np.isfinite(t[k, :t_count[k]]).all() for k in range(t.shape[0])):
        raise ValueError("template values inside their count must be finite")
    return t, t_count


def dtw_distances(q, q_count, t, t_count, band: int = 0, device=0, engine=None) -> np.ndarray:
    """The DTW distance of every query (q float64 [nq, Eq], its first q_count[p] entries) to every template (t [nt, Et], t_count)
    -> float64 [nq, nt]; a NaN row for a query whose count lies outside [1, Eq] or that holds a value that is not finite"""
    if int(band) < 0:
        raise ValueError("band must be >= 0")
    q, q_count = _sequences(q, q_count, "queries")
    t, t_count = _templates(t, t_count)
    if q.shape[0] == 0:
        return np.zeros((0, t.shape[0]))
    return (engine or _engine(device)).dtw_assign(q, q_count, t, t_count, band)[0]


@dataclass
class Templates:
    """names: one per template; levels float64 [nt, Et], NaN beyond counts int32 [nt]"""
    names: list
    levels: np.ndarray
    counts: np.ndarray


@dataclass
class BarcodeAssignment:
    """best / second int32 [nq]: the nearest and the second nearest template (-1: none); dist / dist_second float64 [nq] (NaN
    where -1); margin = dist_second - dist"""
    best: np.ndarray
    second: np.ndarray
    dist: np.ndarray
    dist_second: np.ndarray
    margin: np.ndarray


def assignment_of(best, bestdist) -> BarcodeAssignment:
    """Engine.dtw_assign's best [nq, 2] and bestdist [nq, 2] as a BarcodeAssignment"""
    with np.errstate(invalid="ignore"):
        return BarcodeAssignment(best[:, 0].copy(), best[:, 1].copy(), bestdist[:, 0].copy(), bestdist[:, 1].copy(),
                                 bestdist[:, 1] - bestdist[:, 0])


def assign_barcodes(q, q_count, templates: Templates, band: int = 0, device=0, engine=None) -> BarcodeAssignment:
    """The nearest template of every fingerprint (the lowest index on equal distances) and the second nearest"""
    if int(band) < 0:
        raise ValueError("band must be >= 0")
    q, q_count = _sequences(q, q_count, "queries")
    t, t_count = template_arrays(templates)
    if q.shape[0] == 0:
        return assignment_of(np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2)))
    _, best, bestdist = (engine or _engine(device)).dtw_assign(q, q_count, t, t_count, band, want_dist=False)
    return assignment_of(best, bestdist)


def _nan_only_beyond(templates: Templates) -> bool:
    """(the NaN padding of a template file is fine; a NaN inside a count is refused by _templates)"""
    lv, c = np.asarray(templates.levels), np.asarray(templates.counts).reshape(-1)
    return lv.ndim == 2 and c.size == lv.shape[0] and all(0 <= c[k] <= lv.shape[1] and np.isfinite(lv[k, :c[k]]).all() for k in range(c.size))


def medoid_templates(fingerprints, counts, labels, band: int = 0, device=0, engine=None, distances=None) -> Templates:
    """Templates from labelled fingerprints: per label (in sorted order) the member with the least sum of DTW distances to the
    other members of its label, added in index order; the lowest index on equal sums.  The distances come from dtw_distances on
    the GPU, one call per label (``distances``: another function of the same arguments -- tests).  Members whose fingerprint is
    not usable (a count outside [1, E], a value that is not finite) are left out; a label without a usable member is an error."""
    fp, counts = _sequences(fingerprints, counts, "fingerprints")
    labels = np.asarray(labels).reshape(-1)
    if labels.size != fp.shape[0]:
        raise ValueError("one label per fingerprint")
    distances = distances or (lambda q, qc, t, tc, band: dtw_distances(q, qc, t, tc, band, device=device, engine=engine))
    usable = np.asarray([1 <= counts[p] <= fp.shape[1] and bool(np.isfinite(fp[p, :counts[p]]).all()) for p in range(fp.shape[0])], dtype=bool)
    names, rows = [], []
    for lab in sorted(set(labels.tolist())):
        idx = np.flatnonzero((labels == lab) & usable)
        if idx.size == 0:
            raise ValueError("label %r has no usable fingerprint" % (lab,))
        sub = np.where(np.isfinite(fp[idx]), fp[idx], 0.0)  # (beyond the counts: not read)
        d = np.asarray(distances(sub, counts[idx], sub, counts[idx], band))
        sums = [sum(float(d[i, j]) for j in range(idx.size) if j != i) for i in range(idx.size)]
        names.append(str(lab))
        rows.append(int(idx[int(np.argmin(np.asarray(sums, dtype=np.float64)))]))
    levels = np.full((len(rows), fp.shape[1]), np.nan)
    for k, p in enumerate(rows):
        levels[k, :counts[p]] = fp[p, :counts[p]]
    return Templates(names, levels, counts[rows].astype(np.int32))


def save_templates(path, templates: Templates):
    """an .npz with names, levels [nt, Et] (NaN beyond each count) and counts"""
    lv = np.array(templates.levels, dtype=np.float64)
    counts = np.asarray(templates.counts, dtype=np.int32).reshape(-1)
    for k in range(lv.shape[0]):
        lv[k, counts[k]:] = np.nan
    with open(path, "wb") as fh:
        np.savez(fh, names=np.asarray([str(s) for s in templates.names]), levels=lv, counts=counts)


def load_templates(path) -> Templates:
    """save_templates' file, checked: ValueError for a file that is not one"""
    try:
        with np.load(path, allow_pickle=False) as z:
            names, lv, counts = [str(s) for s in z["names"]], np.asarray(z["levels"], dtype=np.float64), np.asarray(z["counts"])
    except (OSError, KeyError, ValueError, EOFError) as e:
        raise ValueError("not a template file (%s): %s" % (path, e)) from e
    if lv.ndim != 2 or counts.ndim != 1 or not np.issubdtype(counts.dtype, np.integer) or not len(names) == lv.shape[0] == counts.size:
        raise ValueError("not a template file (%s): names [nt], levels [nt, Et] and counts [nt] are needed" % path)
    t = Templates(names, lv, counts.astype(np.int32))
    if not (1 <= lv.shape[0] <= lib.DTW_MAX_TEMPLATES and 1 <= lv.shape[1] <= lib.FINGERPRINT_MAX_EVENTS and counts.min() >= 1
            and _nan_only_beyond(t)):
        raise ValueError("not a template file (%s): 1 to %d templates of 1 to %d finite levels each are needed"
                         % (path, lib.DTW_MAX_TEMPLATES, lib.FINGERPRINT_MAX_EVENTS))
    return t


def template_arrays(templates: Templates):
    """(levels with 0.0 for the NaN padding, counts): what Engine.dtw_assign takes"""
    if not _nan_only_beyond(templates):
        raise ValueError("template values inside their count must be finite")
    return _templates(np.where(np.isnan(templates.levels), 0.0, templates.levels), templates.counts)


__all__ = ["FingerprintParams", "EventLevels", "Templates", "BarcodeAssignment", "event_levels", "event_levels_batch", "event_levels_packed", "dtw_distances",
           "assign_barcodes", "medoid_templates", "save_templates", "load_templates"]
