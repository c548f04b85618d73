"""The reference's partition statistics module ``adapted.partition.signal_partitions`` on the HIP library: its two dataclasses and
three functions with the same arguments, defaults and return types, so that ``from adapted.partition.signal_partitions import ...``
can become ``from adapted_amd.partition.signal_partitions import ...``.  Next to them sit the batch forms (``*_batch``): padded
[n, L] signals with per-read lengths (read r is ``signals[r, :lens[r]]``), or a device pointer (int) with ``n``, ``L`` and
``dtype``, so that resident signals never cross PCIe.

Every statistic is taken by one batch call of segments (adp_seg_stats: adapted_amd/csrc/sigstats_api.h); the per-read functions
are that call with n = 1.  There is no CPU path: without the HIP library every function raises ``HipLibraryError``.

float32 input computes in float32 and float64 in float64, in numpy's order of operations (np.mean, np.std, np.median and the
median of ``np.abs(sig - median)``); integer input is widened to float64, which is what numpy computes for it; anything else
raises TypeError.  What a caller can trip over, as in the reference: ``len`` is ``end - start`` unclipped, also when ``end`` lies
beyond the signal (the statistics are those of the clipped slice); ``start`` at or beyond the signal's size gives four NaN, and
so does a NaN sample anywhere in the slice.

Difference from the reference: negative positions raise ValueError (the reference gives them Python's slice wrap-around
meaning).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..container_types import Boundaries
from ..detect._rows import _engine, position, positions, rows_in


@dataclass
class Partition:
    start: Optional[int]
    len: Optional[int]
    mean: Optional[float]
    std: Optional[float]
    med: Optional[float]
    mad: Optional[float]

    def to_dict(self, name: str = ""):
        prefix = name + "_" if name else ""
        return {prefix + k: getattr(self, k) for k in ("start", "len", "mean", "std", "med", "mad")}


@dataclass
class Partitions:
    adapter: Partition
    polya: Partition
    rna: Partition

    def to_dict(self, name: str = ""):
        prefix = name + "_" if name else ""
        d = {}
        for part in ("adapter", "polya", "rna"):
            d.update(getattr(self, part).to_dict(name=prefix + part))
        return d


def _segments(x, lens, f64, nn, rows, starts, ends, n, L, device):
    """the statistics of signals[rows[g], starts[g]:ends[g]] -> (length int64 [G] (-1: the reference's None), stats float64
    [G, 4] (NaN where the length is None))"""
    live = (starts >= 0) & (ends > starts)
    length = np.where(live, ends - starts, -1)
    stats = np.full((rows.size, 4), np.nan)
    if live.any():
        g = np.flatnonzero(live)
        stats[g], _ = _engine(device).seg_stats(x, lens, rows[g], starts[g], ends[g], n=n, L=L, f64=f64)
    return length, stats


def calc_partition_stats_batch(signals, lens, starts, ends, device=0, n: Optional[int] = None, L: Optional[int] = None,
                               dtype=np.float32):
    """`calc_partition_stats` for many reads -> (length int64 [n], stats float64 [n, 4]: mean, std, med, mad).  starts / ends: -1
    stands for None.  length -1: the reference's ``Partition(start, None, None, None, None, None)`` (a None position, or
    end <= start); the row of stats is NaN then.  Otherwise length is ``end - start``, unclipped."""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    s, e = positions(starts, nn, "starts", True), positions(ends, nn, "ends", True)
    return _segments(x, lens, f64, nn, np.arange(nn, dtype=np.int32), s, np.where(e < 0, -1, e), n, L, device)


def calc_partitions_from_vals_batch(signals, lens, adapter_starts, adapter_ends, polya_ends, polya_truncated=False, device=0,
                                    n: Optional[int] = None, L: Optional[int] = None, dtype=np.float32):
    """`calc_partitions_from_vals` for many reads -> (start int64 [n, 3], length int64 [n, 3], stats float64 [n, 3, 4]); axis 1:
    adapter, poly(A), RNA.  Positions: -1 stands for None (it comes back as the partition's start).  ``polya_truncated``: a bool,
    or one per read; the RNA partition of a truncated read is all None (start -1, length -1, NaN)."""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    a_s, a_e, p_e = (positions(v, nn, w, True) for v, w in ((adapter_starts, "adapter_starts"), (adapter_ends, "adapter_ends"),
                                                       (polya_ends, "polya_ends")))
    trunc = np.broadcast_to(np.asarray(polya_truncated, dtype=bool).reshape(-1), (nn,)) if np.ndim(polya_truncated) else \
        np.full(nn, bool(polya_truncated))
    start = np.stack([a_s, a_e, np.where(trunc, -1, p_e)], axis=1)
    end = np.stack([a_e, p_e, np.where(trunc, -1, lens)], axis=1)
    rows = np.repeat(np.arange(nn, dtype=np.int32), 3)
    length, stats = _segments(x, lens, f64, nn, rows, start.reshape(-1), end.reshape(-1), n, L, device)
    return start, length.reshape(nn, 3), stats.reshape(nn, 3, 4)


def _partition(start, length, stats) -> Partition:
    if length < 0:
        return Partition(start, None, None, None, None, None)
    return Partition(start, int(length), *(float(v) for v in stats))


def _one(signal):
    x = np.asarray(signal).reshape(1, -1)
    return x, [x.shape[1]]


def calc_partition_stats(signal: np.ndarray, start: Optional[int], end: Optional[int]) -> Partition:
    x, lens = _one(signal)
    length, stats = calc_partition_stats_batch(x, lens, [position(start, "start", True)], [position(end, "end", True)])
    return _partition(start, length[0], stats[0])


def calc_partitions_from_vals(signal: np.ndarray, adapter_start: Optional[int], adapter_end: Optional[int],
                              polya_end: Optional[int], polya_truncated: Optional[bool] = False) -> Partitions:
    x, lens = _one(signal)
    _, length, stats = calc_partitions_from_vals_batch(x, lens, [position(adapter_start, "adapter_start", True)],
                                                       [position(adapter_end, "adapter_end", True)], [position(polya_end, "polya_end", True)],
                                                       bool(polya_truncated))
    starts = (adapter_start, adapter_end, None if polya_truncated else polya_end)
    return Partitions(*(_partition(starts[k], length[0, k], stats[0, k]) for k in range(3)))


def calc_partitions(signal: np.ndarray, boundaries: Boundaries) -> Partitions:
    return calc_partitions_from_vals(signal, boundaries.adapter_start, boundaries.adapter_end, boundaries.polya_end)


__all__ = ["Partition", "Partitions", "calc_partitions", "calc_partitions_from_vals", "calc_partition_stats",
           "calc_partition_stats_batch", "calc_partitions_from_vals_batch"]
