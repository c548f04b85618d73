"""An independent numpy restatement of the partition statistics the drop-in ``adapted_amd.partition.signal_partitions`` returns:
the statistics of many segments at once (`seg_stats`), and on top of it the module's surface with result types of the same names
and fields, so that tests/sigstats_module_cases.py encodes both alike.  TEST INFRASTRUCTURE: numpy on the CPU."""
import dataclasses
import warnings
from typing import Optional

import numpy as np


def _work(x):
    x = np.asarray(x)
    return x.astype(np.float64) if np.issubdtype(x.dtype, np.integer) else x


def seg_stats(x, lens, rows, starts, ends):
    """signals [n, L] (float32 / float64; integers are widened to float64), lens [n], segments (row, start, end) with -1 for
    None -> (length int64 [G]: end - start, -1 where a position is None or end <= start; stats float64 [G, 4]: mean, std,
    median, MAD of the slice clipped to the read, in the signals' type, NaN where the length is -1 or the slice is empty)"""
    x = _work(x)
    rows, starts, ends = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (rows, starts, ends))
    live = (starts >= 0) & (ends > starts)
    length = np.where(live, ends - starts, -1)
    stats = np.full((rows.size, 4), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for g in np.flatnonzero(live):
            s = x[rows[g], :lens[rows[g]]][starts[g]:ends[g]]
            if s.size == 0:
                continue
            med = np.median(s)
            dev = np.abs(s - s.dtype.type(med))
            stats[g] = (np.mean(s), np.std(s), med, np.median(dev))
    return length, stats


@dataclasses.dataclass
class Partition:
    start: Optional[int]
    len: Optional[int]
    mean: Optional[float]
    std: Optional[float]
    med: Optional[float]
    mad: Optional[float]

    def to_dict(self, name=""):
        return {(name + "_" if name else "") + f.name: getattr(self, f.name) for f in dataclasses.fields(self)}


@dataclasses.dataclass
class Partitions:
    adapter: Partition
    polya: Partition
    rna: Partition

    def to_dict(self, name=""):
        out = {}
        for f in dataclasses.fields(self):
            out.update(getattr(self, f.name).to_dict((name + "_" if name else "") + f.name))
        return out


def _m1(v):
    return -1 if v is None else int(v)


def _many(x, segs):
    """segs: (start, end) pairs of the 1-D signal x, None allowed -> a Partition each"""
    x = np.asarray(x).reshape(1, -1)
    length, stats = seg_stats(x, [x.shape[1]], [0] * len(segs), [_m1(s) for s, _ in segs], [_m1(e) for _, e in segs])
    return [Partition(s, None, None, None, None, None) if n < 0 else Partition(s, int(n), *map(float, st))
            for (s, _), n, st in zip(segs, length, stats)]


def calc_partition_stats(signal, start, end):
    return _many(signal, [(start, end)])[0]


def calc_partitions_from_vals(signal, adapter_start, adapter_end, polya_end, polya_truncated=False):
    rna = (None, None) if polya_truncated else (polya_end, np.asarray(signal).size)
    return Partitions(*_many(signal, [(adapter_start, adapter_end), (adapter_end, polya_end), rna]))


def calc_partitions(signal, boundaries):
    return calc_partitions_from_vals(signal, boundaries.adapter_start, boundaries.adapter_end, boundaries.polya_end)


# ---- normalize / downscale / real_range / anomalies ---------------------------------------------------------------------------------
def _median_pair(flat, skip_nan):
    """median and median absolute deviation of a flat array; skip_nan: of its numbers only"""
    if skip_nan:
        flat = flat[flat == flat]
    if flat.size == 0:
        return float("nan"), float("nan")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        med = np.median(flat)
        mad = np.median(np.abs(flat - med))
    return float(med), float(mad)


def med_mad(signal, with_nan=False):
    return _median_pair(_work(signal).reshape(-1), with_nan)


def _winsorise(x, lo, hi):
    """x limited to [lo, hi] (bounds rounded once to x's type); NaN stays"""
    t = x.dtype.type
    return np.minimum(np.maximum(x, t(lo)), t(hi))


def clip_signal(signal, outlier_thresh, med, mad):
    w = float(mad) * outlier_thresh
    return _winsorise(_work(signal), float(med) - w, float(med) + w)


def normalize_signal(signal, outlier_thresh=5.0, with_nan=False):
    if len(signal) == 0:
        return np.zeros(0)
    x = _work(signal)
    med, mad = med_mad(x, with_nan)
    if mad == 0:
        raise ValueError("MAD normalization failed: scale is 0")
    t = x.dtype.type
    with np.errstate(all="ignore"):
        return (clip_signal(x, outlier_thresh, med, mad) - t(med)) / t(mad)


def efficient_average_pooling(data, pool_size=2):
    x = _work(data)
    if x.ndim != 2:
        raise ValueError("Data must be a 2D array")
    n, m = x.shape
    full, rest = divmod(m, pool_size)
    out = np.zeros((n, full + (rest > 0)), dtype=x.dtype)
    out[:, :full] = x[:, :full * pool_size].reshape(n, full, pool_size).sum(axis=2)
    if rest:
        last = np.zeros((n, pool_size), dtype=x.dtype)
        last[:, :rest] = x[:, full * pool_size:]
        out[:, full] = last.sum(axis=1)
    return out / x.dtype.type(pool_size)


def downscale_signal(signal, factor=2):
    return efficient_average_pooling(signal, factor)


def _inside(v, rng):
    lo, hi = rng
    return bool((-np.inf if lo is None else lo) <= v <= (np.inf if hi is None else hi))


def real_range_check(calibrated_signal, params, return_values=False):
    x = _work(calibrated_signal)
    w, n = params.mean_window, x.size
    if n < 2 * w:
        return (False, None, None, None) if return_values else False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first, last = x[:w].mean(), x[n - w:].mean()
        ok, spread = False, None
        if _inside(float(first), params.mean_start_range) and _inside(float(last), params.mean_end_range):
            hi85, lo15 = np.percentile(x[n - min(params.max_obs_local_range, n):], (85, 15))
            spread = hi85 - lo15
            ok = _inside(spread, params.local_range)
    return (ok, first, last, spread) if return_values else ok


def open_pore_positions(x, lo, hi, min_obs_diff):
    """(positions in [lo, hi], those of them at least min_obs_diff behind their predecessor)"""
    x = _work(x)
    inside = np.flatnonzero(((-np.inf if lo is None else lo) <= x) & (x <= (np.inf if hi is None else hi)))
    return inside, inside[1:][np.diff(inside) >= min_obs_diff]


def find_open_pores(signal, sig_range=(200.0, None), min_obs_diff=10):
    inside, far = open_pore_positions(signal, sig_range[0], sig_range[1], min_obs_diff)
    if inside.size <= 1:
        return inside.reshape(-1, 1)
    return far.reshape(-1, 1) if far.size else inside[-1:].copy()
