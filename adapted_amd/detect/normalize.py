"""The reference's normalisation module ``adapted.detect.normalize`` on the HIP library: `med_mad`, `clip_signal` and
`normalize_signal` with the same arguments, defaults and return types, so that ``from adapted.detect.normalize import ...`` can
become ``from adapted_amd.detect.normalize import ...``; next to them `med_mad_batch` and `normalize_signal_batch`, which treat
every row of a padded [n, L] batch by its own median and MAD (a host array with ``lens``, or a device pointer with ``n``, ``L``
and ``dtype``).

The per-read functions take an array of any rank as ONE population, as the reference does (its callers pass a whole [N, m]
minibatch with NaN tails and ``with_nan=True``): adp_med_mad / adp_normalize with ADP_SS_WHOLE (adapted_amd/csrc/
sigstats_api.h).  There is no CPU path: without the HIP library every function raises ``HipLibraryError``.

float32 input computes and returns float32 (the reference's docstring says float64; numpy keeps float32), float64 float64.
Integer input is widened to float64: numpy's own result type for ``np.clip`` of an integer array with Python floats differs
between numpy 1.x and 2.x.  ``med`` and ``mad`` of `clip_signal` are taken as Python floats.
"""
from __future__ import annotations

import logging
from typing import Optional, Tuple

import numpy as np

from ._rows import _engine, as_work, rows_in

ST_MAD_ZERO = 1  # `status` of normalize_signal_batch: the reference raises ValueError


def _population(signal):
    """any array as one population -> (float32 / float64 [1, size], shape)"""
    x = as_work(signal)
    return x.reshape(1, -1), x.shape


def med_mad(signal: np.ndarray, with_nan: bool = False) -> Tuple[float, float]:
    x, _ = _population(signal)
    if x.size == 0:
        return float("nan"), float("nan")
    mm = _engine().med_mad(x, with_nan=bool(with_nan), whole=True)
    return float(mm[0, 0]), float(mm[0, 1])


def clip_signal(signal: np.ndarray, outlier_thresh: float, med: float, mad: float) -> np.ndarray:
    x, shape = _population(signal)
    if x.size == 0:
        return x.reshape(shape)
    out, _, _ = _engine().normalize(x, outlier_thresh=float(outlier_thresh), whole=True, clip_medmad=[[float(med), float(mad)]])
    return out.reshape(shape)


def normalize_signal(signal: np.ndarray, outlier_thresh: float = 5.0, with_nan: bool = False) -> np.ndarray:
    if len(signal) == 0:
        return np.array([], dtype=np.float64)
    x, shape = _population(signal)
    if x.size == 0:
        return x.reshape(shape)
    out, _, status = _engine().normalize(x, outlier_thresh=float(outlier_thresh), with_nan=bool(with_nan), whole=True)
    if status[0]:
        msg = "MAD normalization failed: scale is 0"
        logging.error(msg)
        raise ValueError(msg)
    return out.reshape(shape)


def med_mad_batch(signals, lens, with_nan: bool = False, device=0, n: Optional[int] = None, L: Optional[int] = None,
                  dtype=np.float32):
    """`med_mad` of every read by itself -> float64 [n, 2]: median, MAD (NaN for an empty read)"""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    if nn == 0:
        return np.zeros((0, 2))
    return _engine(device).med_mad(x, lens, with_nan=bool(with_nan), n=n, L=L, f64=f64)


def normalize_signal_batch(signals, lens, outlier_thresh: float = 5.0, with_nan: bool = False, device=0, n: Optional[int] = None,
                           L: Optional[int] = None, dtype=np.float32, out: Optional[int] = None):
    """`normalize_signal` of every read by its own median and MAD -> (normalised [n, L] in the input's type, 0 behind a read's
    end; medmad float64 [n, 2]; status int32 [n]: 1 where the MAD is 0 -- the reference raises ValueError -- and the row is left
    0).  ``out``: a device pointer to write the rows to instead ([n, L]; cells behind a read's end and rows of status 1 are not
    written); the first item is None then."""
    x, lens, f64, nn = rows_in(signals, lens, n, L, dtype)
    if nn == 0:
        return np.zeros((0, 0), dtype=np.float64 if f64 else np.float32), np.zeros((0, 2)), np.zeros(0, dtype=np.int32)
    return _engine(device).normalize(x, lens, float(outlier_thresh), bool(with_nan), n=n, L=L, f64=f64, out_ptr=out)


__all__ = ["med_mad", "clip_signal", "normalize_signal", "med_mad_batch", "normalize_signal_batch"]
