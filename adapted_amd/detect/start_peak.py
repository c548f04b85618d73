"""The reference's start-peak module ``adapted.detect.start_peak`` on the HIP library: `detect_rna_start_peak` with the same
arguments and the same ``DataFrame`` (seven columns, None / NaN cells, indices in samples), so that
``from adapted.detect.start_peak import detect_rna_start_peak`` can become ``from adapted_amd.detect.start_peak import ...``.
Next to it sits `detect_rna_start_peak_batch`: the raw per-read values of a host array or of signals resident on the device.

Both are one call of adp_start_peak (k_startpeak_mod: adapted_amd/csrc/startmods_api.h), which takes every parameter as an
argument and float32 or float64 signals; the detect pipeline's own start peak (adp_detect_start_peak, the engine's configuration,
float32, folded into the result rows) is another kernel and computes the same values on the same input.  There is no CPU path:
without the HIP library every function raises ``HipLibraryError``.

Dtypes: float32 pools and compares in float32, float64 in float64; integers are widened to float64 (numpy's own result type for
their pooled means).  The reference's quirks are kept: the open-pore scan reads the first ``min(len, m) // downscale_factor`` RAW
samples; a ragged last block is pooled over zeros; a NaN in ``[offset1:start_peak_max_idx]`` is the maximum, equals nothing and
exceeds nothing; an empty slice or a successor index past the pooled row is the reference's caught exception: an all-None row;
a read shorter than one block makes the whole call raise numpy's ValueError (the batch form reports no open pore for it).

Differences from the reference: a negative offset1, offset2 or start_peak_max_idx and negative lengths raise ValueError (the
reference gives them Python's slice wrap-around meaning); a downscale_factor below 1 raises ValueError.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import lib
from ._rows import _engine, as_work

FLAGGED_TYPES = lib.START_PEAK_TYPES  # code of `flagged_type` -> the reference's string (0: None)

# what `detect_rna_start_peak_batch` returns per read; indices in SAMPLES (pooled index * downscale_factor), -1 for None
BATCH_DTYPE = np.dtype([("valid", "?"), ("start_peak_idx", "<i8"), ("start_peak_pa", "<f8"), ("next_greater_idx", "<i8"),
                        ("next_greater_pa", "<f8"), ("open_pore_idx", "<i8"), ("flagged_type", "<i4")])


def _args(params) -> "lib.AdpStartPeakArgs":
    a = lib.AdpStartPeakArgs()
    a.open_pore_pa = float(params.open_pore_pa)
    for k in ("downscale_factor", "start_peak_max_idx", "offset1", "offset2"):
        setattr(a, k, int(getattr(params, k)))
    if a.downscale_factor < 1:
        raise ValueError("downscale_factor must be >= 1")
    if min(a.start_peak_max_idx, a.offset1, a.offset2) < 0:
        raise ValueError("start_peak_max_idx, offset1 and offset2 must be >= 0 (negative positions are not supported)")
    return a


def detect_rna_start_peak_batch(signals, full_signal_lens, params, device=0, n: Optional[int] = None, m: Optional[int] = None,
                                dtype=np.float32):
    """`detect_rna_start_peak`'s per-read values for signals [n, m] -- a host array, or a device pointer (int) with ``n``, ``m``
    and ``dtype`` -- and the reads' full lengths (they may exceed m).  ``params``: any object with downscale_factor,
    start_peak_max_idx, offset1, offset2 and open_pore_pa (``spc.rna_start_peak``).  -> a structured array [n] (BATCH_DTYPE):
    valid (False: the reference's row is all None), the two indices in samples and their pooled values (the input type's), the
    open pore's index (-1: None) and the flagged type's code (FLAGGED_TYPES)"""
    a = _args(params)
    lens = np.asarray(full_signal_lens, dtype=np.int64).reshape(-1)
    if isinstance(signals, int):
        if n is None or m is None:
            raise ValueError("a device pointer needs n and m")
        dt = np.dtype(dtype)
        if dt not in (np.float32, np.float64):
            raise TypeError("device signals must be float32 or float64")
        x, nn, f64 = signals, int(n), dt == np.float64
    else:
        x = as_work(signals)
        if x.ndim != 2:
            raise ValueError("signals must be [n, m]")
        nn, f64 = x.shape[0], x.dtype == np.float64
    if lens.size != nn or (lens.size and (lens.min() < 0 or lens.max() > np.iinfo(np.int32).max)):
        raise ValueError("need one full length per read, 0 <= full_signal_lens < 2^31")
    out = np.zeros(nn, dtype=BATCH_DTYPE)
    out["open_pore_idx"] = -1
    if nn == 0 or (not isinstance(x, int) and x.shape[1] == 0):
        return out
    info, vals = _engine(device).start_peak(x, lens, a, n=n, m=m, f64=f64)
    ds = a.downscale_factor
    ok = info[:, 0] != 0
    out["valid"] = ok
    out["start_peak_idx"] = np.where(ok, info[:, 1].astype(np.int64) * ds, 0)
    out["next_greater_idx"] = np.where(ok, info[:, 2].astype(np.int64) * ds, 0)
    out["start_peak_pa"], out["next_greater_pa"] = vals[:, 0], vals[:, 1]
    out["open_pore_idx"] = np.where(info[:, 3] >= 0, info[:, 3].astype(np.int64) * ds, -1)
    out["flagged_type"] = info[:, 4]
    return out


def detect_rna_start_peak(batch_of_signals: np.ndarray, full_signal_lens: np.ndarray, spc):
    """start_peak.py:7-119 -> the reference's DataFrame: start_peak_idx, start_peak_pa, next_greater_idx, next_greater_pa,
    open_pore_idx, flagged_type, scale"""
    import pandas as pd

    x = as_work(batch_of_signals)
    if x.ndim != 2:
        raise ValueError("batch_of_signals must be [n, m]")
    sp = spc.rna_start_peak
    lens = np.asarray(full_signal_lens, dtype=np.int64).reshape(-1)
    if lens.size == x.shape[0] and (np.minimum(lens, x.shape[1]) // max(int(sp.downscale_factor), 1) == 0).any():
        # (the open-pore scan of a read shorter than one block: np.argmax outside the reference's try block)
        raise ValueError("attempt to get argmax of an empty sequence")
    rows = detect_rna_start_peak_batch(x, lens, sp)
    ds, val = int(sp.downscale_factor), x.dtype.type
    # the per-read tuples as the reference collects them: POOLED indices, numpy scalars of the arrays' types, None
    res = []
    for r in rows:
        if not r["valid"]:
            res.append((None,) * 6)
            continue
        flagged = int(r["flagged_type"]) != 0
        res.append((np.int64(r["start_peak_idx"] // ds), val(r["start_peak_pa"]), np.int64(r["next_greater_idx"] // ds),
                    val(r["next_greater_pa"]), np.int64(r["open_pore_idx"] // ds) if flagged else None,
                    FLAGGED_TYPES[int(r["flagged_type"])]))
    # the frame by pandas itself, with the reference's operations in their order: the column dtypes are what the installed
    # pandas makes of them (float64 columns; object columns when every row is None)
    df = pd.DataFrame(res, columns=["start_peak_idx", "start_peak_pa", "next_greater_idx", "next_greater_pa", "open_pore_idx",
                                    "flagged_type"])
    both = df.next_greater_pa.notna() & df.start_peak_pa.notna()
    df.loc[both, "scale"] = df.loc[both, "next_greater_pa"] / df.loc[both, "start_peak_pa"]
    for col in ("start_peak_idx", "next_greater_idx", "open_pore_idx"):  # back to samples, only where there is an index
        have = df[col].notna()
        df.loc[have, col] = (df.loc[have, col] * ds).astype(int)
    return df


__all__ = ["detect_rna_start_peak", "detect_rna_start_peak_batch"]
