"""The adapter's front boundary (an extension).  ``DetectResults.adapter_start`` is 0 on almost every read: the reference moves it
in one place only -- validate_boundaries sets it to the last open pore above 200 pA inside the adapter -- so a stall or start peak
at 100-190 pA in front of the adapter stays inside [adapter_start, adapter_end) and with it in adapter_len / mean / std / med /
mad, in the translocation speed of ``--polya_length adapter`` and in the first events of every fingerprint.  The reference ships
the remedy, ``adapted.detect.adapter_start.moving_mean_adapter_start_detect``, and never calls it.

``adapter_front_rows`` runs that detector as a post-pass over the result rows of a detect call, on the GPU, on the calibrated
samples the call took (adp_adapter_front / adp_adapter_front_i16, include/adapted_hip_adapter_front.h).  For every row with
success == 1 and an adapter end, with a0 = adapter_start (0 if absent) and ae = adapter_end:

    s = moving_mean_adapter_start_detect(pA[r, a0:ae], params)   (float32 arithmetic, as adapted_amd.detect.adapter_start's)
    s > 0 and ae - (a0 + s) >= min_adapter_len: adapter_start = a0 + s, adapter_len = ae - adapter_start, adapter_mean / std /
        med / mad = calc_partition_stats(pA[r, adapter_start:ae]), bit 3 of the row's ``reserved_`` (lib.ROW_ADAPTER_FRONT)
    otherwise -- a failing row, s == 0, a NaN in the slice, too little adapter left, or bottleneck's ValueError for a slice
        shorter than min_obs_adapter + window (status 2) -- the row keeps every byte.

Every other byte of a patched row stays: real_adapter_*, adapter_rna_median_shift, the MVS columns, open_pores, success and
fail_code are those of the validation with the first adapter_start.  VALIDATION IS NOT REPEATED.

``AdapterFrontParams.revalidate`` (the command line's --adapter_front_revalidate) asks for the other mode: validation IS repeated
for every read the detector accepts (adp_adapter_front_revalidate / _i16, include/adapted_hip_revalidate.h).  Such a read is
validated again with Boundaries.adapter_start = a0 + s and the bounds its first validation took (the primary adapter end and the
poly(A) candidates, read back from the row; a row flagged polya_truncated is validated as the truncation look validated it).  A
validation that passes REPLACES the row -- adapter_med / adapter_mad, open_pores, real_adapter_*, the MVS mean gate whose range
follows adapter_med, and the partitions are those of the trimmed adapter; the start-peak columns, polya_candidates and
``reserved_`` bits 0-2 are carried over, bits 3 and 4 (lib.ROW_REVALIDATED) set.  A validation that fails leaves every byte of the
row: the trim is rejected, adapter_start does not move and bit 3 is not set -- an opt-in, untuned pass never costs a read its pass
status.  This mode needs the detect call's own engine (its configuration is the validation's), host rows, min_adapter_len >= 1
and a configuration without mvs_detect_overwrite.

The defaults of ``AdapterFrontParams`` are the reference's MMAdapterStartConfig (window 100, min_obs_adapter 2500, min_shift 20,
min_pA_current 90).  They are UNTUNED for RNA004, and nothing here has been validated on real pod5 data.  This module is not part
of ``adapted_amd.detect``, which mirrors the reference's package name for name.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import lib

ST_SKIPPED, ST_OK, ST_VALUE = -1, 0, 2  # info[:, 0]: the row was not looked at; fine; the reference raises bottleneck's ValueError


@dataclass
class AdapterFrontParams:
    """window, min_obs_adapter, min_shift, min_pA_current: MMAdapterStartConfig's fields with the reference's defaults (untuned
    for RNA004); min_adapter_len: the least adapter a patched row may be left with (the command line passes
    core.min_obs_adapter)."""
    window: int = 100
    min_obs_adapter: int = 2500
    min_shift: float = 20.0
    min_pA_current: float = 90.0
    min_adapter_len: int = 0
    revalidate: bool = False  # validate the accepted reads again from the trimmed start; a failing validation rejects the trim

    def args(self) -> "lib.AdpAdapterFrontArgs":
        a = lib.AdpAdapterFrontArgs()
        a.min_shift, a.min_pA_current = float(self.min_shift), float(self.min_pA_current)
        a.window, a.min_obs_adapter, a.min_adapter_len = int(self.window), int(self.min_obs_adapter), int(self.min_adapter_len)
        return a

    @classmethod
    def parse(cls, text: str, min_adapter_len: int = 0, revalidate: bool = False) -> "AdapterFrontParams":
        """"WINDOW,MIN_OBS_ADAPTER,MIN_SHIFT,MIN_PA" (the command line's --adapter_front_params)"""
        parts = [p.strip() for p in str(text).split(",")]
        if len(parts) != 4:
            raise ValueError("adapter-front parameters are WINDOW,MIN_OBS_ADAPTER,MIN_SHIFT,MIN_PA")
        p = cls(window=int(parts[0]), min_obs_adapter=int(parts[1]), min_shift=float(parts[2]), min_pA_current=float(parts[3]),
                min_adapter_len=int(min_adapter_len), revalidate=bool(revalidate))
        p.check()
        return p

    def check(self):
        """what the library refuses, said without a GPU (and a shift or a current that is no number, which it would take)"""
        if not 1 <= int(self.window) < 2 ** 31:
            raise ValueError("window must be >= 1")
        if not 0 <= int(self.min_obs_adapter) < 2 ** 31:
            raise ValueError("min_obs_adapter must be >= 0")
        if not 0 <= int(self.min_adapter_len) < 2 ** 31:
            raise ValueError("min_adapter_len must be >= 0")
        for name in ("min_shift", "min_pA_current"):
            if not np.isfinite(float(getattr(self, name))):
                raise ValueError("%s must be finite" % name)


def adapter_front_rows(signals, lens, rows, params: Optional[AdapterFrontParams] = None, device=0, n: Optional[int] = None,
                       m: Optional[int] = None, calibration=None, engine=None):
    """The post-pass over the rows of a detect call.
    signals: the float32 [n, m] minibatch that call took -- a host array, or a device pointer (int) with ``n`` and ``m``; with
    ``calibration`` = (scale, offset) device pointers, a device pointer to the raw int16 [n, m] matrix (m a multiple of 4) and
    ``lens`` the device pointer of the int32 full lengths, as detect_llr_rows_i16 / detect_cnn_rows_i16 take them.  lens is not
    read for float32 signals (the matrix is read as it lies) and may be None.
    rows: the call's rows -- a host ROW_DTYPE array (a patched copy comes back), or a device pointer (patched in place; None comes
    back).
    -> (rows or None, info int32 [n, 4]: status (-1 not looked at, 0, 2 the ValueError), the exception's window and slice size,
    1 where the row was patched; shift int64 [n]: the detector's result; cand int64 [n]; difference[cand] float64 [n])
    With ``params.revalidate`` the accepted reads are validated again (see the module's text): host rows, ``engine`` = the detect
    call's engine, ``lens`` read for float32 signals too, min_adapter_len >= 1; the answer gains a last item, reval int32 [n, 2]:
    (-1, 0) not accepted, (1, 0) replaced, (0, fail_code) the trim was rejected -- and info[:, 3] is 1 only where the row was
    replaced."""
    params = params or AdapterFrontParams()
    params.check()
    host_rows = not isinstance(rows, int)
    if host_rows:
        rows = np.array(rows, dtype=lib.ROW_DTYPE, copy=True).reshape(-1)
        nn = rows.size
        if n is not None and int(n) != nn:
            raise ValueError("need one row per read")
    elif n is None:
        raise ValueError("device rows need n")
    else:
        nn = int(n)
    reval = bool(getattr(params, "revalidate", False))
    if reval:
        if not host_rows:
            raise ValueError("the re-validating form takes host rows")
        if engine is None:
            raise ValueError("the re-validating form needs the detect call's engine (its configuration is the validation's)")
        if int(params.min_adapter_len) < 1:
            raise ValueError("the re-validating form needs min_adapter_len >= 1")
    if nn == 0:
        empty = ((rows if host_rows else None), np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
        return empty + ((np.zeros((0, 2), dtype=np.int32),) if reval else ())
    if engine is None:
        from .detect._rows import _engine

        engine = _engine(device)
    if calibration is not None:
        if not isinstance(signals, int) or not isinstance(lens, int) or m is None:
            raise ValueError("raw int16 rows are device memory: pointers to the samples, the full lengths and the calibration, with n and m")
        fn = engine.adapter_front_revalidate_i16 if reval else engine.adapter_front_i16
        out = fn(signals, lens, calibration[0], calibration[1], rows, params.args(), n=nn, m=m)
    else:
        out = (engine.adapter_front_revalidate if reval else engine.adapter_front)(signals, lens, rows, params.args(), n=nn, m=m)
    return ((rows if host_rows else None),) + out


__all__ = ["AdapterFrontParams", "adapter_front_rows", "ST_SKIPPED", "ST_OK", "ST_VALUE"]
