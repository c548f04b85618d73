"""The adapter-front post-pass (adp_adapter_front, include/adapted_hip_adapter_front.h; adapted_amd/adapter_front.py) in numpy: its
exact oracle on ROW_DTYPE rows.  The detector is tests/startmods_module_restated.py's adapter_start_details (pinned to the real
reference's vectors by tests/test_startmods_module_cpu.py), the statistics are tests/sigstats_module_restated.py's seg_stats
(numpy's own mean / std / median in float32).  TEST INFRASTRUCTURE: numpy on the CPU."""
import types
import warnings

import numpy as np

import sigstats_module_restated as S
import startmods_module_restated as R

ROW_ADAPTER_FRONT = 8
C_START, C_END, C_LEN, C_MEAN = 2, 3, 4, 5  # adapter_start, adapter_end, adapter_len, adapter_mean (.. std, med, mad) of row["col"]
ST_SKIPPED, ST_OK, ST_VALUE = -1, 0, 2


def params(window=100, min_obs_adapter=2500, min_shift=20.0, min_pA_current=90.0, min_adapter_len=0):
    """the reference's MMAdapterStartConfig defaults, plus the least adapter a patched row may be left with"""
    return types.SimpleNamespace(window=int(window), min_obs_adapter=int(min_obs_adapter), min_shift=float(min_shift),
                                 min_pA_current=float(min_pA_current), min_adapter_len=int(min_adapter_len))


def bounds_of(row, m):
    """(a0, ae) of a row the pass looks at, else None: success == 1, adapter_end present, 0 <= a0 <= ae <= m"""
    pres = int(row["present"])
    if int(row["success"]) != 1 or not pres >> C_END & 1:
        return None
    a0 = int(row["col"][C_START]) if pres >> C_START & 1 else 0
    ae = int(row["col"][C_END])
    return (a0, ae) if 0 <= a0 <= ae <= m else None


def front(sig, rows, p):
    """sig: float32 [n, m], the calibrated minibatch as the detect call took it (NaN behind each read's end); rows: ROW_DTYPE [n]
    -> (patched copy of rows, info int32 [n, 4], shift int64 [n], cand int64 [n], diff float64 [n])"""
    sig = np.asarray(sig)
    assert sig.dtype == np.float32 and sig.ndim == 2
    n, m = sig.shape
    out = np.array(rows, copy=True)
    assert out.shape == (n,)
    info = np.zeros((n, 4), dtype=np.int32)
    info[:, 0] = ST_SKIPPED
    shift, cand, diff = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64), np.zeros(n)
    take = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in range(n):
            b = bounds_of(out[r], m)
            if b is None:
                continue
            a0, ae = b
            x = sig[r, a0:ae]
            info[r, 0] = ST_OK
            try:
                s, _, c, val = R.adapter_start_details(x, p)
            except ValueError:
                info[r] = (ST_VALUE, p.window, max(x.size - p.min_obs_adapter, 0), 0)
                continue
            shift[r], cand[r], diff[r] = int(s), c, val
            if s > 0 and ae - (a0 + int(s)) >= p.min_adapter_len:
                info[r, 3] = 1
                take.append((r, a0 + int(s), ae))
    if take:
        rr, starts, ends = (np.asarray(v, dtype=np.int64) for v in zip(*take))
        _, stats = S.seg_stats(sig, np.full(n, m), rr, starts, ends)
        for (r, start, ae), st in zip(take, stats):
            out["col"][r, C_START], out["col"][r, C_LEN] = start, ae - start
            out["col"][r, C_MEAN:C_MEAN + 4] = st
            out["present"][r] |= np.uint64(1 << C_START | 31 << C_LEN)
            out["reserved_"][r] |= ROW_ADAPTER_FRONT
    return out, info, shift, cand, diff


def make_rows(bounds, success=None):
    """hand-made rows of a detect call: (a0 or None, ae) per read -> ROW_DTYPE rows with adapter_start (absent for None),
    adapter_end, adapter_len and placeholder statistics present, success 1 unless given"""
    from adapted_amd import lib

    rows = lib.empty_rows(len(bounds))
    for r, (a0, ae) in enumerate(bounds):
        rows["col"][r, C_END], rows["col"][r, C_LEN] = ae, ae - (a0 or 0)
        rows["col"][r, C_MEAN:C_MEAN + 4] = (-1.0, -2.0, -3.0, -4.0)
        rows["present"][r] = 1 << C_END | 31 << C_LEN
        if a0 is not None:
            rows["col"][r, C_START] = a0
            rows["present"][r] |= np.uint64(1 << C_START)
    rows["success"] = 1 if success is None else success
    rows["col"][:, 30:38] = np.arange(8) + 0.5  # (bytes the pass must leave alone: the MVS and real-range columns)
    rows["present"] |= np.uint64(255 << 30)
    return rows
