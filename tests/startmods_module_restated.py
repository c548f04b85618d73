"""A CPU restatement of the reference's start-peak and adapter-start modules (adapted/detect/start_peak.py, adapter_start.py) with
numpy only, in the project's own words.  bottleneck's move_mean is tests/mvs_module_restated.py's (bottleneck/src/move_template.c
as it runs, NaN-aware, in the input dtype); tests/test_startmods_module_cpu.py pins both functions to the fixture the real
reference wrote (tests/golden/startmods_module.npz).  Integer input is widened to float64.  TEST INFRASTRUCTURE."""
import numpy as np

from mvs_module_restated import move_mean, work

FLAGS = {1: "open pore in adapter", 2: "potential concatemer adapter-only read"}


# ---------------------------------------------------------------- adapter start
def adapter_start_details(x, params):
    """-> (adapter_start or 0, accepted, cand (-1: difference is empty), difference[cand] (0.0 then)); raises bottleneck's
    ValueError.  The moving mean runs DOWN the read (over the reversed slice); both cumulative sums are sequential in the
    dtype; their means and the difference are float64 (numpy's result type of a float array by an int64 array)"""
    x = work(x)
    w, mo = int(params.window), int(params.min_obs_adapter)
    used = x[:max(x.size - mo, 0)]
    mm = move_mean(used[::-1], w)  # (raises for a slice shorter than the window)
    rev = mm[w:]
    size = rev.size
    if size == 0:
        return 0, False, -1, 0.0
    fwd = rev[::-1]
    fsum = np.cumsum(fwd)
    bsum = np.cumsum(rev)[::-1]
    pos = np.arange(size, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = bsum / (size - pos) - fsum / (pos + 1)
    assert diff.dtype == np.float64
    top = diff.max()  # (NaN when any entry is)
    diff[:w] = top
    cand = int(np.argmin(diff))  # (the first NaN, else the first minimum)
    val = float(diff[cand])
    h = w // 2
    near = fwd[max(0, cand - h):cand + h]
    level = x.dtype.type(params.min_pA_current) if x.dtype == np.float32 else float(params.min_pA_current)
    ok = bool(val < -float(params.min_shift)) and bool((near > level).any())
    return (np.int64(cand + h) if ok else 0), ok, cand, val


def adapter_start(x, params):
    return adapter_start_details(x, params)[0]


# ---------------------------------------------------------------- start peak
def pooled(X, ds):
    """non-overlapping block means over zeros behind the row's end, in numpy's own order"""
    n, m = X.shape
    pad = (-m) % ds
    if pad:
        X = np.concatenate([X, np.zeros((n, pad), dtype=X.dtype)], axis=1)
    return X.reshape(n, -1, ds).mean(axis=2)


def start_peak_rows(X, full_lens, sec):
    """per read (valid, start_peak_idx, start_peak_pa, next_greater_idx, next_greater_pa, open_pore_idx or -1, flag code), POOLED
    indices"""
    X = work(X)
    n, m = X.shape
    ds, spmax, o1, o2 = int(sec.downscale_factor), int(sec.start_peak_max_idx), int(sec.offset1), int(sec.offset2)
    level = X.dtype.type(sec.open_pore_pa)
    ends = np.minimum(np.asarray(full_lens, dtype=np.int64), m) // ds
    P = pooled(X, ds)
    width = P.shape[1]
    rows = []
    with np.errstate(invalid="ignore"):
        for r in range(n):
            e = int(ends[r])
            above = np.flatnonzero(X[r, :e] > level)  # (RAW samples, the first `e` of them)
            pore = int(above[0]) // ds if above.size else 0
            head = P[r, o1:spmax]
            tail = P[r, spmax + o2:e]
            if head.size == 0 or tail.size == 0:
                rows.append((False, 0, 0.0, 0, 0.0, -1, 0))
                continue
            if np.isnan(head).any():
                top, at = X.dtype.type(np.nan), o1
            else:
                top = head.max()
                at = int(np.flatnonzero(head == top)[0]) + o1
            over = np.flatnonzero(tail > top)
            nxt = (int(over[0]) if over.size else 0) + spmax + o2
            if nxt >= width:
                rows.append((False, 0, 0.0, 0, 0.0, -1, 0))
                continue
            flag = 0
            if pore > 0:
                if abs(float(nxt) - float(pore)) <= 2.0 + 0.01 * abs(float(pore)):
                    flag = 1
                elif at < pore < nxt:
                    flag = 2
            rows.append((True, at, top, nxt, P[r, nxt], pore if flag else -1, flag))
    return rows


def start_peak_frame(X, full_lens, sec):
    """the reference's DataFrame from those rows, built by pandas with the reference's operations in their order"""
    import pandas as pd

    ds = int(sec.downscale_factor)
    res = []
    for ok, at, top, nxt, nv, pore, flag in start_peak_rows(X, full_lens, sec):
        res.append((np.int64(at), top, np.int64(nxt), nv, np.int64(pore) if flag else None, FLAGS.get(flag)) if ok else (None,) * 6)
    df = pd.DataFrame(res, columns=["start_peak_idx", "start_peak_pa", "next_greater_idx", "next_greater_pa", "open_pore_idx",
                                    "flagged_type"])
    both = df.next_greater_pa.notna() & df.start_peak_pa.notna()
    df.loc[both, "scale"] = df.loc[both, "next_greater_pa"] / df.loc[both, "start_peak_pa"]
    for col in ("start_peak_idx", "next_greater_idx", "open_pore_idx"):
        have = df[col].notna()
        df.loc[have, col] = (df.loc[have, col] * ds).astype(int)
    return df
