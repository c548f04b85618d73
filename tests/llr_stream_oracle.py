"""What the kernels of the LLR path's phase C hand to each other, restated in plain numpy (llr_stream.h: k_cumsum /
k_cumsum_gather -> k_gains<1> -> k_adapter_peak -> k_gains<2> -> k_polya_peak).  TEST INFRASTRUCTURE: imports nothing from the
product.  Functions of a float32 pooled row `down[:n]` or of a float64 trace `g[:n]`; every one is exact, so the device's
buffers are compared bit for bit (the two sums of `nanstd_sums` are compared within the bound of a float64 sum in any order).
"""
import math

import numpy as np

CK = 16        # pooled points per checkpoint
SUMBLK = 64    # trace points per summary block
F64_MAX = np.finfo(np.float64).max


def checkpoints(down, n):
    """-> (ck float64[ceil(n/16), 2], tail float64[2]): ck[q] = (c, c2)[16 q - 1] with ck[0] = (0, 0); tail = (c, c2)[n - 2],
    (0, 0) for n == 1.  c = np.cumsum(down[:n]) in float64 and c2 of the squares: np.cumsum is a sequential recurrence and the
    square of a float32 is exact in float64, so there is nothing to round differently."""
    x = np.asarray(down[:n]).astype(np.float64)
    c, c2 = np.cumsum(x), np.cumsum(x * x)
    nq = (n + CK - 1) // CK
    ck = np.zeros((nq, 2), dtype=np.float64)
    for q in range(1, nq):
        ck[q] = (c[CK * q - 1], c2[CK * q - 1])
    tail = np.array([c[n - 2], c2[n - 2]] if n >= 2 else [0.0, 0.0], dtype=np.float64)
    return ck, tail


def summaries(g, n, sanitised):
    """-> (bmax, bmin) float64[ceil(n/64)] of g[:n].  Pass 1 (sanitised=False): NaN counts as +inf in bmax and is left out of
    bmin (+inf when nothing is left).  Pass 2: both of np.nan_to_num(g)."""
    g = np.asarray(g[:n], dtype=np.float64)
    nb = (n + SUMBLK - 1) // SUMBLK
    bmax, bmin = np.empty(nb), np.empty(nb)
    for b in range(nb):
        v = g[b * SUMBLK: (b + 1) * SUMBLK]
        if sanitised:
            v = np.nan_to_num(v)
            bmax[b], bmin[b] = v.max(), v.min()
        else:
            nan = np.isnan(v)
            bmax[b] = np.inf if nan.any() else v.max()
            bmin[b] = v[~nan].min() if (~nan).any() else np.inf
    return bmax, bmin


def t1(g):
    """LLRTrace._trace_start_end: first and last index whose gain is not <= 0 (NaN counts); (0, size - 1) when there is none"""
    pos = ~(g <= 0)
    if not pos.any():
        return 0, g.size - 1
    idx = np.flatnonzero(pos)
    return int(idx[0]), int(idx[-1])


def nanstd_sums(g):
    """-> (NaN count, fsum of the non-NaN values, fsum of their squares): np.nanstd's input.  An infinity makes fsum raise;
    callers compare the non-finite class with np.sum then."""
    g = np.asarray(g, dtype=np.float64)
    v = g[~np.isnan(g)]
    if not np.isfinite(v).all():
        with np.errstate(invalid="ignore", over="ignore"):
            return int(np.isnan(g).sum()), float(np.sum(v)), float(np.sum(v * v))
    return int(np.isnan(g).sum()), math.fsum(v.tolist()), math.fsum((float(a) * float(a) for a in v.tolist()))


def maxima(g, n, E_minus_ot):
    """-> (idx int64[k], heights float64[k], plateau) on x = np.nan_to_num(g[:n]): the ascending j in [1, n - 2] with
    x[j-1] < x[j] > x[j+1]; plateau: some j has x[j-1] < x[j] == x[j+1], unless x[j] == 0 and j >= E - ot (the zeros behind the
    computed range never peak).  Pass 2: E - ot = n - 2."""
    x = np.nan_to_num(np.asarray(g[:n], dtype=np.float64))
    if n < 3:
        return np.zeros(0, dtype=np.int64), np.zeros(0), False
    a, b, c = x[:-2], x[1:-1], x[2:]
    j = np.arange(1, n - 1)
    strict = (a < b) & (b > c)
    flat = (a < b) & (b == c) & ~((b == 0.0) & (j >= E_minus_ot))
    return j[strict].astype(np.int64), b[strict].copy(), bool(flat.any())
