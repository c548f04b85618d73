"""adp_dtw_align and adp_dba_step (include/adapted_hip_templates.h) in numpy, cell by cell: their exact oracle.  Every operation is
float64 in the order the header writes it, so device results are compared bit for bit (fingerprint_oracle.same)."""
import numpy as np

from fingerprint_oracle import dtw_pair, same  # noqa: F401  (same: what the tests compare with)


def matrix(a, c, band=0):
    """D [n + 1, m + 1] of one pair: matrix_cells' values, one anti-diagonal i + j = s per step (a cell's value does not depend on
    the order of the visits, and every cell sees the same operations -- fingerprint_oracle.dtw does the same over all pairs)"""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    n, m = a.size, c.size
    R = max(band, abs(n - m)) if band > 0 else n + m
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    with np.errstate(over="ignore"):
        for s in range(2, n + m + 1):
            i = np.arange(max(1, s - m), min(n, s - 1) + 1)
            j = s - i
            d = a[i - 1] - c[j - 1]
            v = d * d + np.minimum(np.minimum(D[i - 1, j], D[i, j - 1]), D[i - 1, j - 1])
            D[i, j] = np.where(np.abs(i - j) <= R, v, np.inf)
    return D


def matrix_cells(a, c, band=0):
    """D [n + 1, m + 1] of one pair, cell by cell as fingerprint_oracle.dtw_pair makes it"""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    n, m = a.size, c.size
    R = max(band, abs(n - m)) if band > 0 else n + m
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    with np.errstate(over="ignore"):
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                if abs(i - j) <= R:
                    d = a[i - 1] - c[j - 1]
                    D[i, j] = d * d + min(min(D[i - 1, j], D[i, j - 1]), D[i - 1, j - 1])
    return D


def path(D):
    """the cells (i, j), 1-based, from (n, m) back to (1, 1): left at i == 1, up at j == 1, else the predecessor of the least D --
    the diagonal first on equal values, then up, then left"""
    i, j = D.shape[0] - 1, D.shape[1] - 1
    cells = [(i, j)]
    while i > 1 or j > 1:
        if i == 1:
            j -= 1
        elif j == 1:
            i -= 1
        else:
            dg, up, lf = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
            if dg <= up and dg <= lf:
                i, j = i - 1, j - 1
            elif up <= lf:
                i -= 1
            else:
                j -= 1
        cells.append((i, j))
    return cells


def align_pair(a, c, Et, band=0):
    """-> (dist, status 0 or 2, lo int32 [Et], hi int32 [Et], sum float64 [Et], the path's cells or None) of a usable query"""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    D = matrix(a, c, band)
    dist = D[a.size, c.size]
    lo, hi, sm = np.full(Et, -1, dtype=np.int32), np.full(Et, -1, dtype=np.int32), np.full(Et, np.nan)
    if not np.isfinite(dist):
        return dist, 2, lo, hi, sm, None
    cells = path(D)
    for i, j in cells:  # (i descends along the path)
        if hi[j - 1] < 0:
            hi[j - 1] = i - 1
        lo[j - 1] = i - 1
    for j in range(c.size):
        s = a[lo[j]]
        for i in range(lo[j] + 1, hi[j] + 1):
            s = s + a[i]
        sm[j] = s
    return dist, 0, lo, hi, sm, cells


def usable(q, q_count):
    q, qc = np.asarray(q, dtype=np.float64), np.asarray(q_count, dtype=np.int64)
    return np.asarray([1 <= qc[p] <= q.shape[1] and bool(np.isfinite(q[p, :qc[p]]).all()) for p in range(q.shape[0])], dtype=bool).reshape(-1)


def align(q, q_count, which, t, t_count, band=0):
    """adp_dtw_align -> dict: dist [nq], status int32 [nq], lo / hi int32 [nq, Et], sum float64 [nq, Et]"""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    nq, Et = q.shape[0], t.shape[1]
    ok = usable(q, q_count)
    out = {"dist": np.full(nq, np.nan), "status": np.zeros(nq, dtype=np.int32), "lo": np.full((nq, Et), -1, dtype=np.int32),
           "hi": np.full((nq, Et), -1, dtype=np.int32), "sum": np.full((nq, Et), np.nan)}
    for p in range(nq):
        k = int(which[p])
        if k < 0:
            out["status"][p] = 3
        elif not ok[p]:
            out["status"][p] = 1
        else:
            d, st, lo, hi, sm, _ = align_pair(q[p, :q_count[p]], t[k, :t_count[k]], Et, band)
            out["dist"][p], out["status"][p], out["lo"][p], out["hi"][p], out["sum"][p] = d, st, lo, hi, sm
    return out


def dba_step(q, q_count, which, t, t_count, band=0):
    """adp_dba_step -> (t_new [nt, Et], members int32 [nt], inertia [nt], dist [nq])"""
    t = np.asarray(t, dtype=np.float64)
    nt, Et = t.shape
    r = align(q, q_count, which, t, t_count, band)
    t_new, members, inertia = np.full((nt, Et), np.nan), np.zeros(nt, dtype=np.int32), np.zeros(nt)
    for k in range(nt):
        m = int(t_count[k])
        idx = [p for p in range(len(which)) if which[p] == k and r["status"][p] == 0]
        members[k] = len(idx)
        if not idx:
            t_new[k, :m] = t[k, :m]
            continue
        T, N, acc = np.zeros(m), np.zeros(m, dtype=np.int64), 0.0
        for p in idx:
            T = T + r["sum"][p, :m]
            N = N + (r["hi"][p, :m].astype(np.int64) - r["lo"][p, :m] + 1)
            acc = acc + r["dist"][p]
        t_new[k, :m] = T / N.astype(np.float64)
        inertia[k] = acc
    return t_new, members, inertia, r["dist"]
