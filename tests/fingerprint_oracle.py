"""adp_event_levels and adp_dtw_assign (include/adapted_hip_fingerprint.h) in numpy, on top of events_oracle: their exact oracle.
Every operation is float64 in the order the header writes it, so device results are compared bit for bit."""
import warnings

import numpy as np

import events_oracle as eo


def select(b, score, E):
    """the boundaries that stay when at most E - 1 may: the greatest in the order (score, index), in index order"""
    b = np.asarray(b, dtype=np.int64)
    if b.size <= E - 1:
        return b
    order = np.lexsort((b, score[b]))  # ascending by score, then by index
    return np.sort(b[order[b.size - (E - 1):]])


def levels(x, E, w=8, D=8, thr=16.0, var_floor=1e-3):
    """-> dict: nk, seg_status, med_gap, mad_gap (events_oracle.segment's), count, status, lengths int32 [E], levels / fp float64
    [E], norm (med, mad)"""
    x = np.asarray(x)
    b, st, gmed, gmad = eo.segment(x, w, D, thr, var_floor)
    out = {"nk": int(b.size), "seg_status": st, "med_gap": gmed, "mad_gap": gmad, "count": 0, "status": st,
           "lengths": np.zeros(E, dtype=np.int32), "levels": np.full(E, np.nan), "fp": np.full(E, np.nan), "norm": (np.nan, np.nan)}
    if st != 0:
        return out
    if b.size > E - 1:
        b = select(b, eo.scores(x, w, var_floor), E)
    edge = np.concatenate([[0], b, [x.size]]).astype(np.int64)
    c = edge.size - 1
    lev = np.asarray([np.mean(x[edge[e]:edge[e + 1]].astype(np.float64)) for e in range(c)])
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        med = np.median(lev)
        mad = np.median(np.abs(lev - med))
        ok = mad != 0 and np.isfinite(med) and np.isfinite(mad)
        out["count"], out["status"], out["norm"] = c, 0 if ok else 4, (float(med), float(mad))
        out["lengths"][:c] = np.diff(edge)
        out["levels"][:c] = lev
        if ok:
            out["fp"][:c] = (lev - med) / mad
    return out


def dtw_pair(a, c, band=0):
    """one pair, cell by cell as the header writes it"""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    n, m = a.size, c.size
    R = max(band, abs(n - m)) if band > 0 else n + m
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if abs(i - j) <= R:
                d = a[i - 1] - c[j - 1]
                D[i, j] = d * d + min(min(D[i - 1, j], D[i, j - 1]), D[i - 1, j - 1])
    return D[n, m]


def dtw(q, q_count, t, t_count, band=0):
    """-> dist float64 [nq, nt]: dtw_pair for every pair at once, one anti-diagonal i + j = s of all pairs per step (a cell's
    value does not depend on the order of the visits, and every pair's cell sees the same operations); NaN rows for queries whose
    count lies outside [1, Eq] or that hold a non-finite value inside it"""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    qc, tc = np.asarray(q_count, dtype=np.int64), np.asarray(t_count, dtype=np.int64)
    nq, Eq = q.shape
    nt, Et = t.shape
    good = np.asarray([1 <= qc[p] <= Eq and bool(np.isfinite(q[p, :qc[p]]).all()) for p in range(nq)], dtype=bool).reshape(nq)
    n = np.where(good, qc, 1)[:, None]  # [nq, 1]
    m = tc[None, :]  # [1, nt]
    R = (np.maximum(band, np.abs(n - m)) if band > 0 else np.full((nq, nt), Eq + Et))[:, :, None]
    a = np.where(np.isfinite(q), q, 0.0)  # (beyond the counts: cells that D[n][m] does not depend on)
    c = np.where(np.isfinite(t), t, 0.0)
    # d1 / d2: the diagonals s - 1 and s - 2, indexed by i: D[i][s - i]
    d2 = np.full((nq, nt, Eq + 1), np.inf)
    d2[:, :, 0] = 0.0  # s = 0
    d1 = np.full((nq, nt, Eq + 1), np.inf)  # s = 1: D[0][1], D[1][0]
    dist = np.full((nq, nt), np.nan)
    for s in range(2, Eq + Et + 1):
        lo, hi = max(1, s - Et), min(Eq, s - 1)  # rows i of this diagonal; columns j = s - i
        i = np.arange(lo, hi + 1)
        j = s - i
        d = a[:, None, i - 1] - c[None, :, j - 1]
        v = d * d + np.minimum(np.minimum(d1[:, :, i - 1], d1[:, :, i]), d2[:, :, i - 1])
        cur = np.full((nq, nt, Eq + 1), np.inf)
        cur[:, :, lo:hi + 1] = np.where(np.abs(i - j)[None, None, :] <= R, v, np.inf)
        ends = (n + m) == s
        if ends.any():
            dist = np.where(ends, np.take_along_axis(cur, np.broadcast_to(n, (nq, nt))[:, :, None], axis=2)[:, :, 0], dist)
        d2, d1 = d1, cur
    dist[~good] = np.nan
    return dist


def assign(dist):
    """-> (best int32 [nq, 2], bestdist float64 [nq, 2]): the least distance (the lowest index on ties) and the second least; -1 and
    NaN where there is none"""
    nq, nt = dist.shape
    best = np.full((nq, 2), -1, dtype=np.int32)
    bd = np.full((nq, 2), np.nan)
    for p in range(nq):
        if np.isnan(dist[p]).any():
            continue
        order = np.argsort(dist[p], kind="stable")
        best[p, 0], bd[p, 0] = order[0], dist[p, order[0]]
        if nt > 1:
            best[p, 1], bd[p, 1] = order[1], dist[p, order[1]]
    return best, bd


def medoids(dist, labels):
    """per label (sorted): the member with the least sum of distances to the members of its label, the lowest index on ties"""
    labels = np.asarray(labels)
    out = []
    for lab in sorted(set(labels.tolist())):
        idx = np.flatnonzero(labels == lab)
        sums = np.asarray([sum(dist[i, j] for j in idx if j != i) for i in idx])
        out.append(int(idx[int(np.argmin(sums))]))
    return out


def same(a, b):
    """bit for bit, all NaNs counting as one"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
