"""include/adapted_hip_clusters.h in plain numpy, from the header alone: the all-pairs DTW matrix (the DTW itself is
fingerprint_oracle's), PAM's BUILD, alternating k-medoids and the silhouette, every float64 sum in THE ORDER the header states, as
explicit loops over the 64 partials' steps and over the fold (vectorised only across what is independent: rows, and the 64
partials).  ``OracleEngine`` stands in for adapted_amd.lib.Engine where a test has no GPU."""
import numpy as np

import fingerprint_oracle as fo

same = fo.same


def osum(terms):
    """THE ORDER over the last axis of ``terms`` [..., n] -> [...]: partial l adds, from +0.0, the terms j = l (mod 64) in
    ascending j; then p[l] += p[l + s] for l < s, s = 32 .. 1"""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[-1]
    p = np.zeros(terms.shape[:-1] + (64,))
    for j0 in range(0, n, 64):
        w = min(64, n - j0)
        p[..., :w] = p[..., :w] + terms[..., j0:j0 + w]
    s = 32
    while s >= 1:
        p[..., :s] = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0].copy()


def usable(q, q_count):
    q, qc = np.asarray(q, dtype=np.float64), np.asarray(q_count)
    return np.asarray([1 <= qc[p] <= q.shape[1] and bool(np.isfinite(q[p, :qc[p]]).all()) for p in range(q.shape[0])], dtype=bool).reshape(-1)


def pairwise(q, q_count, band=0):
    """-> dist float64 [n, n]: pairs i < j as query i against template j, mirrored; a +0.0 diagonal; NaN rows and columns (the
    diagonal included) for the rows that are not usable"""
    q, qc = np.asarray(q, dtype=np.float64), np.asarray(q_count, dtype=np.int32)
    n = q.shape[0]
    good = np.flatnonzero(usable(q, qc))
    out = np.full((n, n), np.nan)
    if good.size:
        sub = np.where(np.isfinite(q[good]), q[good], 0.0)
        d = fo.dtw(sub, qc[good], sub, qc[good], band)
        up = np.triu(d, 1)
        full = up + up.T  # (every entry: one value and +0.0)
        out[np.ix_(good, good)] = full
    return out


def check_matrix(D):
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError("a [n, n] matrix")
    if not bool(((D >= 0.0) & (D < np.inf)).all()):
        raise ValueError("the distance matrix holds a NaN, a negative value or an infinity")
    return D


def build(D, kmax):
    """-> (medoids int32 [kmax], gain float64 [kmax])"""
    D = check_matrix(D)
    n = D.shape[0]
    if not 1 <= kmax <= min(n, 4096):
        raise ValueError("kmax")
    medoids, gain = np.zeros(kmax, dtype=np.int32), np.zeros(kmax)
    rows = osum(D)
    m = int(np.argmin(rows))  # (the first of equal values)
    medoids[0], gain[0] = m, rows[m]
    ismed = np.zeros(n, dtype=bool)
    ismed[m] = True
    dmin = D[m].copy()
    for c in range(1, kmax):
        g = osum(np.maximum(dmin[None, :] - D, 0.0))
        cand = np.flatnonzero(~ismed)
        m = int(cand[int(np.argmax(g[cand]))])
        medoids[c], gain[c] = m, g[m]
        ismed[m] = True
        dmin = np.minimum(dmin, D[m])
    return medoids, gain


def assign_rows(D, med):
    n = D.shape[0]
    slot = {int(m): c for c, m in enumerate(med)}
    a = np.zeros(n, dtype=np.int32)
    for i in range(n):
        a[i] = slot[i] if i in slot else int(np.argmin(D[i, med]))
    return a


def cluster_sums(D, assign, k):
    """sums [n, k]: over the members of every cluster, THE ORDER (the other columns contribute nothing)"""
    n = D.shape[0]
    out = np.zeros((n, k))
    for c in range(k):
        out[:, c] = osum(np.where((assign == c)[None, :], D, 0.0))
    return out


def kmedoids(D, medoids, max_iter=50):
    """-> dict: medoids, assign, sums, cost [iters + 1], iters"""
    D = check_matrix(D)
    n = D.shape[0]
    med = np.array(medoids, dtype=np.int32).reshape(-1)
    k = med.size
    if not 1 <= k <= min(n, 4096) or max_iter < 0 or len(set(med.tolist())) != k or med.min() < 0 or med.max() >= n:
        raise ValueError("medoids")
    cost, it = [], 0
    while True:
        a = assign_rows(D, med)
        cost.append(osum(D[np.arange(n), med[a]]))
        sums = cluster_sums(D, a, k)
        if it == max_iter:
            break
        new = med.copy()
        for c in range(k):
            idx = np.flatnonzero(a == c)
            new[c] = idx[int(np.argmin(sums[idx, c]))]
        if (new == med).all():
            break
        med = new
        it += 1
    return {"medoids": med, "assign": a, "sums": sums, "cost": np.asarray(cost, dtype=np.float64), "iters": it}


def silhouette(D, assign, k):
    D = check_matrix(D)
    n = D.shape[0]
    a_ = np.asarray(assign, dtype=np.int32).reshape(-1)
    if a_.size != n or not 1 <= k <= min(n, 4096) or a_.min() < 0 or a_.max() >= k:
        raise ValueError("assign")
    size = np.bincount(a_, minlength=k)
    if (size == 0).any():
        raise ValueError("a cluster without a member")
    sums = cluster_sums(D, a_, k)
    sil = np.zeros(n)
    for i in range(n):
        own = int(a_[i])
        if k == 1 or size[own] == 1:
            continue
        a = sums[i, own] / np.float64(size[own] - 1)
        b = min(sums[i, c] / np.float64(size[c]) for c in range(k) if c != own)
        mx = max(a, b)
        sil[i] = 0.0 if mx == 0.0 else (b - a) / mx
    return sil


class OracleEngine:
    """the methods of adapted_amd.lib.Engine that adapted_amd/clusters.py calls, on the oracle; a "device pointer" is a key of
    ``mem``"""

    def __init__(self):
        self.mem, self.next, self.freed, self.pairwise_calls = {}, 1000, [], 0

    def dev_alloc(self, nbytes):
        self.next += 1
        self.mem[self.next] = None
        return self.next

    def dev_free(self, ptr):
        del self.mem[ptr]
        self.freed.append(ptr)

    def _d(self, dist):
        return self.mem[dist] if isinstance(dist, int) else dist

    def dtw_pairwise(self, q, q_count, band=0, n=None, E=None, out_ptr=None):
        self.pairwise_calls += 1
        d = pairwise(q, q_count, band)
        if out_ptr is None:
            return d
        self.mem[out_ptr] = d
        return None

    def kmedoids_build(self, dist, kmax, n=None):
        return build(self._d(dist), int(kmax))

    def kmedoids(self, dist, medoids, max_iter=50, n=None, want_sums=False):
        r = kmedoids(self._d(dist), medoids, int(max_iter))
        if not want_sums:
            r["sums"] = None
        return r

    def silhouette(self, dist, assign, k, n=None):
        return silhouette(self._d(dist), assign, int(k))

    def dtw_assign(self, q, q_count, t, t_count, band=0, nq=None, Eq=None, want_dist=True):
        d = fo.dtw(q, q_count, t, t_count, band)
        best, bd = fo.assign(d)
        return (d if want_dist else None), best, bd
