"""adp_dtw_knn (include/adapted_hip_knn.h), adapted_amd.knn.vote and leave_one_out in numpy: their exact oracle.  The distances are
fingerprint_oracle.dtw's -- adp_dtw_assign's, bit for bit --; the k nearest are taken by np.lexsort((index, dist)); nothing is
abandoned here, which is the point: the device's answer with pruning must be this one."""
import numpy as np

import fingerprint_oracle as fo

same = fo.same


def topk(D, k, exclude=None):
    """a distance matrix [nq, nr] (NaN rows: unusable queries) -> (idx int32 [nq, k], dist float64 [nq, k]): per row the k least of
    (D[p, j], j), j != exclude[p], ascending; -1 and NaN where there are fewer, and in a NaN row"""
    D = np.asarray(D, dtype=np.float64)
    nq, nr = D.shape
    idx, dist = np.full((nq, k), -1, dtype=np.int32), np.full((nq, k), np.nan)
    for p in range(nq):
        if np.isnan(D[p]).any():
            continue
        cand = np.asarray([j for j in range(nr) if exclude is None or j != int(exclude[p])], dtype=np.int64)
        if cand.size == 0:
            continue
        order = cand[np.lexsort((cand, D[p, cand]))][:k]
        idx[p, :order.size] = order
        dist[p, :order.size] = D[p, order]
    return idx, dist


def knn(q, qc, r, rc, k, band=0, exclude=None):
    return topk(fo.dtw(q, qc, r, rc, band), k, exclude)


def candidates(q, qc, nr, exclude=None):
    """the pairs of every query that count: nr, less the excluded one; 0 for an unusable query"""
    q, qc = np.asarray(q, dtype=np.float64), np.asarray(qc)
    good = np.asarray([1 <= qc[p] <= q.shape[1] and bool(np.isfinite(q[p, :qc[p]]).all()) for p in range(q.shape[0])], dtype=bool).reshape(-1)
    c = np.full(q.shape[0], nr, dtype=np.int64)
    if exclude is not None:
        c -= (np.asarray(exclude) >= 0).astype(np.int64)
    return np.where(good, c, 0)


def full_steps(q, qc, rc, Er, exclude=None):
    """the DP steps of every query when no pair is abandoned: n + (m - 1) // C over its candidates, C the least of 1, 2, 4, 8 that
    is >= ceil(Er / 64)"""
    C = next(c for c in (1, 2, 4, 8) if c * 64 >= Er)
    rc = np.asarray(rc, dtype=np.int64)
    cand = candidates(q, qc, rc.size, exclude)
    out = np.zeros(len(qc), dtype=np.int64)
    for p in range(len(qc)):
        if cand[p] == 0:
            continue
        keep = np.ones(rc.size, dtype=bool)
        if exclude is not None and exclude[p] >= 0:
            keep[int(exclude[p])] = False
        out[p] = int((int(qc[p]) + (rc[keep] - 1) // C).sum())
    return out


def vote(idx, dist, ref_labels):
    """-> per query (label, votes, dist, second label, its votes, its dist, nearest); None / 0 / NaN / -1 where there is none"""
    out = []
    for p in range(len(idx)):
        seen = []  # [label, votes, first t]
        for t, j in enumerate(idx[p]):
            if j < 0:
                continue
            lab = str(ref_labels[j])
            hit = [s for s in seen if s[0] == lab]
            if hit:
                hit[0][1] += 1
            else:
                seen.append([lab, 1, t])
        seen.sort(key=lambda s: (-s[1], s[2]))
        a = (seen[0][0], seen[0][1], float(dist[p][seen[0][2]])) if seen else (None, 0, np.nan)
        b = (seen[1][0], seen[1][1], float(dist[p][seen[1][2]])) if len(seen) > 1 else (None, 0, np.nan)
        out.append(a + b + (int(idx[p][0]) if seen else -1,))
    return out


def usable(fp, counts):
    return np.asarray([1 <= counts[p] <= fp.shape[1] and bool(np.isfinite(fp[p, :counts[p]]).all()) for p in range(fp.shape[0])],
                      dtype=bool).reshape(-1)


def leave_one_out(fp, counts, labels, k, band=0):
    """-> (names, confusion int64 [labels, labels] true by predicted, accuracy) over the usable members"""
    fp, counts, labels = np.asarray(fp, dtype=np.float64), np.asarray(counts), np.asarray(labels)
    use = np.flatnonzero(usable(fp, counts))
    sub = np.where(np.isfinite(fp[use]), fp[use], 0.0)
    idx, dist = knn(sub, counts[use], sub, counts[use], k, band, exclude=np.arange(use.size))
    names = sorted(set(str(s) for s in labels[use]))
    conf = np.zeros((len(names), len(names)), dtype=np.int64)
    for true, v in zip(labels[use], vote(idx, dist, labels[use])):
        conf[names.index(str(true)), names.index(v[0])] += 1
    return names, conf, float(np.trace(conf)) / use.size


class OracleEngine:
    """Engine.dtw_knn on the oracle, in place of the GPU"""

    def __init__(self):
        self.calls = []

    def dtw_knn(self, q, q_count, r, r_count, k, band=0, exclude=None, prune=True, n=None, E=None, want_work=False):
        self.calls.append({"nq": len(q_count), "nr": len(r_count), "k": k, "band": band, "prune": prune,
                           "exclude": None if exclude is None else np.array(exclude)})
        idx, dist = knn(q, q_count, r, r_count, k, band, exclude)
        if not want_work:
            return idx, dist
        work = np.zeros((len(q_count), 3), dtype=np.int64)
        work[:, 0] = candidates(q, q_count, len(r_count), exclude)
        work[:, 2] = full_steps(q, q_count, r_count, np.asarray(r).shape[1], exclude)
        return idx, dist, work
