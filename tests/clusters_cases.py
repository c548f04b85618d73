"""Inputs shared by tests/test_clusters_cpu.py and the GPU tests of the clustering: the planted set, ragged fingerprints with
unusable rows, distance matrices with duplicates, and a fake run directory of fingerprints_<k>.npz files."""
import numpy as np

E_PLANTED = 48


def planted(seed=20240611, protos=4, events=40, per=30, noise=0.05, edits=3):
    """``protos`` prototypes of ``events`` events; ``per`` members each: the prototype with ``edits`` events duplicated or dropped
    and small noise; members of the prototypes interleaved in a fixed shuffled order -> (fp [n, E_PLANTED] NaN beyond the counts,
    counts int32 [n], truth int [n])"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((protos, events)) * 2.0
    rows, truth = [], []
    for p in range(protos):
        for _ in range(per):
            x = list(base[p])
            for _e in range(edits):
                at = int(rng.integers(0, len(x)))
                if rng.random() < 0.5:
                    x.insert(at, x[at])
                else:
                    x.pop(at)
            x = np.asarray(x) + noise * rng.standard_normal(len(x))
            rows.append(x)
            truth.append(p)
    order = rng.permutation(len(rows))
    fp = np.full((len(rows), E_PLANTED), np.nan)
    counts = np.zeros(len(rows), dtype=np.int32)
    for at, o in enumerate(order):
        fp[at, :rows[o].size] = rows[o]
        counts[at] = rows[o].size
    return fp, counts, np.asarray(truth)[order]


def same_partition(a, b):
    """do the labelings a and b name the same groups?"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def ragged(n, E, seed, low=1, unusable=True):
    """n fingerprints of width E with counts ragged from ``low`` to E (zeros beyond the counts), and -- with n >= 5 and
    ``unusable`` -- one row of each unusable kind: a count of 0, a count above E, a NaN and an infinity inside the count
    -> (q, counts, usable bool [n])"""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, E))
    counts = rng.integers(low, E + 1, n).astype(np.int32)
    counts[0] = E
    if n > 1:
        counts[1] = low
    for p in range(n):
        q[p, :counts[p]] = rng.standard_normal(counts[p])
    ok = np.ones(n, dtype=bool)
    if unusable and n >= 5:
        counts[n // 2] = 0
        counts[n - 1] = E + 1
        p = 2
        counts[p] = max(counts[p], 1)
        q[p, counts[p] - 1] = np.nan
        p = n - 2
        counts[p] = max(counts[p], 1)
        q[p, 0] = np.inf
        ok[[n // 2, n - 1, 2, n - 2]] = False
    return q, counts, ok


def points_matrix(n, seed, duplicates=True, integer=False):
    """a symmetric distance matrix of n points in the plane (squared distances), a few points repeated to the bit"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 40, (n, 2)).astype(np.float64) if integer else rng.standard_normal((n, 2)) * 3.0
    if duplicates and n >= 4:
        x[n - 1] = x[0]
        x[n // 2] = x[1]
        x[n // 3] = x[1]
    d = x[:, None, :] - x[None, :, :]
    D = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]
    assert (D == D.T).all() and (np.diag(D) == 0.0).all()
    return D


def write_run(tmp_path, fp, counts, cut=None, name="run"):
    """a run directory with two fingerprint files -> (its path, the read ids)"""
    d = tmp_path / name / "fingerprints"
    d.mkdir(parents=True)
    ids = np.asarray(["read_%04d" % i for i in range(len(counts))])
    cut = len(counts) // 3 if cut is None else cut
    for k, sl in ((0, slice(0, cut)), (1, slice(cut, None))):
        np.savez(d / ("fingerprints_%d.npz" % k), read_id=ids[sl], count=counts[sl], status=np.zeros(len(counts[sl]), dtype=np.int32),
                 lengths=np.zeros(fp[sl].shape, dtype=np.int32), levels=fp[sl], fingerprints=fp[sl])
    return str(tmp_path / name), ids
