"""Barcode clusters without labels, found on the GPU (an extension, beside adapted_amd/barcode_templates.py: that one builds
templates from labelled fingerprints, this one finds the groups first).

``dtw_pairwise`` is the symmetric all-pairs DTW matrix of a set of fingerprints (adp_dtw_pairwise, include/adapted_hip_clusters.h:
every pair once, adp_dtw_assign's bits); ``kmedoids_build`` is PAM's BUILD, ``kmedoids`` alternating k-medoids and ``silhouette``
the silhouette of an assignment, each on a host matrix or on one that stayed on the device.  ``discover_clusters`` samples the
usable fingerprints, builds the matrix once on the device, sweeps K and keeps the K of the greatest mean silhouette;
``clusters_command`` is ``adapted clusters``: it labels every fingerprint by its nearest medoid, refines the medoids by DBA and
writes a template file ``adapted detect --barcode_templates`` reads.

Untuned, nothing validated on real data: whether fingerprints of real barcodes separate is what the silhouette lets a user find
out, NOT something this module claims.
"""
from __future__ import annotations

import csv
import os

import numpy as np

from . import lib
from .barcode_templates import _fingerprint_file, _fingerprint_files, _usable, dba_templates
from .fingerprint import Templates, _sequences, assign_barcodes


class DeviceMatrix:
    """a float64 [n, n] matrix in device memory: ``ptr``, ``n``; ``free()`` gives it back to its engine"""

    def __init__(self, engine, ptr: int, n: int):
        self.engine, self.ptr, self.n = engine, int(ptr), int(n)

    def free(self):
        if self.ptr:
            self.engine.dev_free(self.ptr)
            self.ptr = 0


def _eng(device, engine):
    if engine is not None:
        return engine
    from .detect._rows import _engine

    return _engine(device)


def _matrix(dist, n):
    """a host matrix, a DeviceMatrix, or a device pointer with ``n`` -> what the engine's methods take"""
    if isinstance(dist, DeviceMatrix):
        return dist.ptr, dist.n
    if isinstance(dist, int):
        if n is None:
            raise ValueError("a device pointer needs n")
        return dist, int(n)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1] or not 1 <= dist.shape[0] <= lib.CLUSTER_MAX_ROWS:
        raise ValueError("distances: a float64 [n, n] array, 1 <= n <= %d" % lib.CLUSTER_MAX_ROWS)
    return dist, dist.shape[0]


def dtw_pairwise(fp, counts, band: int = 0, device=0, engine=None, out_device: bool = False):
    """The DTW distance of every fingerprint (fp float64 [n, E], its first counts[p] entries) to every other -> float64 [n, n],
    symmetric to the bit with a +0.0 diagonal: dtw_distances(fp, counts, fp, counts)'s values, every pair computed once; NaN rows
    and columns for the fingerprints that are not usable.  ``out_device``: the matrix stays on the device -> a DeviceMatrix."""
    if int(band) < 0:
        raise ValueError("band must be >= 0")
    fp, counts = _sequences(fp, counts, "fingerprints")
    n = fp.shape[0]
    if not 1 <= n <= lib.CLUSTER_MAX_ROWS:
        raise ValueError("1 to %d fingerprints" % lib.CLUSTER_MAX_ROWS)
    eng = _eng(device, engine)
    if not out_device:
        return eng.dtw_pairwise(fp, counts, int(band))
    m = DeviceMatrix(eng, eng.dev_alloc(n * n * 8), n)
    try:
        eng.dtw_pairwise(fp, counts, int(band), out_ptr=m.ptr)
    except Exception:
        m.free()
        raise
    return m


def kmedoids_build(dist, kmax: int, n=None, device=0, engine=None):
    """PAM's BUILD -> (medoids int32 [kmax], gain float64 [kmax]); the first K medoids are BUILD's answer for every K <= kmax"""
    dist, n = _matrix(dist, n)
    if not 1 <= int(kmax) <= min(n, lib.CLUSTER_MAX_K):
        raise ValueError("kmax must lie in [1, min(n, %d)]" % lib.CLUSTER_MAX_K)
    return _eng(device, engine).kmedoids_build(dist, int(kmax), n=n)


def kmedoids(dist, medoids, max_iter: int = 50, n=None, device=0, engine=None, want_sums: bool = False) -> dict:
    """Alternating k-medoids from ``medoids`` (k different rows) -> a dict: medoids int32 [k], assign int32 [n], sums float64 [n, k]
    with ``want_sums``, cost float64 [iters + 1] (before each update and at the end), iters"""
    dist, n = _matrix(dist, n)
    med = np.asarray(medoids, dtype=np.int64).reshape(-1)
    if not 1 <= med.size <= min(n, lib.CLUSTER_MAX_K) or med.min() < 0 or med.max() >= n or len(set(med.tolist())) != med.size:
        raise ValueError("medoids: 1 to min(n, %d) different rows" % lib.CLUSTER_MAX_K)
    if int(max_iter) < 0:
        raise ValueError("max_iter must be >= 0")
    return _eng(device, engine).kmedoids(dist, med.astype(np.int32), int(max_iter), n=n, want_sums=want_sums)


def silhouette(dist, assign, k: int, n=None, device=0, engine=None) -> np.ndarray:
    """The silhouette float64 [n] of every row under ``assign`` (values in [0, k), no cluster empty); scikit-learn's conventions"""
    dist, n = _matrix(dist, n)
    assign = np.ascontiguousarray(assign, dtype=np.int32).reshape(-1)
    if assign.size != n or not 1 <= int(k) <= min(n, lib.CLUSTER_MAX_K) or assign.min() < 0 or assign.max() >= int(k):
        raise ValueError("assign: one cluster in [0, k) per row, 1 <= k <= min(n, %d)" % lib.CLUSTER_MAX_K)
    if (np.bincount(assign, minlength=int(k)) == 0).any():
        raise ValueError("a cluster without a member")
    return _eng(device, engine).silhouette(dist, assign, int(k), n=n)


def _k_range(k):
    kmin, kmax = (k, k) if isinstance(k, (int, np.integer)) else k
    kmin, kmax = int(kmin), int(kmax)
    if kmin < 1:
        raise ValueError("k must be >= 1")
    if kmax < kmin:
        raise ValueError("kmax must be >= kmin")
    if kmax > lib.CLUSTER_MAX_K:
        raise ValueError("k must be <= %d" % lib.CLUSTER_MAX_K)
    return kmin, kmax


def _check_options(sample, band, iters):
    if not 2 <= int(sample) <= lib.CLUSTER_MAX_ROWS:
        raise ValueError("sample must lie in [2, %d]" % lib.CLUSTER_MAX_ROWS)
    if int(band) < 0:
        raise ValueError("band must be >= 0")
    if int(iters) < 0:
        raise ValueError("iters must be >= 0")


def discover_clusters(fingerprints, counts, k, sample: int = 4096, band: int = 0, iters: int = 50, device=0, engine=None):
    """Clusters of fingerprints by their DTW distances -> (Templates, info).  ``k``: the number of clusters, or (kmin, kmax).

    The usable fingerprints (barcode_templates' rule) are sampled as dba_templates samples: S = min(sample, usable) members,
    idx[(s * len) // S].  Their matrix is built once and stays on the device; BUILD runs once, to kmax; for every K alternating
    k-medoids runs from BUILD's first K medoids, then the silhouette.  The K of the greatest mean silhouette is chosen, the lowest
    K on exact ties.  The templates are the medoids' fingerprints, named cluster_000, cluster_001, ...
    info: "k"; "medoid_index" int64 [k] (into ``fingerprints``); "sizes" int32 [k] and "silhouette_mean" float64 [k] (of the sample
    members of every cluster); "sweep" float64 [Ks, 4] (K, final cost, mean silhouette, iterations); "assign" int32 [S] and
    "silhouette" float64 [S] of the sample members; "sample_index" int64 [S]."""
    fp, counts = _sequences(fingerprints, counts, "fingerprints")
    kmin, kmax = _k_range(k)
    _check_options(sample, band, iters)
    idx = np.flatnonzero(_usable(fp, counts))
    if kmax > idx.size:
        raise ValueError("k (%d) is above the number of usable fingerprints (%d)" % (kmax, idx.size))
    S = min(int(sample), idx.size)
    sample_index = np.asarray([int(idx[(s * idx.size) // S]) for s in range(S)], dtype=np.int64)
    q = np.where(np.isfinite(fp[sample_index]), fp[sample_index], 0.0)  # (beyond the counts: not read)
    qc = np.ascontiguousarray(counts[sample_index], dtype=np.int32)
    eng = _eng(device, engine)
    ptr = eng.dev_alloc(S * S * 8)
    try:
        eng.dtw_pairwise(q, qc, int(band), out_ptr=ptr)
        start, _gain = eng.kmedoids_build(ptr, kmax, n=S)
        sweep, best = [], None
        for K in range(kmin, kmax + 1):
            r = eng.kmedoids(ptr, np.asarray(start[:K], dtype=np.int32), int(iters), n=S)
            sil = eng.silhouette(ptr, r["assign"], K, n=S)
            mean = float(np.mean(sil))
            sweep.append((float(K), float(r["cost"][-1]), mean, float(r["iters"])))
            if best is None or mean > best[1]:
                best = (K, mean, r, sil)
    finally:
        eng.dev_free(ptr)
    K, _mean, r, sil = best
    med = sample_index[np.asarray(r["medoids"], dtype=np.int64)]
    levels = np.full((K, fp.shape[1]), np.nan)
    for c, p in enumerate(med):
        levels[c, :counts[p]] = fp[p, :counts[p]]
    assign = np.asarray(r["assign"], dtype=np.int32)
    info = {"k": K, "medoid_index": med, "sizes": np.bincount(assign, minlength=K).astype(np.int32),
            "silhouette_mean": np.asarray([float(np.mean(sil[assign == c])) for c in range(K)], dtype=np.float64),
            "sweep": np.asarray(sweep, dtype=np.float64).reshape(-1, 4), "assign": assign, "silhouette": np.asarray(sil, dtype=np.float64),
            "sample_index": sample_index}
    return Templates(["cluster_%03d" % c for c in range(K)], levels, counts[med].astype(np.int32)), info


def read_fingerprints(paths):
    """The fingerprints of `adapted detect --fingerprints`, in file order -> (read ids [n] of str, fingerprints float64 [n, E],
    counts int32 [n]).  paths: as barcode_templates.labelled_fingerprints takes them"""
    ids, fps, cnts = [], [], []
    for f in _fingerprint_files(paths):
        i, fp, c = _fingerprint_file(f, fps[0].shape[1] if fps else None)
        ids.extend(i)
        fps.append(fp)
        cnts.append(c)
    return np.asarray(ids, dtype=str), np.concatenate(fps), np.concatenate(cnts)


def add_arguments(t):
    """the options of `adapted clusters` on its sub-parser"""
    t.add_argument("-f", "--fingerprints", type=str, nargs="+", required=True, metavar="RUN_DIR|FILE.npz",
                   help="a run directory of `adapted detect --fingerprints`, or fingerprints_<k>.npz files")
    t.add_argument("-o", "--output", type=str, required=True, metavar="OUT.npz", help="the template file (for detect --barcode_templates)")
    t.add_argument("-k", "--clusters", type=str, required=True, metavar="K|KMIN:KMAX",
                   help="the number of clusters, or a range: the K of the greatest mean silhouette is chosen")
    t.add_argument("--sample", type=int, default=4096, help="fingerprints the clusters are found on (2 .. 16384; default 4096)")
    t.add_argument("--iters", type=int, default=50, help="the most k-medoids updates per K (default 50)")
    t.add_argument("--dtw_band", type=int, default=0, metavar="R", help="the DTW's band (default 0: none)")
    t.add_argument("--refine", type=str, choices=["dba", "none"], default="dba",
                   help="dba: DTW barycentre averaging over every fingerprint's cluster (default); none: the medoids themselves")
    t.add_argument("--dba_iters", type=int, default=10, help="the most DBA iterations (default 10)")
    t.add_argument("--assignments", type=str, default=None, metavar="FILE.csv", help="write every fingerprint's cluster and distances here")
    t.add_argument("--device", type=int, default=0, help="GPU index (default 0)")


def _parse_k(text):
    parts = str(text).split(":")
    try:
        vals = [int(p) for p in parts]
    except ValueError:
        vals = []
    if len(vals) not in (1, 2):
        raise SystemExit("-k: a number K, or a range KMIN:KMAX.")
    return vals[0], vals[-1]


def _num(v) -> str:
    return "" if v is None or (isinstance(v, float) and np.isnan(v)) else repr(float(v))


def clusters_command(args, engine=None, align=None) -> dict:
    """`adapted clusters`: everything that can be refused is, with a message, before a GPU is touched -> a report: "k", "sweep",
    "names", "fingerprints", "usable".  ``engine`` / ``align``: in place of the GPU (tests), as discover_clusters and dba_templates
    take them"""
    kmin, kmax = _parse_k(args.clusters)
    if kmin < 1:
        raise SystemExit("-k: K must be >= 1.")
    if kmax < kmin:
        raise SystemExit("-k: KMAX must be >= KMIN.")
    if kmax > lib.CLUSTER_MAX_K:
        raise SystemExit("-k: at most %d clusters." % lib.CLUSTER_MAX_K)
    if not 2 <= args.sample <= lib.CLUSTER_MAX_ROWS:
        raise SystemExit("--sample must lie in [2, %d]." % lib.CLUSTER_MAX_ROWS)
    if args.iters < 0:
        raise SystemExit("--iters must be >= 0.")
    if args.dba_iters < 0:
        raise SystemExit("--dba_iters must be >= 0.")
    if args.dtw_band < 0:
        raise SystemExit("--dtw_band must be >= 0.")
    if args.device < 0:
        raise SystemExit("--device must be >= 0.")
    for what, path in (("--output", args.output), ("--assignments", args.assignments)):
        if path is not None and not os.path.isdir(os.path.dirname(os.path.abspath(path))):
            raise SystemExit("%s: no directory %s." % (what, os.path.dirname(os.path.abspath(path))))
    for p in args.fingerprints:
        if not os.path.exists(p):
            raise SystemExit("--fingerprints: %s does not exist." % p)
    try:
        ids, fp, counts = read_fingerprints(args.fingerprints)
    except ValueError as e:
        raise SystemExit("adapted clusters: %s." % e)
    if not 1 <= fp.shape[1] <= lib.FINGERPRINT_MAX_EVENTS:
        raise SystemExit("adapted clusters: fingerprints of 1 to %d events are needed." % lib.FINGERPRINT_MAX_EVENTS)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    usable = _usable(fp, counts)
    if kmax > int(usable.sum()):
        raise SystemExit("-k: %d clusters of %d usable fingerprints (of %d)." % (kmax, int(usable.sum()), fp.shape[0]))
    templates, info = discover_clusters(fp, counts, (kmin, kmax), sample=args.sample, band=args.dtw_band, iters=args.iters,
                                        device=args.device, engine=engine)
    K = info["k"]
    # every usable fingerprint to its nearest medoid
    use = np.flatnonzero(usable)
    q = np.where(np.isfinite(fp[use]), fp[use], 0.0)
    near = assign_barcodes(q, counts[use], templates, band=args.dtw_band, device=args.device, engine=engine)
    labels = np.asarray([templates.names[b] for b in near.best], dtype=str)
    members = np.bincount(near.best, minlength=K).astype(np.int32)
    built = {"members": members, "inertia": np.zeros((0, K)), "iterations": 0}
    if args.refine == "dba":
        # (a medoid that equals one of a lower slot to the bit has no member here: then dba_templates has fewer labels)
        templates, built = dba_templates(fp[use], counts[use], labels, band=args.dtw_band, iters=args.dba_iters, device=args.device,
                                         engine=engine, align=align)
    lv = np.array(templates.levels, dtype=np.float64)
    tc = np.asarray(templates.counts, dtype=np.int32).reshape(-1)
    for c in range(lv.shape[0]):
        lv[c, tc[c]:] = np.nan
    with open(args.output, "wb") as fh:  # (save_built_templates' keys, and what the discovery found)
        np.savez(fh, names=np.asarray([str(s) for s in templates.names]), levels=lv, counts=tc,
                 method=np.asarray("clusters+dba" if args.refine == "dba" else "clusters"), band=np.asarray(int(args.dtw_band), dtype=np.int32),
                 members=np.asarray(built["members"], dtype=np.int32), inertia=np.asarray(built["inertia"], dtype=np.float64),
                 iterations=np.asarray(int(built["iterations"]), dtype=np.int32), medoid_read_id=ids[info["medoid_index"]],
                 sizes=info["sizes"], silhouette=info["silhouette_mean"], sweep=info["sweep"])
    if args.assignments is not None:
        in_sample = {int(p): s for s, p in enumerate(info["sample_index"])}
        at = {int(p): u for u, p in enumerate(use)}
        with open(args.assignments, "w", newline="") as fh:
            wr = csv.writer(fh)
            wr.writerow(["read_id", "cluster", "dtw_dist", "cluster_second", "dtw_dist_second", "dtw_margin", "in_sample", "silhouette"])
            for p in range(fp.shape[0]):
                u = at.get(p)
                if u is None:
                    wr.writerow([ids[p], "", "", "", "", "", 0, ""])
                    continue
                b2 = int(near.second[u])
                s = in_sample.get(p)
                wr.writerow([ids[p], "cluster_%03d" % int(near.best[u]), _num(float(near.dist[u])), "" if b2 < 0 else "cluster_%03d" % b2,
                             _num(float(near.dist_second[u])), _num(float(near.margin[u])), int(s is not None),
                             "" if s is None else _num(float(info["silhouette"][s]))])
    print("    K          cost  silhouette  iterations")
    for row in info["sweep"]:
        print("%5d  %12.6g  %10.6f  %10d%s" % (int(row[0]), row[1], row[2], int(row[3]), "  <-" if int(row[0]) == K else ""))
    print("{} clusters of {} usable fingerprints (of {}; {} sampled) saved to {} ({})".format(
        K, use.size, fp.shape[0], info["sample_index"].size, args.output, "refined by DBA, %d iterations" % built["iterations"]
        if args.refine == "dba" else "the medoids"))
    return {"k": K, "sweep": info["sweep"], "names": list(templates.names), "fingerprints": int(fp.shape[0]), "usable": int(use.size),
            "info": info}


__all__ = ["DeviceMatrix", "dtw_pairwise", "kmedoids_build", "kmedoids", "silhouette", "discover_clusters", "read_fingerprints",
           "clusters_command"]
