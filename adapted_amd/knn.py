"""Barcodes by the k nearest labelled fingerprints, found on the GPU (an extension, beside adapted_amd/barcode_templates.py and
adapted_amd/clusters.py: those keep one averaged sequence per label, this one keeps the labelled reads themselves).

``dtw_knn`` is the k nearest references of every query under DTW (adp_dtw_knn, include/adapted_hip_knn.h: adp_dtw_assign's distance
to the bit, no distance matrix, up to 262144 references, pairs abandoned behind a lower bound without a bit of the answer
changing); ``vote`` turns the neighbours' labels into a barcode; ``knn_barcodes`` is both; ``leave_one_out`` classifies every
labelled fingerprint with itself excluded and reports how often it gets its own label back; ``knn_command`` is ``adapted knn``.

Untuned, nothing validated on real data: whether fingerprints of real barcodes separate is what the leave-one-out accuracy lets a
user find out, NOT something this module claims.
"""
from __future__ import annotations

import csv
import json
import logging
import os
from dataclasses import dataclass

import numpy as np

from . import lib
from .barcode_templates import _fingerprint_file, _fingerprint_files, _usable, read_labels
from .fingerprint import _sequences


def _eng(device, engine):
    if engine is not None:
        return engine
    from .detect._rows import _engine

    return _engine(device)


def _references(r, r_count):
    r, r_count = _sequences(r, r_count, "references")
    if not 1 <= r.shape[0] <= lib.KNN_NR_MAX:
        raise ValueError("1 to %d references" % lib.KNN_NR_MAX)
    if r_count.min() < 1 or r_count.max() > r.shape[1]:
        raise ValueError("every reference needs 1 <= count <= its width")
    if not _usable(r, r_count).all():
        raise ValueError("reference values inside their count must be finite")
    return np.where(np.isfinite(r), r, 0.0), r_count  # (beyond the counts: not read)


def dtw_knn(q, q_count, r, r_count, k: int = 5, band: int = 0, exclude=None, prune: bool = True, device=0, engine=None,
            want_work: bool = False):
    """The k nearest references (r float64 [nr, Er], the first r_count[j] entries of each) of every query (q [nq, Eq], q_count) under
    dtw_distances' distance -> (idx int32 [nq, k], dist float64 [nq, k][, work int64 [nq, 3]]): ascending in (distance, index); -1 and
    NaN where a query has fewer candidates, and for a query that is not usable.  ``exclude`` int [nq]: the reference that does not
    count for a query, -1 for none.  ``prune=False``: no pair is abandoned (the same answer).  work: pairs finished, pairs abandoned,
    DP steps -- a diagnostic."""
    if not 1 <= int(k) <= lib.KNN_KMAX:
        raise ValueError("k must lie in [1, %d]" % lib.KNN_KMAX)
    if int(band) < 0:
        raise ValueError("band must be >= 0")
    q, q_count = _sequences(q, q_count, "queries")
    r, r_count = _references(r, r_count)
    if exclude is not None:
        exclude = np.ascontiguousarray(exclude, dtype=np.int32).reshape(-1)
        if exclude.size != q.shape[0] or (exclude.size and (exclude.min() < -1 or exclude.max() >= r.shape[0])):
            raise ValueError("exclude: one reference in [-1, nr) per query")
    return _eng(device, engine).dtw_knn(q, q_count, r, r_count, int(k), int(band), exclude=exclude, prune=bool(prune), want_work=want_work)


@dataclass
class KnnAssignment:
    """one entry per query.  label / label_second: the winning label and the next (None: none); votes / votes_second int32: their
    neighbours (0: none); dtw_dist / dtw_dist_second float64: the distance of the nearest neighbour of that label (NaN: none);
    nearest int32: the nearest neighbour (-1: none); idx / dist: the neighbours the vote was taken on"""
    label: np.ndarray
    votes: np.ndarray
    dtw_dist: np.ndarray
    label_second: np.ndarray
    votes_second: np.ndarray
    dtw_dist_second: np.ndarray
    nearest: np.ndarray
    idx: np.ndarray
    dist: np.ndarray


def vote(idx, dist, ref_labels) -> KnnAssignment:
    """The labels of dtw_knn's neighbours to one barcode per query, in numpy on the host.  The valid neighbours t = 0 .. c - 1 in the
    order the call returns them; votes[L] = how many carry label L, first[L] = the least such t.  The winner is the label of the
    greatest (votes[L], -first[L]) -- the most votes, and among equals the one whose nearest member is nearer --, the second is the
    next label in that order.  A label's dtw_dist is dist[first[L]]."""
    idx, dist = np.asarray(idx), np.asarray(dist, dtype=np.float64)
    ref_labels = np.asarray(ref_labels).reshape(-1)
    nq = idx.shape[0]
    out = KnnAssignment(np.full(nq, None, dtype=object), np.zeros(nq, dtype=np.int32), np.full(nq, np.nan), np.full(nq, None, dtype=object),
                        np.zeros(nq, dtype=np.int32), np.full(nq, np.nan), np.full(nq, -1, dtype=np.int32), idx, dist)
    for p in range(nq):
        votes, first = {}, {}
        for t in range(idx.shape[1]):
            if idx[p, t] < 0:
                break
            lab = str(ref_labels[idx[p, t]])
            votes[lab] = votes.get(lab, 0) + 1
            first.setdefault(lab, t)
        order = sorted(votes, key=lambda lab: (-votes[lab], first[lab]))
        if order:
            out.label[p], out.votes[p], out.dtw_dist[p], out.nearest[p] = order[0], votes[order[0]], dist[p, first[order[0]]], idx[p, 0]
        if len(order) > 1:
            out.label_second[p], out.votes_second[p], out.dtw_dist_second[p] = order[1], votes[order[1]], dist[p, first[order[1]]]
    return out


def knn_barcodes(fp, counts, ref_fp, ref_counts, ref_labels, k: int = 5, band: int = 0, exclude=None, prune: bool = True, device=0,
                 engine=None, want_work: bool = False):
    """Every fingerprint's barcode by the vote of its k nearest references -> KnnAssignment (with ``want_work`` a pair: it and
    dtw_knn's work).  A fingerprint that is not usable gets no label."""
    ref_labels = np.asarray(ref_labels).reshape(-1)
    if ref_labels.size != np.asarray(ref_counts).size:
        raise ValueError("one label per reference")
    r = dtw_knn(fp, counts, ref_fp, ref_counts, k, band, exclude=exclude, prune=prune, device=device, engine=engine, want_work=want_work)
    a = vote(r[0], r[1], ref_labels)
    return (a, r[2]) if want_work else a


def leave_one_out(fp, counts, labels, k: int = 5, band: int = 0, prune: bool = True, device=0, engine=None) -> dict:
    """How often a labelled fingerprint gets its own label back from the others: every usable member (barcode_templates' rule) is
    classified by knn_barcodes against all usable members with itself excluded -> a dict: "names" (the labels, sorted), "k", "n" (the
    members classified), "accuracy", "labels" (per name "n", "recall", "precision"; None where there is nothing to divide by),
    "confusion" int64 [labels, labels] (true by predicted), "predicted" (per member), "index" (the members' rows in ``fp``) and
    "work" (dtw_knn's, summed: pairs finished, pairs abandoned, DP steps)."""
    fp, counts = _sequences(fp, counts, "fingerprints")
    labels = np.asarray(labels).reshape(-1)
    if labels.size != fp.shape[0]:
        raise ValueError("one label per fingerprint")
    use = np.flatnonzero(_usable(fp, counts))
    if use.size < int(k) + 1:
        raise ValueError("k + 1 = %d usable fingerprints are needed (there are %d)" % (int(k) + 1, use.size))
    a, work = knn_barcodes(fp[use], counts[use], fp[use], counts[use], labels[use], k, band, exclude=np.arange(use.size, dtype=np.int32),
                           prune=prune, device=device, engine=engine, want_work=True)
    names = sorted(set(str(s) for s in labels[use].tolist()))
    at = {s: i for i, s in enumerate(names)}
    conf = np.zeros((len(names), len(names)), dtype=np.int64)
    for true, pred in zip(labels[use].tolist(), a.label.tolist()):
        conf[at[str(true)], at[pred]] += 1
    rows, cols, hit = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    return {"names": names, "k": int(k), "n": int(use.size), "accuracy": float(hit.sum()) / float(use.size),
            "labels": {s: {"n": int(rows[i]), "recall": float(hit[i]) / float(rows[i]) if rows[i] else None,
                           "precision": float(hit[i]) / float(cols[i]) if cols[i] else None} for i, s in enumerate(names)},
            "confusion": conf, "predicted": a.label, "index": use, "work": np.asarray(work, dtype=np.int64).sum(axis=0)}


def per_label_spread(labels, per_label: int) -> np.ndarray:
    """The rows that stay when at most ``per_label`` members of every label may (0: all): of a label's L members in row order the
    members (s * L) // S for s < S = min(per_label, L) -- dba_templates' spread --; ascending"""
    labels = np.asarray(labels).reshape(-1)
    if per_label <= 0:
        return np.arange(labels.size, dtype=np.int64)
    keep = []
    for lab in sorted(set(labels.tolist())):
        idx = np.flatnonzero(labels == lab)
        S = min(int(per_label), idx.size)
        keep.extend(int(idx[(s * idx.size) // S]) for s in range(S))
    return np.asarray(sorted(keep), dtype=np.int64)


def labelled_reference(paths, labels_csv, read_id_col: str = "read_id", label_col: str = "barcode"):
    """barcode_templates.labelled_fingerprints' join with the read ids kept -> (read ids [n] of str, fingerprints float64 [n, E],
    counts int32 [n], labels [n] of str, the fingerprints read)"""
    label_of = read_labels(labels_csv, read_id_col, label_col)
    rid, fps, cnts, labs, total = [], [], [], [], 0
    for f in _fingerprint_files(paths):
        ids, fp, c = _fingerprint_file(f, fps[0].shape[1] if fps else None)
        keep = [i for i, r in enumerate(ids) if r in label_of]
        total += len(ids)
        rid.extend(ids[i] for i in keep)
        fps.append(fp[keep])
        cnts.append(c[keep])
        labs.extend(label_of[ids[i]] for i in keep)
    return np.asarray(rid, dtype=str), np.concatenate(fps), np.concatenate(cnts).astype(np.int32), np.asarray(labs, dtype=str), total


def add_arguments(t):
    """the options of `adapted knn` on its sub-parser"""
    t.add_argument("-r", "--reference", type=str, nargs="+", required=True, metavar="RUN_DIR|FILE.npz",
                   help="the labelled reads: a run directory of `adapted detect --fingerprints`, or fingerprints_<k>.npz files")
    t.add_argument("-l", "--labels", type=str, required=True, metavar="LABELS.csv", help="a CSV with a read id and a label per line")
    t.add_argument("-f", "--fingerprints", type=str, nargs="+", default=None, metavar="RUN_DIR|FILE.npz",
                   help="the reads to classify (with -o); a read that is also a reference never votes for itself")
    t.add_argument("-o", "--output", type=str, default=None, metavar="OUT.csv", help="a line per fingerprint of -f")
    t.add_argument("--evaluate", action="store_true", help="leave-one-out on the reference: accuracy, per-label table, confusion matrix")
    t.add_argument("--report", type=str, default=None, metavar="FILE.json", help="(with --evaluate) the same as JSON")
    t.add_argument("-k", "--neighbours", type=int, default=5, metavar="K", help="the neighbours that vote (1 .. 32; default 5)")
    t.add_argument("--per_label", type=int, default=0, metavar="N", help="at most N references per label, spread evenly (default 0: all)")
    t.add_argument("--dtw_band", type=int, default=0, metavar="R", help="the DTW's band (default 0: none)")
    t.add_argument("--no_prune", action="store_true", help="compute every pair to the end (the same answer, slower: a check)")
    t.add_argument("--read_id_colname", type=str, default="read_id")
    t.add_argument("--label_colname", type=str, default="barcode")
    t.add_argument("--device", type=int, default=0, help="GPU index (default 0)")


def _num(v) -> str:
    return "" if v is None or np.isnan(v) else repr(float(v))


def _share(work) -> float:
    pairs = int(work[0]) + int(work[1])
    return float(work[1]) / pairs if pairs else 0.0


def knn_command(args, engine=None) -> dict:
    """`adapted knn`: everything that can be refused is, with a message, before a GPU is touched and with nothing created -> a
    report: "references", "k", with -f "fingerprints", "classified" and "abandoned_share", with --evaluate "evaluation"
    (leave_one_out's dict).  ``engine``: in place of the GPU (tests)"""
    K = args.neighbours
    if not 1 <= K <= lib.KNN_KMAX:
        raise SystemExit("-k: K must lie in [1, %d]." % lib.KNN_KMAX)
    if args.per_label < 0:
        raise SystemExit("--per_label must be >= 0.")
    if args.dtw_band < 0:
        raise SystemExit("--dtw_band must be >= 0.")
    if args.device < 0:
        raise SystemExit("--device must be >= 0.")
    if args.fingerprints is None and not args.evaluate:
        raise SystemExit("adapted knn: give -f with -o, --evaluate, or both.")
    if (args.fingerprints is None) != (args.output is None):
        raise SystemExit("-f and -o go together.")
    if args.report is not None and not args.evaluate:
        raise SystemExit("--report goes with --evaluate.")
    for what, path in (("--output", args.output), ("--report", args.report)):
        if path is not None and not os.path.isdir(os.path.dirname(os.path.abspath(path))):
            raise SystemExit("%s: no directory %s." % (what, os.path.dirname(os.path.abspath(path))))
    for what, paths in (("--reference", args.reference), ("--fingerprints", args.fingerprints or [])):
        for p in paths:
            if not os.path.exists(p):
                raise SystemExit("%s: %s does not exist." % (what, p))
    try:
        rid, rfp, rc, rlab, total = labelled_reference(args.reference, args.labels, args.read_id_colname, args.label_colname)
        ids = fp = counts = None
        if args.fingerprints is not None:
            from .clusters import read_fingerprints

            ids, fp, counts = read_fingerprints(args.fingerprints)
            counts = np.ascontiguousarray(counts, dtype=np.int32)
    except ValueError as e:
        raise SystemExit("adapted knn: %s." % e)
    for what, a in (("reference", rfp), ("query", fp)):
        if a is not None and not 1 <= a.shape[1] <= lib.FINGERPRINT_MAX_EVENTS:
            raise SystemExit("adapted knn: %s fingerprints of 1 to %d events are needed." % (what, lib.FINGERPRINT_MAX_EVENTS))
    use = np.flatnonzero(_usable(rfp, rc))
    if use.size == 0:
        raise SystemExit("adapted knn: none of the %d fingerprints of the reference has a label in %s and is usable." % (total, args.labels))
    use = use[per_label_spread(rlab[use], args.per_label)]
    if use.size > lib.KNN_NR_MAX:
        raise SystemExit("adapted knn: %d references, at most %d are taken: thin them with --per_label." % (use.size, lib.KNN_NR_MAX))
    need = K + 1 if args.evaluate else K
    if use.size < need:
        raise SystemExit("adapted knn: %d usable references, K%s = %d are needed." % (use.size, " + 1" if args.evaluate else "", need))
    rid, rfp, rc, rlab = rid[use], rfp[use], rc[use], rlab[use]
    report = {"references": int(use.size), "k": K, "labels": sorted(set(rlab.tolist()))}
    prune = not args.no_prune
    eng = _eng(args.device, engine)
    if fp is not None:
        first = {}
        for j, s in enumerate(rid.tolist()):
            first.setdefault(s, j)
        exclude = np.asarray([first.get(s, -1) for s in ids.tolist()], dtype=np.int32)  # a read never votes for itself
        a, work = knn_barcodes(fp, counts, rfp, rc, rlab, K, args.dtw_band, exclude=exclude, prune=prune, engine=eng, want_work=True)
        work = np.asarray(work, dtype=np.int64).sum(axis=0)
        with open(args.output, "w", newline="") as fh:
            wr = csv.writer(fh)
            wr.writerow(["read_id", "n_events", "barcode", "votes", "dtw_dist", "barcode_second", "votes_second", "dtw_dist_second",
                         "nearest_read_id"])
            for p in range(fp.shape[0]):
                if a.label[p] is None:
                    wr.writerow([ids[p], int(counts[p]), "", "", "", "", "", "", ""])
                    continue
                two = a.label_second[p] is not None
                wr.writerow([ids[p], int(counts[p]), a.label[p], int(a.votes[p]), _num(a.dtw_dist[p]), a.label_second[p] if two else "",
                             int(a.votes_second[p]) if two else "", _num(a.dtw_dist_second[p]), rid[a.nearest[p]]])
        done = int(sum(lab is not None for lab in a.label))
        report.update(fingerprints=int(fp.shape[0]), classified=done, abandoned_share=_share(work))
        logging.info("adapted knn: %d of %d pairs abandoned (%.1f %%), %d DP steps", int(work[1]), int(work[0]) + int(work[1]),
                     100.0 * _share(work), int(work[2]))
        print("{} of {} fingerprints classified by their {} nearest of {} references, saved to {} ({:.1f} % of the pairs abandoned)".format(
            done, fp.shape[0], K, use.size, args.output, 100.0 * _share(work)))
    if args.evaluate:
        ev = leave_one_out(rfp, rc, rlab, K, args.dtw_band, prune=prune, engine=eng)
        report["evaluation"] = ev
        logging.info("adapted knn --evaluate: %d of %d pairs abandoned (%.1f %%), %d DP steps", int(ev["work"][1]),
                     int(ev["work"][0]) + int(ev["work"][1]), 100.0 * _share(ev["work"]), int(ev["work"][2]))
        print("leave-one-out: K = %d, n = %d, accuracy = %.6f (%.1f %% of the pairs abandoned)" % (K, ev["n"], ev["accuracy"],
                                                                                                 100.0 * _share(ev["work"])))
        wide = max([len("label")] + [len(s) for s in ev["names"]])
        print("%-*s  %8s  %8s  %9s" % (wide, "label", "n", "recall", "precision"))
        for s in ev["names"]:
            row = ev["labels"][s]
            print("%-*s  %8d  %8s  %9s" % (wide, s, row["n"], "" if row["recall"] is None else "%.6f" % row["recall"],
                                          "" if row["precision"] is None else "%.6f" % row["precision"]))
        print("confusion (true by predicted, labels in the order above):")
        for row in ev["confusion"]:
            print(" ".join("%6d" % v for v in row))
        if args.report is not None:
            with open(args.report, "w") as fh:
                json.dump({"k": K, "n": ev["n"], "accuracy": ev["accuracy"], "names": ev["names"], "labels": ev["labels"],
                           "confusion": ev["confusion"].tolist(), "abandoned_share": _share(ev["work"]), "band": int(args.dtw_band),
                           "references": int(use.size)}, fh, indent=1)
                fh.write("\n")
    return report


__all__ = ["KnnAssignment", "dtw_knn", "vote", "knn_barcodes", "leave_one_out", "per_label_spread", "labelled_reference", "knn_command"]
