"""Barcode templates from labelled adapter fingerprints, built on the GPU (an extension, the step between ``adapted detect
--fingerprints`` and ``adapted detect --barcode_templates``; adapted_amd/fingerprint.py holds the fingerprints, the templates' file
format and their use).

``dtw_align`` gives, for every fingerprint and ONE template each, the DTW distance and the warping path as a run of fingerprint
positions per template position (adp_dtw_align, include/adapted_hip_templates.h); ``dba_step`` is one iteration of DTW barycentre
averaging, DBA: every member is aligned to its label's template and every template position becomes the mean of what landed on it
(adp_dba_step, wholly on the device).  ``dba_templates`` starts from the medoid of a sample of every label and iterates;
``labelled_fingerprints`` reads a run's fingerprint files and joins them with a CSV of labels; ``templates_command`` is
``adapted templates``.

Nothing here is TUNED and no real pod5 data has been through any of this: whether such templates separate real barcodes is NOT
claimed.
"""
from __future__ import annotations

import csv
import os
import re

import numpy as np

from . import lib
from .fingerprint import Templates, _sequences, _templates, medoid_templates


def _inputs(q, q_count, which, t, t_count, band):
    if int(band) < 0:
        raise ValueError("band must be >= 0")
    q, q_count = _sequences(q, q_count, "queries")
    t, t_count = _templates(t, t_count)
    which = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
    if which.size != q.shape[0]:
        raise ValueError("which: one template (or -1) per query")
    if which.size and (which.min() < -1 or which.max() >= t.shape[0]):
        raise ValueError("which must lie in [-1, the number of templates)")
    return q, q_count, which, t, t_count


def dtw_align(q, q_count, which, t, t_count, band: int = 0, device=0, engine=None) -> dict:
    """Every query (q float64 [nq, Eq], its first q_count[p] entries) against the template which[p] (t [nt, Et], t_count; -1: the
    query is skipped) -> a dict: dist float64 [nq] (dtw_distances' value of that pair), status int32 [nq] (0; 1 a query that is not
    usable; 2 a distance that is not finite; 3 skipped), lo / hi int32 [nq, Et] (the first and the last query position aligned to
    every template position; -1 where there is none) and sum float64 [nq, Et] (the query summed over that run)"""
    q, q_count, which, t, t_count = _inputs(q, q_count, which, t, t_count, band)
    if engine is None:
        from .detect._rows import _engine

        engine = _engine(device)
    return engine.dtw_align(q, q_count, which, t, t_count, int(band))


def dba_step(q, q_count, which, t, t_count, band: int = 0, device=0, engine=None):
    """One DBA iteration -> (t_new float64 [nt, Et], NaN at and beyond the counts; members int32 [nt]: the usable queries of every
    template; inertia float64 [nt]: their distances to the OLD template added up).  A template without a member keeps its values."""
    q, q_count, which, t, t_count = _inputs(q, q_count, which, t, t_count, band)
    if engine is None:
        from .detect._rows import _engine

        engine = _engine(device)
    return engine.dba_step(q, q_count, which, t, t_count, int(band))[:3]


def step_from_alignment(r: dict, which, t, t_count):
    """adp_dba_step's reduction in numpy from dtw_align's answer ``r``: the members of a template in ascending order, one add each
    (np.cumsum's order) -> (t_new, members, inertia)"""
    t = np.asarray(t, dtype=np.float64)
    which = np.asarray(which).reshape(-1)
    nt, Et = t.shape
    t_new, members, inertia = np.full((nt, Et), np.nan), np.zeros(nt, dtype=np.int32), np.zeros(nt)
    for k in range(nt):
        m = int(t_count[k])
        idx = np.flatnonzero((which == k) & (np.asarray(r["status"]) == 0))
        members[k] = idx.size
        if idx.size == 0:
            t_new[k, :m] = t[k, :m]
            continue
        T = np.cumsum(np.concatenate([np.zeros((1, m)), r["sum"][idx, :m]]), axis=0)[-1]
        N = (r["hi"][idx, :m].astype(np.int64) - r["lo"][idx, :m] + 1).sum(axis=0)
        t_new[k, :m] = T / N.astype(np.float64)
        inertia[k] = np.cumsum(np.concatenate([[0.0], r["dist"][idx]]))[-1]
    return t_new, members, inertia


def _usable(fp, counts):
    return np.asarray([1 <= counts[p] <= fp.shape[1] and bool(np.isfinite(fp[p, :counts[p]]).all()) for p in range(fp.shape[0])],
                      dtype=bool).reshape(-1)


def _same_bits(a, b) -> bool:
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def dba_templates(fingerprints, counts, labels, band: int = 0, iters: int = 10, init_sample: int = 256, device=0, engine=None, align=None):
    """Templates by DTW barycentre averaging -> (Templates, info).

    Members whose fingerprint is not usable (a count outside [1, E], a value that is not finite inside it) are left out, as
    medoid_templates leaves them out; a label without a usable member is an error.  Per label, in sorted order: the start is the
    medoid (medoid_templates' rule) of S = min(init_sample, usable members) members spread evenly over the usable ones in index
    order -- member (s * len) // S for s in range(S); 1 <= init_sample <= 4096.  Its count is the template's length for good.
    Then up to ``iters`` DBA steps (dba_step) over all usable members, with the fingerprints uploaded once; a step that changes
    no bit of any template is the last.  info: "members" int32 [nt] (the last step's; the usable members without a step),
    "inertia" float64 [iterations, nt] (per step the members' distances to the template the step STARTED from, added up) and
    "iterations" (the steps made).
    ``align``: a function of dtw_align's first six arguments with its answer, in place of the GPU (tests): the medoids' distances
    and the steps are then made from it."""
    fp, counts = _sequences(fingerprints, counts, "fingerprints")
    labels = np.asarray(labels).reshape(-1)
    if labels.size != fp.shape[0]:
        raise ValueError("one label per fingerprint")
    if int(band) < 0:
        raise ValueError("band must be >= 0")
    if int(iters) < 0:
        raise ValueError("iters must be >= 0")
    if not 1 <= int(init_sample) <= lib.DTW_MAX_TEMPLATES:
        raise ValueError("init_sample must lie in [1, %d]" % lib.DTW_MAX_TEMPLATES)
    band, iters, S0 = int(band), int(iters), int(init_sample)
    usable = _usable(fp, counts)
    names = sorted(set(labels.tolist()))
    which = np.full(fp.shape[0], -1, dtype=np.int32)
    sample = []
    for k, lab in enumerate(names):
        idx = np.flatnonzero((labels == lab) & usable)
        if idx.size == 0:
            raise ValueError("label %r has no usable fingerprint" % (lab,))
        which[idx] = k
        S = min(S0, idx.size)
        sample.extend(int(idx[(s * idx.size) // S]) for s in range(S))
    sample = np.asarray(sample, dtype=np.int64)
    if engine is None and align is None:
        from .detect._rows import _engine

        engine = _engine(device)

    def pair_distances(q, qc, t, tc, band):  # (dtw_distances from ``align``: every query against every template)
        nq, nt = q.shape[0], t.shape[0]
        r = align(np.repeat(q, nt, axis=0), np.repeat(qc, nt), np.tile(np.arange(nt, dtype=np.int32), nq), t, tc, band)
        return np.asarray(r["dist"]).reshape(nq, nt)

    start = medoid_templates(fp[sample], counts[sample], labels[sample], band, device=device, engine=engine,
                             distances=pair_distances if align is not None else None)
    t_count = np.asarray(start.counts, dtype=np.int32)
    t = np.where(np.isnan(start.levels), 0.0, start.levels)
    members = np.asarray([int((which == k).sum()) for k in range(len(names))], dtype=np.int32)
    inertia = []
    q = fp  # (beyond the counts: not read; the members that are not usable: skipped, which is -1)
    dq = dqc = None
    try:
        if align is None and iters > 0:
            dq, dqc = engine.dev_alloc(q.nbytes), engine.dev_alloc(counts.nbytes)
            engine.h2d(dq, q)
            engine.h2d(dqc, counts)
        for _ in range(iters):
            if align is None:
                t_new, members, inert, _d = engine.dba_step(dq, dqc, which, t, t_count, band, nq=q.shape[0], Eq=q.shape[1])
            else:
                t_new, members, inert = step_from_alignment(align(q, counts, which, t, t_count, band), which, t, t_count)
            inertia.append(np.asarray(inert, dtype=np.float64))
            t_new = np.where(np.isnan(t_new), 0.0, t_new)
            done = _same_bits(t_new, t)
            t = t_new
            if done:
                break
    finally:
        if dq is not None:
            engine.dev_free(dq)
        if dqc is not None:
            engine.dev_free(dqc)
    levels = np.full(t.shape, np.nan)
    for k in range(t.shape[0]):
        levels[k, :t_count[k]] = t[k, :t_count[k]]
    info = {"members": np.asarray(members, dtype=np.int32), "inertia": np.asarray(inertia, dtype=np.float64).reshape(len(inertia), len(names)),
            "iterations": len(inertia)}
    return Templates([str(s) for s in names], levels, t_count), info


def _fingerprint_files(paths):
    """fingerprints_<k>.npz files in the order given; a directory stands for those of its fingerprints/ folder (or its own), by k"""
    out = []
    for p in [paths] if isinstance(paths, (str, os.PathLike)) else list(paths):
        p = os.fspath(p)
        if os.path.isdir(p):
            d = os.path.join(p, "fingerprints") if os.path.isdir(os.path.join(p, "fingerprints")) else p
            found = []
            for f in os.listdir(d):
                mt = re.fullmatch(r"fingerprints_(\d+)\.npz", f)
                if mt:
                    found.append((int(mt.group(1)), os.path.join(d, f)))
            if not found:
                raise ValueError("no fingerprints_<k>.npz files in %s" % d)
            out.extend(f for _, f in sorted(found))
        else:
            out.append(p)
    if not out:
        raise ValueError("no fingerprint files given")
    return out


def _fingerprint_file(f, width=None):
    """one fingerprints_<k>.npz, checked -> (read ids, fingerprints float64 [n, E], counts int32 [n]); ``width``: the E of the files
    before it.  ValueError: not such a file, or another width"""
    try:
        with np.load(f, allow_pickle=False) as z:
            ids, fp, c = [str(s) for s in z["read_id"]], np.asarray(z["fingerprints"], dtype=np.float64), np.asarray(z["count"], dtype=np.int32)
    except (OSError, KeyError, ValueError, EOFError) as e:
        raise ValueError("not a fingerprint file (%s): %s" % (f, e)) from e
    if fp.ndim != 2 or c.shape != (fp.shape[0],) or len(ids) != fp.shape[0]:
        raise ValueError("not a fingerprint file (%s): read_id [n], count [n] and fingerprints [n, E] are needed" % f)
    if width is not None and fp.shape[1] != width:
        raise ValueError("fingerprint files of different widths (%d, %d in %s)" % (width, fp.shape[1], f))
    return ids, fp, c


def read_labels(labels_csv, read_id_col: str = "read_id", label_col: str = "barcode") -> dict:
    """read id -> label from a CSV with a header; rows with an empty label are left out.  ValueError: a file that cannot be read,
    a column that is not there"""
    try:
        with open(labels_csv, newline="") as fh:
            rd = csv.reader(fh)
            header = next(rd, None)
            if header is None:
                raise ValueError("labels file %s is empty" % labels_csv)
            for col in (read_id_col, label_col):
                if col not in header:
                    raise ValueError("labels file %s has no column %r" % (labels_csv, col))
            ci, cl = header.index(read_id_col), header.index(label_col)
            return {row[ci]: row[cl] for row in rd if len(row) > max(ci, cl) and row[cl] != ""}
    except (OSError, UnicodeDecodeError, csv.Error) as e:
        raise ValueError("labels file %s cannot be read: %s" % (labels_csv, e)) from e


def labelled_fingerprints(paths, labels_csv, read_id_col: str = "read_id", label_col: str = "barcode"):
    """The fingerprints of `adapted detect --fingerprints` with their labels -> (fingerprints float64 [n, E], counts int32 [n],
    labels [n] of str, report).  paths: fingerprints_<k>.npz files, or a run directory (its fingerprints/ folder); labels_csv: a CSV
    with a read id and a label per line.  Only reads that have a label are returned, in file order; report: "fingerprints" (read),
    "unlabelled" (of them without a label), "labels_without_fingerprint" (lines of the CSV whose read has no fingerprint)."""
    label_of = read_labels(labels_csv, read_id_col, label_col)
    fps, cnts, labs, seen, total = [], [], [], set(), 0
    for f in _fingerprint_files(paths):
        ids, fp, c = _fingerprint_file(f, fps[0].shape[1] if fps else None)
        keep = [i for i, rid in enumerate(ids) if rid in label_of]
        total += len(ids)
        seen.update(ids[i] for i in keep)
        fps.append(fp[keep])
        cnts.append(c[keep])
        labs.extend(label_of[ids[i]] for i in keep)
    fp, c = np.concatenate(fps), np.concatenate(cnts)
    report = {"fingerprints": total, "unlabelled": total - fp.shape[0], "labels_without_fingerprint": len(set(label_of) - seen)}
    return fp, c, np.asarray(labs, dtype=str), report


def save_built_templates(path, templates: Templates, method: str, band: int, info: dict):
    """save_templates' file (load_templates and --barcode_templates take it) with what built it: method, band, members [nt], inertia
    [iterations, nt] and iterations"""
    lv = np.array(templates.levels, dtype=np.float64)
    counts = np.asarray(templates.counts, dtype=np.int32).reshape(-1)
    for k in range(lv.shape[0]):
        lv[k, counts[k]:] = np.nan
    with open(path, "wb") as fh:
        np.savez(fh, names=np.asarray([str(s) for s in templates.names]), levels=lv, counts=counts, method=np.asarray(str(method)),
                 band=np.asarray(int(band), dtype=np.int32), members=np.asarray(info["members"], dtype=np.int32),
                 inertia=np.asarray(info["inertia"], dtype=np.float64), iterations=np.asarray(int(info["iterations"]), dtype=np.int32))


def add_arguments(t):
    """the options of `adapted templates` on its sub-parser"""
    t.add_argument("-f", "--fingerprints", type=str, nargs="+", required=True, metavar="RUN_DIR|FILE.npz",
                   help="a run directory of `adapted detect --fingerprints`, or fingerprints_<k>.npz files")
    t.add_argument("-l", "--labels", type=str, required=True, metavar="LABELS.csv", help="a CSV with a read id and a label per line")
    t.add_argument("-o", "--output", type=str, required=True, metavar="OUT.npz", help="the template file (for detect --barcode_templates)")
    t.add_argument("--method", type=str, choices=["dba", "medoid"], default="dba",
                   help="dba: DTW barycentre averaging from the sampled medoid (default); medoid: the sampled medoid alone")
    t.add_argument("--iters", type=int, default=10, help="the most DBA iterations (default 10)")
    t.add_argument("--init_sample", type=int, default=256, help="members per label the starting medoid is chosen from (1 .. 4096; default 256)")
    t.add_argument("--dtw_band", type=int, default=0, metavar="R", help="the DTW's band (default 0: none)")
    t.add_argument("--read_id_colname", type=str, default="read_id")
    t.add_argument("--label_colname", type=str, default="barcode")
    t.add_argument("--device", type=int, default=0, help="GPU index (default 0)")


def templates_command(args, align=None) -> dict:
    """`adapted templates`: everything that can be refused is, with a message, before a GPU is touched -> the report of
    labelled_fingerprints with "labels" (the templates' names)"""
    if args.iters < 0:
        raise SystemExit("--iters must be >= 0.")
    if not 1 <= args.init_sample <= lib.DTW_MAX_TEMPLATES:
        raise SystemExit("--init_sample must lie in [1, %d]." % lib.DTW_MAX_TEMPLATES)
    if args.dtw_band < 0:
        raise SystemExit("--dtw_band must be >= 0.")
    if args.device < 0:
        raise SystemExit("--device must be >= 0.")
    out_dir = os.path.dirname(os.path.abspath(args.output))
    if not os.path.isdir(out_dir):
        raise SystemExit("--output: no directory %s." % out_dir)
    for p in args.fingerprints:
        if not os.path.exists(p):
            raise SystemExit("--fingerprints: %s does not exist." % p)
    try:
        fp, counts, labels, report = labelled_fingerprints(args.fingerprints, args.labels, args.read_id_colname, args.label_colname)
    except ValueError as e:
        raise SystemExit("adapted templates: %s." % e)
    if fp.shape[0] == 0:
        raise SystemExit("adapted templates: none of the %d fingerprints has a label in %s." % (report["fingerprints"], args.labels))
    if not 1 <= fp.shape[1] <= lib.FINGERPRINT_MAX_EVENTS:
        raise SystemExit("adapted templates: fingerprints of 1 to %d events are needed." % lib.FINGERPRINT_MAX_EVENTS)
    names = sorted(set(labels.tolist()))
    if len(names) > lib.DTW_MAX_TEMPLATES:
        raise SystemExit("adapted templates: at most %d labels." % lib.DTW_MAX_TEMPLATES)
    usable = _usable(fp, np.asarray(counts, dtype=np.int32))
    for lab in names:
        if not usable[labels == lab].any():
            raise SystemExit("adapted templates: label %r has no usable fingerprint." % lab)
    iters = args.iters if args.method == "dba" else 0
    templates, info = dba_templates(fp, counts, labels, band=args.dtw_band, iters=iters, init_sample=args.init_sample, device=args.device, align=align)
    save_built_templates(args.output, templates, args.method, args.dtw_band, info)
    print("Templates of {} labels from {} labelled fingerprints saved to {} ({}, {} iterations; {} fingerprints without a label, {} labels "
          "without a fingerprint)".format(len(names), fp.shape[0], args.output, args.method, info["iterations"], report["unlabelled"],
                                          report["labels_without_fingerprint"]))
    report["labels"] = templates.names
    return report


__all__ = ["dtw_align", "dba_step", "dba_templates", "labelled_fingerprints", "templates_command"]
