"""`adapted events`: the adapter events, poly(A) lengths and fingerprints of a FINISHED run (an extension, as
adapted_amd/polya_length.py and adapted_amd/fingerprint.py are).

`adapted detect --polya_length / --fingerprints` segments every passing read's adapter while the read's whole preload window is
resident on the GPU, so a second setting of --event_params or of the fingerprint width costs a second detection.  This command
takes a run's detected_boundaries_<k>.csv files and the input files instead: it cuts ``[adapter_start, adapter_end)`` out of
every read of the run, packs the slices back to back -- float32 pA, or with --int16_ingest the raw int16 ADC samples with the
read's calibration --, runs the packed forms of the two event calls on them (adp_event_levels_packed /
adp_segment_events_packed, include/adapted_hip_events_packed.h) and writes the files detect would have put beside each CSV,
through detect's own record builders and writers (adapted_amd/main.py).  It also serves the runs detect cannot extend: those made
with --int16_ingest or on several ranks.

The event parameters are UNTUNED, chosen on synthetic staircases, and no real pod5 data has been through any of this.  The
int16 calibration's parity with pod5's own ``signal_pa`` is unpinned.
"""
from __future__ import annotations

import argparse
import csv
import json
import logging
import os
import re
import sys
import time
import types
from typing import List, Optional

import numpy as np

from . import lib, parallel

CSV_COLUMNS = ("read_id", "adapter_start", "adapter_end", "adapter_len", "polya_end", "polya_len", "polya_truncated")
BATCH_SAMPLES = 1 << 24  # samples of one batch of slices in the pinned staging (a longer slice is a batch of its own)
BATCH_SLICES = 16384  # slices of one batch


def add_arguments(t):
    """the options of `adapted events` on its sub-parser"""
    t.add_argument("run_dir", type=str, metavar="RUN_DIR", help="a finished run of `adapted detect`: its boundaries/detected_boundaries_<k>.csv are read")
    t.add_argument("-i", "--input", type=str, nargs="+", required=True, help="the run's input files / directories (.pod5 or .npz bundles)")
    t.add_argument("-o", "--output", type=str, required=True, metavar="OUT_DIR", help="where polya_length/ and fingerprints/ go (may be RUN_DIR)")
    t.add_argument("--polya_length", type=str, choices=["events", "adapter"], default=None, help="as detect's: polya_length/polya_length_<k>.csv")
    t.add_argument("--adapter_nt", type=float, default=None, help="the adapter's length in bases (--polya_length adapter)")
    t.add_argument("--fingerprints", type=int, default=None, metavar="E", help="as detect's: fingerprints/fingerprints_<k>.npz")
    t.add_argument("--barcode_templates", type=str, default=None, metavar="FILE.npz", help="(with --fingerprints) as detect's: fingerprints/barcodes_<k>.csv")
    t.add_argument("--dtw_band", type=int, default=None, metavar="R", help="(with --barcode_templates) the DTW's band (default 0: none)")
    t.add_argument("--event_params", type=str, default=None, metavar="WINDOW,MIN_DISTANCE,THRESHOLD",
                   help="the event segmentation's parameters (default 8,8,16.0: untuned, chosen on synthetic signals)")
    t.add_argument("--int16_ingest", action="store_true",
                   help="move the slices as raw int16 ADC samples with each read's calibration and compute pA on the GPU "
                        "(pA = scale * (float32(adc) + offset)); .pod5 inputs or .npz bundles with raw/scale/offset")
    t.add_argument("--force", action="store_true", help="overwrite output files that exist")
    t.add_argument("--device", type=int, default=0, help="GPU index (default 0)")


class RunFile:
    """one detected_boundaries_<k>.csv: its read ids in file order, what polya_length_records reads of every read's DetectResults
    (``results``: adapter_start None where the file has none), the adapter slices' bounds (an empty adapter_start counts as 0, an
    empty adapter_end as 0: no slice), and, while the file is in flight, its reads' events and fingerprints"""

    def __init__(self, k: int, path: str, ids: List[str], results: list):
        self.k, self.path, self.ids, self.results = k, path, ids, results
        self.starts = np.asarray([r.adapter_start or 0 for r in results], dtype=np.int64)
        self.ends = np.asarray([r.adapter_end or 0 for r in results], dtype=np.int64)
        self.seen = np.zeros(len(ids), dtype=bool)
        self.ev = self.fp = None


def _integer(text: str) -> Optional[int]:
    """a CSV cell of an integer column (pandas prints 610.0 where the column has an empty cell)"""
    return None if text == "" else int(float(text))


def read_run_file(k: int, path: str) -> RunFile:
    """a detected_boundaries_<k>.csv -> its RunFile; ValueError names a column it lacks"""
    with open(path, newline="") as fh:
        rd = csv.reader(fh)
        header = next(rd, None) or []
        missing = [c for c in CSV_COLUMNS if c not in header]
        if missing:
            raise ValueError("%s has no column %s" % (path, ", ".join(missing)))
        at = {c: header.index(c) for c in CSV_COLUMNS}
        ids, results = [], []
        for row in rd:
            if not row:
                continue
            cell = {c: row[j] if j < len(row) else "" for c, j in at.items()}
            ids.append(cell["read_id"])
            results.append(types.SimpleNamespace(
                adapter_start=_integer(cell["adapter_start"]), adapter_end=_integer(cell["adapter_end"]),
                adapter_len=_integer(cell["adapter_len"]), polya_end=_integer(cell["polya_end"]), polya_len=_integer(cell["polya_len"]),
                polya_truncated={"True": True, "False": False}.get(cell["polya_truncated"])))
    return RunFile(k, path, ids, results)


def file_records(rf: RunFile, ev, fp, method: Optional[str] = None, adapter_nt=None, names=None):
    """the records of one file from its reads' events (the pipeline's EVENT_DTYPE array) and fingerprints (its
    AdapterFingerprints), through detect's builders -> (polya_length_records or None, fingerprint_records or None)"""
    from .main import fingerprint_records, polya_length_records

    return (polya_length_records(rf.ids, rf.results, ev, method, adapter_nt) if method else None,
            fingerprint_records(rf.ids, fp, names) if fp is not None else None)


def find_run_files(run_dir: str):
    """[(k, path)] of RUN_DIR/boundaries/detected_boundaries_<k>.csv in the order of k; SystemExit where there is none"""
    where = os.path.join(run_dir, "boundaries")
    if not os.path.isdir(where):
        raise SystemExit("adapted events: %s has no boundaries/ directory: not a run of `adapted detect`." % run_dir)
    found = []
    for f in os.listdir(where):
        mt = re.fullmatch(r"detected_boundaries_(\d+)\.csv", f)
        if mt:
            found.append((int(mt.group(1)), os.path.join(where, f)))
    if not found:
        raise SystemExit("adapted events: no detected_boundaries_<k>.csv in %s." % where)
    return sorted(found)


def _outputs(out_dir: str, k: int, args):
    paths = []
    if args.polya_length:
        paths.append(os.path.join(out_dir, "polya_length", "polya_length_%d.csv" % k))
    if args.fingerprints is not None:
        paths.append(os.path.join(out_dir, "fingerprints", "fingerprints_%d.npz" % k))
        if args.barcode_templates:
            paths.append(os.path.join(out_dir, "fingerprints", "barcodes_%d.csv" % k))
    return paths


def check_arguments(args):
    """everything that is refused before a GPU is touched and before anything is created -> (the RunFiles, the input files, the
    templates of --barcode_templates or None)"""
    from .io_utils import input_to_filelist
    from .main import _check_fingerprints, _check_polya_length

    if not args.polya_length and args.fingerprints is None:
        raise SystemExit("adapted events: give --polya_length, --fingerprints or both.")
    if parallel.world()[1] > 1:
        raise SystemExit("adapted events runs on one GPU (WORLD_SIZE is %d): the slices are small, and nothing is gathered from several "
                         "ranks." % parallel.world()[1])
    if args.device < 0:
        raise SystemExit("--device must be >= 0.")
    # detect's own option rules, apart from the two this command lifts (int16 ingestion; the primary: the run is finished)
    rules = argparse.Namespace(**dict(vars(args), int16_ingest=False, config=None, chemistry=None))
    _check_polya_length(rules)
    templates = _check_fingerprints(rules)
    found = find_run_files(args.run_dir)
    try:
        run = [read_run_file(k, path) for k, path in found]
    except ValueError as e:
        raise SystemExit("adapted events: %s." % e)
    files = input_to_filelist(args.input)
    if not files:
        raise SystemExit("adapted events: no valid input files found in %s." % " ".join(args.input))
    if not args.force:
        exist = [p for rf in run for p in _outputs(args.output, rf.k, args)] + [os.path.join(args.output, "events_command.json")]
        exist = [p for p in exist if os.path.exists(p)]
        if exist:
            raise SystemExit("adapted events: %s exists (%d output file(s) do): --force overwrites." % (exist[0], len(exist)))
    return run, files, templates


class _Batch:
    """slices packed back to back in pinned staging, with where each belongs: (file, index) and, for raw samples, its calibration"""

    def __init__(self, eng, dtype):
        self.eng, self.dtype, self.buf = eng, np.dtype(dtype), None
        self.clear()

    def clear(self):
        self.offsets, self.where, self.scale, self.offset = [0], [], [], []

    def room(self, n: int) -> bool:
        return not self.where or (self.offsets[-1] + n <= BATCH_SAMPLES and len(self.where) < BATCH_SLICES)

    def add(self, x: np.ndarray, where, scale=0.0, offset=0.0):
        a, n = self.offsets[-1], int(x.size)
        if self.buf is None or a + n > self.buf.size:  # (the first batch, or one slice longer than a batch)
            new = self.eng.host_alloc((max(BATCH_SAMPLES, a + n),), self.dtype)
            if self.buf is not None:
                new[:a] = self.buf[:a]
                self.eng.host_free(self.buf)
            self.buf = new
        self.buf[a:a + n] = x  # (the one copy of the slice; other dtypes become the staging's here, as detect's staging does)
        self.offsets.append(a + n)
        self.where.append(where)
        self.scale.append(scale)
        self.offset.append(offset)

    def close(self):
        if self.buf is not None:
            self.eng.host_free(self.buf)
            self.buf = None


def events_command(args, engine=None) -> dict:
    """`adapted events` -> a report: "reads", "samples", "files" written, "missing" reads.  ``engine``: in place of the GPU's
    (tests)"""
    from .fingerprint import FingerprintParams, template_arrays
    from .io_utils import _iter_reads, _iter_reads_i16
    from .main import write_fingerprint_files, write_polya_length_file
    from .pipeline import AdapterFingerprints, HostPipeline
    from .polya_length import EventParams

    run, files, templates = check_arguments(args)
    i16, method, want_fp = bool(args.int16_ingest), args.polya_length, args.fingerprints is not None
    events = EventParams.parse(args.event_params) if args.event_params else EventParams()
    E, band = int(args.fingerprints or 0), int(args.dtw_band or 0)
    if want_fp:
        FingerprintParams(E, events, band).check()
    ev_args = events.args()
    tm = template_arrays(templates) if templates is not None else None
    names = templates.names if templates is not None else None
    out_dir = args.output
    for sub in (["polya_length"] if method else []) + (["fingerprints"] if want_fp else []):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    with open(os.path.join(out_dir, "events_command.json"), "w") as fh:
        json.dump(vars(args), fh, indent=2)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s", handlers=[logging.StreamHandler(sys.stdout)])
    logging.info("adapted events: %d file(s) of %s, %d read(s)", len(run), args.run_dir, sum(len(rf.ids) for rf in run))
    where = {}  # read id -> [(file, index)]: the reads still to find
    for f, rf in enumerate(run):
        for i, rid in enumerate(rf.ids):
            where.setdefault(rid, []).append((f, i))
    if engine is None:
        from .detect._rows import _engine

        engine = _engine(args.device)
    eng = engine
    batch = _Batch(eng, np.int16 if i16 else np.float32)
    fp_dev = None  # (fingerprints and counts of a batch, on the device between the two calls)
    t0 = time.time()
    total = {"reads": 0, "samples": 0, "files": 0}

    def begin(rf: RunFile):
        n = len(rf.ids)
        rf.ev = HostPipeline._no_events(n)
        rf.fp = AdapterFingerprints(n, E, tm is not None) if want_fp else None

    def finish(rf: RunFile):
        """file k's last read is done: its records through detect's builders and writers, then nothing of it stays"""
        pl, fr = file_records(rf, rf.ev, rf.fp, method, args.adapter_nt, names)
        if pl is not None:
            write_polya_length_file(os.path.join(out_dir, "polya_length"), rf.k, pl)
        if fr is not None:
            write_fingerprint_files(os.path.join(out_dir, "fingerprints"), rf.k, fr, E, tm is not None)
        rf.ev = rf.fp = None
        total["files"] += 1

    def flush():
        nonlocal fp_dev
        ns = len(batch.where)
        if ns == 0:
            return
        offsets = np.asarray(batch.offsets, dtype=np.int64)
        packed = batch.buf[:max(int(offsets[-1]), 1)]
        cal = dict(scale=np.asarray(batch.scale, dtype=np.float32), offset=np.asarray(batch.offset, dtype=np.float32)) if i16 else {}
        fa, ia = (np.asarray(v, dtype=np.int64) for v in zip(*batch.where))
        if want_fp:
            dev = {}
            if tm is not None:
                if fp_dev is None:
                    fp_dev = (eng.dev_alloc(BATCH_SLICES * E * 8), eng.dev_alloc(BATCH_SLICES * 4))
                dev = dict(fp_ptr=fp_dev[0], count_ptr=fp_dev[1])
            r = eng.event_levels_packed(packed, offsets, ev_args, E, **cal, **dev)
            if tm is not None:  # (as the pipeline does: the fingerprints stay on the device for the DTW)
                _, best, bestdist = eng.dtw_assign(fp_dev[0], fp_dev[1], tm[0], tm[1], band, nq=ns, Eq=E, want_dist=False)
                r["fingerprints"], r["count"] = np.zeros((ns, E)), np.zeros(ns, dtype=np.int32)
                eng.d2h(r["fingerprints"], fp_dev[0])
                eng.d2h(r["count"], fp_dev[1])
            info, stats = r["info"], r["stats"]
        else:
            _, info, stats = eng.segment_events_packed(packed, offsets, ev_args, cap=0, **cal)
        for f in np.unique(fa):
            rf, sel = run[int(f)], fa == f
            idx = ia[sel]
            rf.ev["n_bound"][idx], rf.ev["status"][idx] = info[sel, 0], info[sel, 1]
            rf.ev["med"][idx], rf.ev["mad"][idx] = stats[sel, 0], stats[sel, 1]
            if want_fp:
                for key in ("count", "status", "lengths", "levels", "fingerprints"):
                    getattr(rf.fp, key)[idx] = r[key][sel]
                if tm is not None:
                    rf.fp.best[idx], rf.fp.bestdist[idx] = best[sel], bestdist[sel]
            rf.seen[idx] = True
            if rf.seen.all():
                finish(rf)
        total["reads"] += ns
        total["samples"] += int(offsets[-1])
        batch.clear()

    try:
        for filename in files:
            if not where:
                break
            selection = list(where)
            try:
                reads = _iter_reads_i16(filename, selection) if i16 else _iter_reads(filename, selection)
                for read in reads:
                    rid, n_samples, get = read[0], read[1], read[2]
                    targets = where.pop(rid, None)
                    if targets is None:  # (not of the run, or decoded already)
                        continue
                    sig = np.asarray(get()).reshape(-1)
                    for f, i in targets:
                        rf = run[f]
                        if rf.ev is None:
                            begin(rf)
                        end = min(int(rf.ends[i]), int(n_samples), sig.size)
                        x = sig[min(int(rf.starts[i]), end):end]
                        if not batch.room(x.size):
                            flush()
                        batch.add(x, (f, i), *((read[3], read[4]) if i16 else ()))
            except ValueError as e:  # (_iter_reads_i16: an input without raw samples)
                raise SystemExit("adapted events: %s." % e)
        flush()
    finally:
        batch.close()
        if fp_dev is not None:
            for ptr in fp_dev:
                eng.dev_free(ptr)
    for rf in run:  # (a file without reads has its empty files all the same)
        if not rf.ids and rf.ev is None:
            begin(rf)
            finish(rf)
    dt = max(time.time() - t0, 1e-9)
    missing = [(rf, np.flatnonzero(~rf.seen)) for rf in run if not rf.seen.all()]
    for rf, idx in missing:
        logging.error("%s: %d read(s) are not in the input, the first %s: nothing is written for this file", rf.path, idx.size, rf.ids[int(idx[0])])
    logging.info("Processed %d reads, %d adapter samples in %.2f s (%.0f reads/s)", total["reads"], total["samples"], dt, total["reads"] / dt)
    report = dict(total, missing=int(sum(idx.size for _, idx in missing)))
    if missing:
        rf, idx = missing[0]
        raise SystemExit("adapted events: %d read(s) of the run are not in the input, the first %s (%s): nothing is written for %d file(s)."
                         % (report["missing"], rf.ids[int(idx[0])], os.path.basename(rf.path), len(missing)))
    return report
