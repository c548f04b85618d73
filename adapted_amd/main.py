"""`adapted detect` / `adapted continue` on MI355X.

Keeps the reference's command line (adapted/parser.py:37-269), run-directory layout
(adapted_<ver>_<uuid8>/{command.json, config.toml, adapted.log, boundaries/detected_boundaries_<k>.csv,
failed_reads/failed_reads_<k>.csv}) and CSV columns, but replaces the process pool and manager
queues of adapted/file_proc.py:612-823 with: one process per GPU, minibatches streamed into the
GPU engine, rows written in output batches of `-b` reads.  Launch under torchrun for several
GPUs: ranks own contiguous blocks of whole minibatches and rank 0 writes after one gather.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import shutil
import sys
import time
import uuid
from typing import List, Set

import numpy as np
import pandas as pd

from . import lib, parallel
from ._version import __version__
from .config import get_chemistry_specific_config, load_nested_config_from_file
from .container_types import ReadResult
from .io_utils import input_to_filelist, yield_minibatches
from .output import save_detected_boundaries


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="adapted", formatter_class=argparse.RawTextHelpFormatter,
                                description="ADAPTed detect on MI355X: adapter and poly(A) boundaries in raw dRNA-seq signals.")
    sub = p.add_subparsers(dest="mode", required=True)
    d = sub.add_parser("detect", help="Detect adapter and poly(A) signal boundaries and calculate statistics.")
    c = sub.add_parser("continue", help="Continue processing from a previous incomplete run.")
    c.add_argument("continue_from", type=str)
    t = sub.add_parser("truncated", help="(extension) List the reads whose poly(A) was cut off by the preload window "
                                         "(runs made with --flag_truncated), for a rerun with a larger --max_obs_trace.")
    t.add_argument("directory", type=str, help="a run directory, or the directory that holds its detected_boundaries_*.csv files")
    b = sub.add_parser("templates", help="(extension) Build barcode templates from the fingerprints of a run made with --fingerprints "
                                         "and a CSV of labels, for detect --barcode_templates (on the GPU; untuned, nothing validated).")
    from .barcode_templates import add_arguments

    add_arguments(b)
    k = sub.add_parser("clusters", help="(extension) Find barcode clusters in the fingerprints of a run made with --fingerprints, without "
                                        "labels: pairwise DTW, k-medoids and the silhouette on the GPU; writes templates for detect "
                                        "--barcode_templates (untuned, nothing validated on real data).")
    from .clusters import add_arguments as add_cluster_arguments

    add_cluster_arguments(k)
    n = sub.add_parser("knn", help="(extension) Assign barcodes by the k nearest labelled fingerprints of a run made with --fingerprints "
                                   "(pruned DTW on the GPU), and measure leave-one-out accuracy (untuned, nothing validated on real data).")
    from .knn import add_arguments as add_knn_arguments

    add_knn_arguments(n)
    e = sub.add_parser("events", help="(extension) Recompute the adapter events of a finished run from its detected_boundaries_<k>.csv and "
                                      "the input files: only the adapter slices go to the GPU; writes the polya_length / fingerprints files "
                                      "detect --polya_length / --fingerprints would have (untuned, nothing validated on real data).")
    from .events_command import add_arguments as add_events_arguments

    add_events_arguments(e)
    d.add_argument("-i", "--input", type=str, nargs="+", required=True, help="input files / directories (.pod5 or .npz bundles)")
    d.add_argument("-o", "--output", type=str, default=None)
    d.add_argument("--config", type=str, default=None, help="config TOML (overrides --chemistry)")
    d.add_argument("-c", "--chemistry", type=str, choices=["RNA002", "RNA004"], default=None)
    d.add_argument("--max_obs_trace", type=int, default=None)
    d.add_argument("--read_id_csv", type=str, default=None)
    d.add_argument("--read_id_csv_colname", type=str, default="read_id")
    d.add_argument("-j", "--num_proc", type=int, default=None, help="accepted for compatibility; the GPU engine does not use a process pool")
    d.add_argument("-b", "--batch_size", type=int, default=4000, help="Number of reads per output file.")
    d.add_argument("-s", "--minibatch_size", type=int, default=1000, help="Number of reads per minibatch (normalisation unit).")
    d.add_argument("--start_peak", action="store_true", help="(extension) LLR and CNN primaries: also fill the start_peak_* columns and start_peak_open_pore_type of every read")
    d.add_argument("--second_opinion", type=str, choices=["llr", "llr_resegment"], default=None,
                   help="(extension) CNN primary: reads it fails get the LLR detector's boundaries where those pass validation.  "
                        "llr_resegment: and where those fail behind a first change point, the boundaries of one more segmentation from "
                        "the LLR detector's poly(A) end, validated from its adapter end, where they pass -- such a row's llr_detect_log "
                        "says so (untuned, nothing validated on real data).  Not with --flag_truncated or mvs_detect_overwrite")
    d.add_argument("--flag_truncated", action="store_true",
                   help="(extension) fill the polya_truncated column: True where the poly(A) runs into the end of the preloaded "
                        "signal (rerun those reads with a larger --max_obs_trace: `adapted truncated`), False on every other passing read")
    d.add_argument("--llr_resegment", action="store_true",
                   help="(extension) LLR primary: a read whose first boundaries fail validation behind a first change point (a stall, a "
                        "level step or a long start peak in front of the adapter) is segmented once more from its first poly(A) end and "
                        "validated from its first adapter end; boundaries that pass replace the failed row, whose llr_detect_log says so "
                        "(untuned, nothing validated on real data).  Not with --flag_truncated or mvs_detect_overwrite")
    d.add_argument("--native_csv", action="store_true",
                   help="(extension) print detected_boundaries_<k>.csv and failed_reads_<k>.csv on the GPU from the result rows, without "
                        "pandas: the same bytes (a file that holds a value the GPU printer is not verified for goes through pandas, "
                        "and the log says how many did).  Every primary, every other option, several ranks")
    d.add_argument("--device", type=int, default=None, help="GPU index (default: LOCAL_RANK or 0)")
    d.add_argument("--int16_ingest", action="store_true",
                   help="(extension) move raw int16 ADC samples + calibration to the GPU and compute pA there "
                        "(pA = scale * (float32(adc) + offset)): both primaries, LLR and CNN, read the raw samples on the GPU and "
                        "no float32 copy of the signal is made there; .pod5 inputs or .npz bundles with raw/scale/offset")
    d.add_argument("--polya_length", type=str, choices=["events", "adapter"], default=None,
                   help="(extension) estimate the poly(A) length in bases of every passing read, into polya_length/polya_length_<k>.csv: "
                        "poly(A) samples divided by the read's translocation speed in samples per base.  events: the speed is the "
                        "median length of the events a segmentation of the adapter signal finds (on the GPU); adapter: the adapter's "
                        "samples divided by --adapter_nt.  One GPU, LLR and CNN primaries, float32 ingestion")
    d.add_argument("--adapter_nt", type=float, default=None, help="(extension) the adapter's length in bases (--polya_length adapter)")
    d.add_argument("--event_params", type=str, default=None, metavar="WINDOW,MIN_DISTANCE,THRESHOLD",
                   help="(extension) the event segmentation's parameters (default 8,8,16.0: untuned, chosen on synthetic signals)")
    d.add_argument("--fingerprints", type=int, default=None, metavar="E",
                   help="(extension) the event table and a normalised fingerprint of at most E events (2 .. 512) of every passing read's "
                        "adapter, into fingerprints/fingerprints_<k>.npz beside each detected_boundaries_<k>.csv (on the GPU; untuned, and "
                        "not validated on real barcodes).  One GPU, LLR and CNN primaries, float32 ingestion")
    d.add_argument("--barcode_templates", type=str, default=None, metavar="FILE.npz",
                   help="(extension, with --fingerprints) templates (adapted_amd.fingerprint.save_templates): every fingerprint's DTW "
                        "distance to each and the nearest two, into fingerprints/barcodes_<k>.csv")
    d.add_argument("--adapter_front", action="store_true",
                   help="(extension) trim the front of every passing read's adapter with the reference's moving-mean start detector, on "
                        "the GPU, after validation: adapter_start, adapter_len and the adapter_mean / std / med / mad columns describe the "
                        "trimmed adapter, which --polya_length and --fingerprints then use (validation is not repeated; untuned, nothing "
                        "validated on real data).  LLR and CNN primaries")
    d.add_argument("--adapter_front_revalidate", action="store_true",
                   help="(extension, with --adapter_front) validate every trimmed read again from the new adapter_start, in the same "
                        "call: a row whose validation passes is replaced by it (adapter MAD gate, open pores, real-range check and the "
                        "MVS mean gate are the trimmed adapter's), a read whose validation fails keeps its first row and its "
                        "adapter_start (the trim is rejected).  Not with mvs_detect_overwrite; the detector is still untuned")
    d.add_argument("--adapter_front_params", type=str, default=None, metavar="WINDOW,MIN_OBS_ADAPTER,MIN_SHIFT,MIN_PA",
                   help="(extension, with --adapter_front) the detector's parameters (default 100,2500,20,90: the reference's "
                        "MMAdapterStartConfig, untuned for RNA004)")
    d.add_argument("--dtw_band", type=int, default=None, metavar="R", help="(extension, with --barcode_templates) the DTW's band (default 0: none)")
    return p


def scan_processed_reads(run_dir: str):
    done: Set[str] = set()
    mx = {"failed_reads": -1, "boundaries": -1}
    for sub, prefix in (("failed_reads", "failed_reads_"), ("boundaries", "detected_boundaries_")):
        d = os.path.join(run_dir, sub)
        if not os.path.isdir(d):
            continue
        for f in os.listdir(d):
            if f.startswith(prefix) and f.endswith(".csv"):
                mx[sub] = max(mx[sub], int(f.split("_")[-1].split(".")[0]))
                with open(os.path.join(d, f)) as fh:
                    done.update(line.split(",")[0] for line in fh.readlines()[1:])
    return done, mx["boundaries"], mx["failed_reads"]


POLYA_LENGTH_COLUMNS = ["read_id", "adapter_len", "polya_len", "n_events", "event_len_med", "event_len_mad", "samples_per_nt", "polya_nt",
                        "polya_truncated"]


def polya_length_records(read_ids, results, events, method: str, adapter_nt=None) -> List[dict]:
    """one polya_length_<k>.csv line (POLYA_LENGTH_COLUMNS) per read: its DetectResults and its entry of the pipeline's
    EVENT_DTYPE array -> lengths in samples, the adapter's events, the speed and the poly(A) length in bases"""
    from .polya_length import estimate_polya_length

    med = np.asarray(events["med"], dtype=np.float64)
    nt, spn = estimate_polya_length([r.adapter_start for r in results], [r.adapter_end for r in results], [r.polya_end for r in results],
                                    method=method, event_len_med=med if method == "events" else None, adapter_nt=adapter_nt)
    out = []
    for i, (rid, r) in enumerate(zip(read_ids, results)):
        nb = int(events["n_bound"][i])
        out.append({"read_id": str(rid), "adapter_len": r.adapter_len, "polya_len": r.polya_len,
                    "n_events": max(nb - 1, 0) if nb >= 0 else None, "event_len_med": float(med[i]), "event_len_mad": float(events["mad"][i]),
                    "samples_per_nt": float(spn[i]), "polya_nt": float(nt[i]), "polya_truncated": r.polya_truncated})
    return out


BARCODE_COLUMNS = ["read_id", "n_events", "barcode", "dtw_dist", "barcode_second", "dtw_dist_second", "dtw_margin"]


def fingerprint_records(read_ids, fp, names=None) -> List[dict]:
    """one record per read from the pipeline's AdapterFingerprints: its entries of fingerprints_<k>.npz and, with the templates'
    ``names``, its barcodes_<k>.csv line (BARCODE_COLUMNS) under its "barcode" key"""
    out = []
    for i, rid in enumerate(read_ids):
        rec = {"read_id": str(rid), "count": fp.count[i], "status": fp.status[i], "lengths": fp.lengths[i], "levels": fp.levels[i],
               "fingerprints": fp.fingerprints[i]}
        if names is not None:
            b, b2 = int(fp.best[i, 0]), int(fp.best[i, 1])
            d, d2 = float(fp.bestdist[i, 0]), float(fp.bestdist[i, 1])
            rec["barcode"] = {"read_id": str(rid), "n_events": int(fp.count[i]), "barcode": names[b] if b >= 0 else None, "dtw_dist": d,
                              "barcode_second": names[b2] if b2 >= 0 else None, "dtw_dist_second": d2, "dtw_margin": d2 - d}
        out.append(rec)
    return out


def write_polya_length_file(polya_dir: str, k: int, records):
    """polya_length_<k>.csv from the polya_length_records of a file's reads, in the CSV's order"""
    pd.DataFrame(records, columns=POLYA_LENGTH_COLUMNS).round(3).to_csv(os.path.join(polya_dir, "polya_length_%d.csv" % k), index=False)


def write_fingerprint_files(fp_dir: str, k: int, recs, E: int, barcodes: bool):
    """fingerprints_<k>.npz and, with ``barcodes``, barcodes_<k>.csv from the fingerprint_records of a file's reads, in the CSV's
    order.  Distances are written in full precision."""
    with open(os.path.join(fp_dir, "fingerprints_%d.npz" % k), "wb") as fh:
        np.savez(fh, read_id=np.asarray([r["read_id"] for r in recs], dtype=str),
                 count=np.asarray([r["count"] for r in recs], dtype=np.int32), status=np.asarray([r["status"] for r in recs], dtype=np.int32),
                 lengths=np.asarray([r["lengths"] for r in recs], dtype=np.int32).reshape(len(recs), E),
                 levels=np.asarray([r["levels"] for r in recs], dtype=np.float64).reshape(len(recs), E),
                 fingerprints=np.asarray([r["fingerprints"] for r in recs], dtype=np.float64).reshape(len(recs), E))
    if barcodes:
        pd.DataFrame([r["barcode"] for r in recs], columns=BARCODE_COLUMNS).to_csv(os.path.join(fp_dir, "barcodes_%d.csv" % k), index=False)


class _Writer:
    """Accumulates pass / fail results and flushes CSV files of `batch` reads each."""

    def __init__(self, run_dir: str, batch: int, bidx_pass: int = 0, bidx_fail: int = 0, polya_length: bool = False):
        """polya_length: every detected_boundaries_<k>.csv gets a polya_length/polya_length_<k>.csv beside it, one line per read
        from the `polya_length` record its ReadResult carries (polya_length_records)"""
        self.dirs = {True: os.path.join(run_dir, "boundaries"), False: os.path.join(run_dir, "failed_reads")}
        self.polya_dir = os.path.join(run_dir, "polya_length") if polya_length else None
        for d in list(self.dirs.values()) + ([self.polya_dir] if polya_length else []):
            os.makedirs(d, exist_ok=True)
        self.names = {True: "detected_boundaries", False: "failed_reads"}
        self.bidx = {True: bidx_pass, False: bidx_fail}
        self.pending = {True: [], False: []}
        self.batch = batch
        self.n = {True: 0, False: 0}
        self.fp_dir, self.fp_width, self.barcodes = None, 0, False
        self.csv_engine, self.csv_primary = None, None

    def enable_fingerprints(self, run_dir: str, width: int, barcodes: bool = False):
        """every detected_boundaries_<k>.csv gets a fingerprints/fingerprints_<k>.npz beside it (read_id, count, status, lengths,
        levels, fingerprints: one entry per read, in the CSV's order) and, with ``barcodes``, a fingerprints/barcodes_<k>.csv, from
        the `fingerprint` record its ReadResult carries (fingerprint_records).  Distances are written in full precision."""
        self.fp_dir, self.fp_width, self.barcodes = os.path.join(run_dir, "fingerprints"), int(width), bool(barcodes)
        os.makedirs(self.fp_dir, exist_ok=True)

    def enable_native_csv(self, engine, primary: str):
        """detected_boundaries_<k>.csv and failed_reads_<k>.csv are printed on the GPU from the rows themselves
        (engine.format_csv: the same bytes, no DetectResults, ReadResult or DataFrame): the writer takes `add_rows` instead of
        `add` and keeps pending rows as ROW_DTYPE arrays -- a file's text depends on ALL its rows (pandas picks a column's type
        from the whole file) and a file's rows can come from two detect calls, so a file is formatted when it is flushed.
        engine: an Engine of the writer's own (the writer runs beside the detect calls, and a handle serves one thread at a time)"""
        self.csv_engine, self.csv_primary = engine, primary
        self.pending = {True: ([], [], []), False: ([], [], [])}  # per kind: row arrays, read ids, extension records

    def add_rows(self, rows: np.ndarray, read_ids, extras=None):
        """the rows of a detect call (with enable_native_csv).  extras: None, or per read an object that carries the `polya_length`
        / `fingerprint` record of the extension files, as a ReadResult does in `add`"""
        passed = (rows["success"] != 0) & ~((rows["fail_code"] >= 9) & (rows["fail_code"] <= 14))  # ReadResult.success of rows_to_results
        for ok in (True, False):
            idx = np.flatnonzero(passed == ok)
            chunks, ids, ext = self.pending[ok]
            chunks.append(rows[idx])
            ids.extend(str(read_ids[i]) for i in idx)
            ext.extend(extras[i] if extras is not None else None for i in idx)
            while len(ids) >= self.batch:
                held = np.concatenate(chunks)
                self._flush_rows(ok, held[: self.batch], ids[: self.batch], ext[: self.batch])
                chunks[:] = [held[self.batch:]]
                del ids[: self.batch], ext[: self.batch]

    def _flush_rows(self, ok: bool, rows: np.ndarray, ids, ext):
        with open(os.path.join(self.dirs[ok], "%s_%d.csv" % (self.names[ok], self.bidx[ok])), "wb") as fh:
            fh.write(self.csv_engine.format_csv(rows, ids, self.csv_primary, fail=not ok, consume=True))
        self._flush_extensions(ok, ext)

    def add(self, results: List[ReadResult]):
        for r in results:
            self.pending[bool(r.success)].append(r)
        for ok in (True, False):
            while len(self.pending[ok]) >= self.batch:
                self._flush(ok, self.pending[ok][: self.batch])
                self.pending[ok] = self.pending[ok][self.batch:]

    def _flush(self, ok: bool, items: List[ReadResult]):
        fn = os.path.join(self.dirs[ok], "%s_%d.csv" % (self.names[ok], self.bidx[ok]))
        save_detected_boundaries(items, fn, save_fail_reasons=not ok)
        self._flush_extensions(ok, items)

    def _flush_extensions(self, ok: bool, items):
        """the extension files beside a flushed CSV file, from the records its reads carry; then the file counts"""
        if ok and self.polya_dir:
            write_polya_length_file(self.polya_dir, self.bidx[ok], [r.polya_length for r in items])
        if ok and self.fp_dir:
            write_fingerprint_files(self.fp_dir, self.bidx[ok], [r.fingerprint for r in items], self.fp_width, self.barcodes)
        self.bidx[ok] += 1
        self.n[ok] += len(items)

    def close(self):
        for ok in (True, False):
            if self.csv_engine is not None:
                chunks, ids, ext = self.pending[ok]
                if ids:
                    self._flush_rows(ok, np.concatenate(chunks), ids, ext)
                self.pending[ok] = ([], [], [])
            elif self.pending[ok]:
                self._flush(ok, self.pending[ok])
                self.pending[ok] = []


def _init_dist(device=None):
    """one process per GPU: the process group (RCCL = "nccl"; ADAPTED_DIST_BACKEND=gloo for CPU-side rehearsals / tests)"""
    rank, ws, local = parallel.world()
    if ws <= 1 and os.environ.get("ADAPTED_DIST_FORCE", "0") != "1":  # (forced: the several-ranks code on a group of one)
        return None
    import torch
    import torch.distributed as dist

    backend = os.environ.get("ADAPTED_DIST_BACKEND", "nccl")
    if not dist.is_initialized():
        if backend == "nccl":
            torch.cuda.set_device(local if device is None else device)
        if "MASTER_ADDR" not in os.environ:  # (forced group of one without a launcher)
            import socket

            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
            os.environ["MASTER_ADDR"] = "127.0.0.1"
        dist.init_process_group(backend, rank=rank, world_size=ws)
    return dist


def _load_spc(args):
    spc = load_nested_config_from_file(args.config) if args.config else get_chemistry_specific_config(args.chemistry)
    if args.max_obs_trace:
        spc.core.max_obs_trace = args.max_obs_trace
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


def _check_second_opinion(args):
    """--second_opinion goes with the CNN primary only, and llr_resegment not with everything: said before a GPU is touched"""
    choice = getattr(args, "second_opinion", None)
    if choice and (args.config or args.chemistry):
        spc = _load_spc(args)
        primary = spc.primary_method
        if primary != "cnn":
            raise SystemExit("--second_opinion %s needs the CNN primary (cnn_boundaries.cnn_detect); this configuration's primary is %s." % (choice, primary))
        if choice == "llr_resegment":
            why = lib.second_resegment_unsupported(spc, bool(getattr(args, "flag_truncated", False)))
            if why:
                raise SystemExit("--second_opinion llr_resegment does not go with this run: %s." % why)


def _check_flag_truncated(args):
    """--flag_truncated and what it does not go with: said before a GPU is touched"""
    if getattr(args, "flag_truncated", False) and (args.config or args.chemistry):
        spc = _load_spc(args)
        if spc.primary_method not in ("llr", "cnn"):
            raise SystemExit("--flag_truncated goes with the LLR and CNN primaries; this configuration's primary is %s." % spc.primary_method)
        why = lib.truncation_unsupported(spc)
        if why:
            raise SystemExit("--flag_truncated does not go with this configuration: %s." % why)


def _check_llr_resegment(args):
    """--llr_resegment and what it does not go with: said before a GPU is touched"""
    if getattr(args, "llr_resegment", False) and (args.config or args.chemistry):
        spc = _load_spc(args)
        why = lib.resegment_unsupported(spc, bool(getattr(args, "flag_truncated", False)))
        if why:
            hint = " (with the CNN primary: --second_opinion llr_resegment)" if spc.primary_method == "cnn" else ""
            raise SystemExit("--llr_resegment does not go with this run: %s%s." % (why, hint))


def _check_adapter_front(args):
    """--adapter_front and what it does not go with: said before a GPU is touched.  -> its AdapterFrontParams (min_adapter_len left
    to run_detect, which knows the configuration), or None"""
    text = getattr(args, "adapter_front_params", None)
    reval = bool(getattr(args, "adapter_front_revalidate", False))
    if not getattr(args, "adapter_front", False):
        if text:
            raise SystemExit("--adapter_front_params goes with --adapter_front.")
        if reval:
            raise SystemExit("--adapter_front_revalidate goes with --adapter_front.")
        return None
    from .adapter_front import AdapterFrontParams

    try:
        params = AdapterFrontParams.parse(text) if text else AdapterFrontParams()
    except ValueError as e:
        raise SystemExit("--adapter_front_params: %s." % e)
    if args.config or args.chemistry:
        primary = _load_spc(args).primary_method
        if primary not in ("llr", "cnn"):
            raise SystemExit("--adapter_front goes with the LLR and CNN primaries; this configuration's primary is %s." % primary)
        if reval and bool(_load_spc(args).mvs_polya.mvs_detect_overwrite):
            raise SystemExit("--adapter_front_revalidate does not go with mvs_polya.mvs_detect_overwrite.")
    params.revalidate = reval
    return params


def _check_fingerprints(args):
    """--fingerprints and what it does not go with: said before a GPU is touched.  -> the templates of --barcode_templates, or None"""
    E = getattr(args, "fingerprints", None)
    if E is None:
        if getattr(args, "barcode_templates", None) or getattr(args, "dtw_band", None) is not None:
            raise SystemExit("--barcode_templates and --dtw_band go with --fingerprints.")
        return None
    from .fingerprint import FingerprintParams, load_templates
    from .polya_length import EventParams

    if not 2 <= E <= lib.FINGERPRINT_MAX_EVENTS:
        raise SystemExit("--fingerprints: the number of events must lie in [2, %d]." % lib.FINGERPRINT_MAX_EVENTS)
    if getattr(args, "int16_ingest", False):
        raise SystemExit("--fingerprints does not go with --int16_ingest: the event segmentation reads the float32 signal on the GPU, "
                         "and that plan keeps none there.")
    if parallel.world()[1] > 1:
        raise SystemExit("--fingerprints runs on one GPU: the fingerprint files are not gathered from several ranks.")
    band = getattr(args, "dtw_band", None)
    if band is not None and not getattr(args, "barcode_templates", None):
        raise SystemExit("--dtw_band goes with --barcode_templates.")
    if band is not None and band < 0:
        raise SystemExit("--dtw_band must be >= 0.")
    try:
        FingerprintParams(E, EventParams.parse(args.event_params) if getattr(args, "event_params", None) else EventParams(), band or 0).check()
    except ValueError as e:
        raise SystemExit("--event_params: %s." % e)
    templates = None
    if getattr(args, "barcode_templates", None):
        try:
            templates = load_templates(args.barcode_templates)
        except ValueError as e:
            raise SystemExit("--barcode_templates: %s." % e)
    if args.config or args.chemistry:
        primary = _load_spc(args).primary_method
        if primary not in ("llr", "cnn"):
            raise SystemExit("--fingerprints goes with the LLR and CNN primaries; this configuration's primary is %s." % primary)
    return templates


def _check_polya_length(args):
    """--polya_length and what it does not go with: said before a GPU is touched"""
    method = getattr(args, "polya_length", None)
    if not method:
        if getattr(args, "adapter_nt", None) is not None or (getattr(args, "event_params", None) and getattr(args, "fingerprints", None) is None):
            raise SystemExit("--adapter_nt and --event_params go with --polya_length.")
        return
    if getattr(args, "int16_ingest", False):
        raise SystemExit("--polya_length does not go with --int16_ingest: the event segmentation reads the float32 signal on the GPU, "
                         "and that plan keeps none there.")
    if parallel.world()[1] > 1:
        raise SystemExit("--polya_length runs on one GPU: the polya_length files are not gathered from several ranks.")
    if method == "adapter" and getattr(args, "adapter_nt", None) is None:
        raise SystemExit("--polya_length adapter needs --adapter_nt, the adapter's length in bases.")
    if getattr(args, "adapter_nt", None) is not None and not args.adapter_nt > 0:
        raise SystemExit("--adapter_nt must be > 0.")
    if getattr(args, "event_params", None):
        from .polya_length import EventParams

        try:
            EventParams.parse(args.event_params)
        except ValueError as e:
            raise SystemExit("--event_params: %s." % e)
    if args.config or args.chemistry:
        primary = _load_spc(args).primary_method
        if primary not in ("llr", "cnn"):
            raise SystemExit("--polya_length goes with the LLR and CNN primaries; this configuration's primary is %s." % primary)


def list_truncated(directory: str) -> int:
    """`adapted truncated`: the read ids whose polya_truncated column reads True, over all detected_boundaries_*.csv of the
    directory (or of its boundaries/ folder) in file order, into truncated_read_ids.csv (header read_id) beside them -- what the
    reference's scripts/get_truncated.sh does, with the column found by name.  -> the number of ids written"""
    import csv
    import re

    where = directory
    if os.path.isdir(os.path.join(directory, "boundaries")):
        where = os.path.join(directory, "boundaries")
    found = []
    if os.path.isdir(where):
        for f in os.listdir(where):
            mt = re.fullmatch(r"detected_boundaries_(\d+)\.csv", f)
            if mt:
                found.append((int(mt.group(1)), f))
    if not found:
        print("No detected_boundaries_*.csv files found in {}".format(where))
        raise SystemExit(1)
    ids = []
    for _, f in sorted(found):
        with open(os.path.join(where, f), newline="") as fh:
            rd = csv.reader(fh)
            header = next(rd, None)
            if header is None:
                continue
            if "read_id" not in header or "polya_truncated" not in header:
                print("{}: no read_id / polya_truncated column".format(os.path.join(where, f)))
                raise SystemExit(1)
            ci, ct = header.index("read_id"), header.index("polya_truncated")
            ids.extend(row[ci] for row in rd if len(row) > max(ci, ct) and row[ct] == "True")
    out = os.path.join(where, "truncated_read_ids.csv")
    with open(out, "w", newline="") as fh:
        fh.write("read_id\n")
        for rid in ids:
            fh.write(rid + "\n")
    print("Truncated read ids saved to {} ({} reads)".format(out, len(ids)))
    return len(ids)


def run_detect(files, read_ids_incl, read_ids_excl, spc, run_dir, minibatch, batch_out, device, start_peak=False,
               bidx_pass=0, bidx_fail=0, int16_ingest=False, second_opinion=None, flag_truncated=False, llr_resegment=False, native_csv=False,
               adapter_front=None, fingerprints=None, polya_length=None, adapter_nt=None, event_params=None):
    """native_csv: --native_csv (rank 0 prints the two reference files on the GPU from the rows: _Writer.enable_native_csv);
    llr_resegment: --llr_resegment (the LLR primary's detect calls re-segment the reads they fail; everything below sees the final rows);
    adapter_front: None, or an adapter_front.AdapterFrontParams (--adapter_front: the adapter's front trimmed on the final rows of
    every detect call, ahead of the two below; its min_adapter_len is set here to core.min_obs_adapter);
    fingerprints: None, or (E, templates or None, band) (--fingerprints: fingerprints/fingerprints_<k>.npz and, with templates,
    fingerprints/barcodes_<k>.csv beside boundaries/; the events' parameters are event_params);
    polya_length: None, "events" or "adapter" (--polya_length: polya_length/polya_length_<k>.csv beside boundaries/);
    adapter_nt: the adapter's bases for "adapter"; event_params: "WINDOW,MIN_DISTANCE,THRESHOLD" or None"""
    rank, ws, local = parallel.world()
    if device is None:
        device = local
        if ws > 1 and os.environ.get("ADAPTED_DIST_BACKEND", "nccl") != "nccl":
            device = local % max(lib.load().adp_device_count(), 1)  # (a rehearsal may share devices)
    dist = _init_dist(device)
    multi = dist is not None  # several ranks (or a forced group of one): rows gathered to rank 0, written in stream order
    primary = spc.primary_method
    model = None  # CNN primary: the weights named in the config go to the engine on first use (no PyTorch module needed)
    m = spc.sig_preload_size
    if polya_length and (ws > 1 or int16_ingest or primary not in ("llr", "cnn")):
        raise ValueError("polya_length: one GPU, the LLR or CNN primary, no int16 ingest")
    if fingerprints and (ws > 1 or int16_ingest or primary not in ("llr", "cnn")):
        raise ValueError("fingerprints: one GPU, the LLR or CNN primary, no int16 ingest")
    writer = (_Writer(run_dir, batch_out, bidx_pass, bidx_fail, polya_length=True) if polya_length
              else _Writer(run_dir, batch_out, bidx_pass, bidx_fail)) if rank == 0 else None
    if fingerprints and writer is not None:
        writer.enable_fingerprints(run_dir, fingerprints[0], barcodes=fingerprints[1] is not None)
    csv_engine = None
    if native_csv and writer is not None:  # (an engine of the writer's own: it formats beside the detect calls)
        csv_engine = lib.Engine(spc, 1, m, device=device)
        writer.enable_native_csv(csv_engine, primary)
    t0 = time.time()
    my_rows, my_ids, my_ord = [], [], []
    dropped_text = {1: "MAD normalization failed: scale is 0", 2: "a read has no signal after min_obs_adapter"}
    from .io_utils import GroupSharder
    from .pipeline import HostPipeline

    # pinned staging slots filled in place by a producer thread, H2D overlapped with the detect call, CSV writing in
    # a third thread (adapted_amd/pipeline.py).  The reads travel packed back to back and the padded matrix is laid out on
    # the device (only the samples that exist cross PCIe).  Several ranks: every rank walks the stream's METADATA and
    # decodes only the groups of whole minibatches a GroupSharder assigns to it (balanced by preloaded samples).
    GROUP = 4  # minibatches per staging slot and detect call (normalisation stays per minibatch)
    pipe = HostPipeline(spc, minibatch, m, device=device, primary=primary, with_start_peak=start_peak,
                        model=model, int16_input="native" if int16_ingest else False, group=GROUP, ragged=True, second_opinion=second_opinion,
                        flag_truncated=flag_truncated, resegment=llr_resegment)
    if adapter_front is not None:
        import dataclasses

        pipe.enable_adapter_front(dataclasses.replace(adapter_front, min_adapter_len=int(spc.core.min_obs_adapter)))
    if polya_length:
        from .polya_length import EventParams

        pipe.enable_polya_length(EventParams.parse(event_params) if event_params else None)
    if fingerprints:
        from .fingerprint import FingerprintParams
        from .polya_length import EventParams

        pipe.enable_fingerprints(FingerprintParams(int(fingerprints[0]), EventParams.parse(event_params) if event_params else EventParams(),
                                                   int(fingerprints[2] or 0)), fingerprints[1])
    n_second = [0]  # rows the LLR second opinion made (they say so themselves: reserved_ bit 0)
    n_trunc = [0]  # rows the truncation look replaced (reserved_ bit 1)
    n_front = [0]  # rows whose adapter_start the adapter-front pass moved (reserved_ bit 3)
    n_reval = [0]  # ... that are the validation from the trimmed start (reserved_ bit 4: --adapter_front_revalidate)
    reseg_marks = []  # reserved_ of the rows the re-segmentation made (bit 5; bits 6-9: the first row's fail_code)
    n_rejected = [0]  # trims that validation rejected (the pipeline counts them: such a row says nothing)
    sharder = GroupSharder(ws, rank, m) if multi else None
    ordinals: List[int] = []  # stream index of the first read of every group this rank yields

    def fill(get_buffers):
        from .io_utils import yield_minibatches_packed

        for k, ids in yield_minibatches_packed(files, read_ids_incl, read_ids_excl, minibatch * GROUP, m, get_buffers,
                                               int16=int16_ingest, sharder=sharder, ordinals=ordinals):
            # ids travel with the stream position of each read: (id, ordinal) pairs survive the slicing of dropped minibatches
            tagged = np.empty((k, 2), dtype=object)
            tagged[:, 0] = ids[:k]
            tagged[:, 1] = np.arange(ordinals[-1], ordinals[-1] + k)
            yield k, tagged

    def on_rows(tagged, rows, events=None, fp=None):
        if multi:
            my_rows.append(rows)
            my_ids.extend(tagged[:, 0].tolist())
            my_ord.extend(int(x) for x in tagged[:, 1])
        else:
            n_second[0] += int(((rows["reserved_"] & lib.ROW_FROM_SECOND_LLR) != 0).sum())
            n_trunc[0] += int(((rows["reserved_"] & lib.ROW_POLYA_TRUNCATED) != 0).sum())
            n_front[0] += int(((rows["reserved_"] & lib.ROW_ADAPTER_FRONT) != 0).sum())
            n_reval[0] += int(((rows["reserved_"] & lib.ROW_REVALIDATED) != 0).sum())
            reseg_marks.append(rows["reserved_"][(rows["reserved_"] & lib.ROW_RESEGMENTED) != 0])
            if csv_engine is not None:
                extras = None
                if events is not None or fp is not None:  # the extension files' records travel beside the rows
                    import types

                    extras = [types.SimpleNamespace() for _ in range(len(rows))]
                    if events is not None:
                        for x, rec in zip(extras, polya_length_records(tagged[:, 0], lib.rows_to_results(rows, primary), events, polya_length, adapter_nt)):
                            x.polya_length = rec
                    if fp is not None:
                        for x, rec in zip(extras, fingerprint_records(tagged[:, 0], fp, fingerprints[1].names if fingerprints[1] is not None else None)):
                            x.fingerprint = rec
                writer.add_rows(rows, tagged[:, 0], extras)
                return
            res = lib.rows_to_results(rows, primary, consume=True)
            out = [ReadResult(read_id=str(rid), success=r.success, fail_reason=r.fail_reason, detect_results=r)
                   for rid, r in zip(tagged[:, 0], res)]
            if events is not None:
                for rr, rec in zip(out, polya_length_records(tagged[:, 0], res, events, polya_length, adapter_nt)):
                    rr.polya_length = rec
            if fp is not None:
                for rr, rec in zip(out, fingerprint_records(tagged[:, 0], fp, fingerprints[1].names if fingerprints[1] is not None else None)):
                    rr.fingerprint = rec
            writer.add(out)

    def on_dropped(tagged, status):
        logging.error("minibatch of %d reads dropped: %s", len(tagged), dropped_text.get(status, status))

    try:
        pipe.run(fill, on_rows, on_dropped)
    finally:
        pipe.close()
    if multi:
        rows = np.concatenate(my_rows) if my_rows else np.zeros(0, dtype=lib.ROW_DTYPE)
        allrows = parallel.gather_rows(rows, dst=0, always=True)
        lists = [None] * ws if rank == 0 else None
        mine = (my_ids, my_ord)
        if getattr(adapter_front, "revalidate", False):  # (the rejected trims: such a row says nothing)
            mine += (int(pipe.front_rejected),)
        dist.gather_object(mine, lists, dst=0)
        if rank == 0:
            ids = [x for part in lists for x in part[0]]
            order = np.argsort(np.array([x for part in lists for x in part[1]], dtype=np.int64), kind="stable")
            n_second[0] += int(((allrows["reserved_"] & lib.ROW_FROM_SECOND_LLR) != 0).sum())
            n_trunc[0] += int(((allrows["reserved_"] & lib.ROW_POLYA_TRUNCATED) != 0).sum())
            n_front[0] += int(((allrows["reserved_"] & lib.ROW_ADAPTER_FRONT) != 0).sum())
            n_reval[0] += int(((allrows["reserved_"] & lib.ROW_REVALIDATED) != 0).sum())
            reseg_marks.append(allrows["reserved_"][(allrows["reserved_"] & lib.ROW_RESEGMENTED) != 0])
            n_rejected[0] += sum(int(part[2]) for part in lists if len(part) > 2)
            if csv_engine is not None:
                writer.add_rows(allrows[order], [ids[i] for i in order])
            else:
                res = lib.rows_to_results(allrows[order], primary, consume=True)  # stream order: the files read like a one-GPU run's
                writer.add([ReadResult(read_id=str(ids[i]), success=r.success, fail_reason=r.fail_reason, detect_results=r)
                            for i, r in zip(order, res)])
    if writer is not None:
        try:
            writer.close()
        finally:
            if csv_engine is not None:
                csv_engine.close()
        tot = writer.n[True] + writer.n[False]
        logging.info("Processed %d reads in %.2f s (%.0f reads/s on %d GPU(s))", tot, time.time() - t0,
                     tot / max(time.time() - t0, 1e-9), ws)
        if tot:
            logging.info("Pass: %d (%.2f%%), fail: %d", writer.n[True], 100.0 * writer.n[True] / tot, writer.n[False])
        if second_opinion:
            logging.info("Second opinion (%s): %d of the passing reads", second_opinion, n_second[0])
        if second_opinion == "llr_resegment":
            logging.info(lib.resegment_log(np.concatenate(reseg_marks) if reseg_marks else np.zeros(0, dtype=np.int32)))
        if flag_truncated:
            logging.info("Truncated poly(A) (polya_truncated): %d of the passing reads", n_trunc[0])
        if adapter_front is not None:
            logging.info("Adapter front (adapter_start moved): %d of the passing reads", n_front[0])
            if getattr(adapter_front, "revalidate", False):
                if not multi:
                    n_rejected[0] = int(getattr(pipe, "front_rejected", 0))
                logging.info("Adapter front re-validated: %d kept, %d trims rejected by validation", n_reval[0], n_rejected[0])
        if csv_engine is not None:
            logging.info("native CSV: %d files, %d through pandas", csv_engine.csv_files, csv_engine.csv_fallback_files)
        if llr_resegment:
            logging.info(lib.resegment_log(np.concatenate(reseg_marks) if reseg_marks else np.zeros(0, dtype=np.int32)))
    if multi:
        dist.barrier()
        logging.info("process group: backend %s, %d rank(s); HIP runtimes mapped: %s", dist.get_backend(), ws, ", ".join(lib.hip_runtimes()))


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode == "truncated":
        list_truncated(args.directory)
        return
    if args.mode == "templates":
        from .barcode_templates import templates_command

        templates_command(args)
        return
    if args.mode == "clusters":
        from .clusters import clusters_command

        clusters_command(args)
        return
    if args.mode == "knn":
        from .knn import knn_command

        knn_command(args)
        return
    if args.mode == "events":
        from .events_command import events_command

        events_command(args)
        return
    if args.mode == "continue":
        run_dir = args.continue_from
        try:
            with open(os.path.join(run_dir, "command.json")) as fh:
                cmd = json.load(fh)
        except FileNotFoundError:
            raise SystemExit("No command.json file found in the continue_from directory.")
        shutil.copy(os.path.join(run_dir, "command.json"), os.path.join(run_dir, "command_previous.json"))
        for k, v in cmd.items():
            if not hasattr(args, k):
                setattr(args, k, v)
        _check_second_opinion(args)
        _check_flag_truncated(args)
        _check_llr_resegment(args)
        _check_polya_length(args)
        front = _check_adapter_front(args)
        templates = _check_fingerprints(args)
    else:
        args.output = args.output or os.getcwd()
        run_dir = os.path.join(args.output, "adapted_" + __version__.replace(".", "_") + "_" + str(uuid.uuid4())[:8])
        _check_second_opinion(args)
        _check_flag_truncated(args)
        _check_llr_resegment(args)
        _check_polya_length(args)
        front = _check_adapter_front(args)
        templates = _check_fingerprints(args)
        dist = _init_dist(getattr(args, "device", None))
        if dist is not None:  # one run directory for all ranks: rank 0's name
            box = [run_dir]
            dist.broadcast_object_list(box, src=0)
            run_dir = box[0]
    if not args.config and not args.chemistry:
        raise SystemExit("Either --config or --chemistry must be provided.")
    read_ids: List[str] = []
    if args.read_id_csv:
        import pandas as pd

        read_ids = pd.read_csv(args.read_id_csv)[args.read_id_csv_colname].astype(str).tolist()
    files = input_to_filelist(args.input)
    if not files:
        print("No valid input files found.\nProvided path: {}".format(args.input))
        raise SystemExit(1)
    spc = _load_spc(args)
    rank = parallel.world()[0]
    if rank == 0:
        os.makedirs(run_dir, exist_ok=True)
        with open(os.path.join(run_dir, "command.json"), "w") as fh:
            json.dump(vars(args), fh, indent=2)
        spc.to_toml(os.path.join(run_dir, "config.toml"))
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s",
                        handlers=[logging.StreamHandler(sys.stdout)] +
                        ([logging.FileHandler(os.path.join(run_dir, "adapted.log"))] if rank == 0 else []))
    logging.info("Command: %s", " ".join(sys.argv))
    logging.info("Saving output to: %s", run_dir)
    excl: Set[str] = set()
    bp = bf = 0
    if args.mode == "continue":
        excl, mp, mf = scan_processed_reads(run_dir)
        bp, bf = mp + 1, mf + 1
        logging.info("Found %d previously processed reads.", len(excl))
    run_detect(files, set(read_ids), excl, spc, run_dir, args.minibatch_size, args.batch_size, args.device,
               start_peak=getattr(args, "start_peak", False), bidx_pass=bp, bidx_fail=bf,
               int16_ingest=getattr(args, "int16_ingest", False), second_opinion=getattr(args, "second_opinion", None),
               flag_truncated=getattr(args, "flag_truncated", False), adapter_front=front, llr_resegment=getattr(args, "llr_resegment", False),
               native_csv=getattr(args, "native_csv", False),
               fingerprints=(args.fingerprints, templates, getattr(args, "dtw_band", None)) if getattr(args, "fingerprints", None) is not None else None,
               polya_length=getattr(args, "polya_length", None),
               adapter_nt=getattr(args, "adapter_nt", None), event_params=getattr(args, "event_params", None))
    logging.info("Done.")


if __name__ == "__main__":
    main()
