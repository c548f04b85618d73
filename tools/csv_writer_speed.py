#!/usr/bin/env python
"""Rows per second of the two CSV writers on the same rows, in one process: Engine.format_csv (the GPU prints the file's text:
`detect --native_csv`) against output.save_detected_boundaries on lib.rows_to_results (pandas).  96 000 synthetic all-present LLR rows
in files of 4000, every file formatted by both routes and the texts compared; the native route's time includes the staging of the
rows, the copy of the text back and the Python around the call (the read ids packed, the text as bytes), and is split into that
Python and the library call.  Neither route writes to a disk.

    python tools/csv_writer_speed.py [--rows 96000] [--file 4000] [--repeats 15] [--out profiles/csv_writer_speed.json]

The yardstick is the best recorded rate of the host pipeline that feeds the writer (BENCH_r05.json, summary.host_pipeline:
260.9 k reads/s): at or above it the writer is not the slowest stage of a run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_PIPELINE_BEST = 260.9e3


def typical_rows(n, seed=0):
    """passing LLR rows as a run makes them: every column of the LLR path present, one poly(A) candidate, now and then open pores"""
    from adapted_amd import lib

    rng = np.random.default_rng(seed)
    rows = lib.empty_rows(n)
    llr_cols = [c for c in range(lib.NCOL) if c not in (22, 23, 24, 25, 26, 27, 38)]
    rows["present"] = sum(1 << c for c in llr_cols)
    for c in llr_cols:
        rows["col"][:, c] = rng.integers(500, 20000, n) if c in lib._INT_COLS else rng.normal(90.0, 25.0, n).astype(np.float32)
    rows["success"] = 1
    rows["n_cand"] = 1
    rows["cand"][:, 0] = rng.integers(3000, 9000, n)
    k = np.where(rng.random(n) < 0.1, rng.integers(1, 6, n), 0)
    rows["n_open_pores"] = k
    rows["open_pores"][:, :5] = np.sort(rng.integers(0, 3000, (n, 5)), axis=1)
    ids = ["%08x-%04x-%04x-%04x-%012x" % tuple(int(x) for x in rng.integers(0, 2 ** 16, 5) * [65536, 1, 1, 1, 2 ** 32]) for _ in range(n)]
    return rows, ids


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=96000)
    ap.add_argument("--file", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=15, help="passes of the native route over all files (the median is reported)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "csv_writer_speed.json"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.update_primary_method()
    spc.update_sig_preload_size()
    eng = lib.Engine(spc, 1, spc.sig_preload_size, device=args.device)
    rows, ids = typical_rows(args.rows)
    files = [(rows[a:a + args.file], ids[a:a + args.file]) for a in range(0, args.rows, args.file)]
    eng.format_csv(*files[0], "llr")  # (both routes once before the clock: the workspace, the string table, pandas' imports)
    lib.rows_csv_text(*files[0], "llr")
    call = [0.0]
    inner = eng.lib.adp_format_rows

    class Timed:  # the library call's share of the native route
        def __getattr__(self, name):
            return getattr(eng_lib, name)

        def adp_format_rows(self, *a):
            t = time.perf_counter()
            rc = inner(*a)
            call[0] += time.perf_counter() - t
            return rc

    eng_lib, eng.lib = eng.lib, Timed()
    passes = []  # the native route is over in milliseconds: several passes over the files, the median pass reported
    for _ in range(args.repeats):
        call[0] = 0.0
        t0 = time.perf_counter()
        native = [eng.format_csv(r, i, "llr") for r, i in files]
        passes.append((time.perf_counter() - t0, call[0]))
    t_native, call[0] = sorted(passes)[len(passes) // 2]
    eng.lib = eng_lib
    t0 = time.perf_counter()
    results = [lib.rows_to_results(r, "llr") for r, _ in files]
    t_results = time.perf_counter() - t0
    t0 = time.perf_counter()
    pandas_text = [lib.rows_csv_text(r, i, "llr") for r, i in files]
    t_pandas = time.perf_counter() - t0
    del results
    same = native == pandas_text
    out = {"rows": args.rows, "rows_per_file": args.file, "files": len(files), "bytes": sum(len(t) for t in native), "texts_identical": same,
           "files_through_pandas_of_all_passes": eng.csv_fallback_files,
           "native": {"passes_seconds": [round(t, 6) for t, _ in passes], "seconds": t_native, "rows_per_s": args.rows / t_native, "library_call_seconds": call[0],
                      "python_packing_seconds": t_native - call[0]},
           "pandas": {"seconds": t_pandas, "rows_per_s": args.rows / t_pandas, "rows_to_results_seconds": t_results,
                      "frame_and_to_csv_seconds": t_pandas - t_results},
           "host_pipeline_best_rows_per_s": HOST_PIPELINE_BEST, "native_reaches_host_pipeline": args.rows / t_native >= HOST_PIPELINE_BEST}
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=2)
        fh.write("\n")
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
