#!/usr/bin/env python3
"""Reads/s of the LLR trace module's batch operators (adp_llr_trace_bounds, adp_llr_trace_peaks, adp_llr_spike_peak;
adapted_amd/csrc/trace_peaks_api.h) on float64 traces resident in HBM: 96 000 traces of 1 600 points (the preset's 16 k window
pooled by 10) and 24 000 of 20 150 points (the 200 k window).  Per-kernel times from adp_kernel_times (HIP events on the handle's
stream) and the mean number of strict local maxima per read's clip (the maxima the peaks kernel evaluates).  The traces: 64
device-computed adapter traces of synthetic reads (offsets 5 / 5, stride 1), rotated.
``--reference``: instead, the reference's per-read adapter_end_from_trace on the CPU over the same kind of traces (run with the
reference's interpreter in the build container: python3.9 tools/llr_module_speed.py --reference).
Usage: python tools/llr_module_speed.py [--reps R] [--out FILE] [--reference] [--ref-reads N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((96_000, 1_600), (24_000, 20_150))
WIDTH, PROM, REL = 200, 1.0, 1.0  # adapter_end_from_trace as combined.py calls it on 10x pooled traces (width 2000 // 10)


def base_raw(L, k=64):
    from adapted_amd.synth import synth_read

    return np.stack([synth_read(3, r, 10 * L, 10 * L).astype(np.float64).reshape(L, 10).mean(axis=1) for r in range(k)])


def n_maxima(y, lo, hi):
    c = y[lo:hi]
    return int(np.count_nonzero((c[1:-1] > c[:-2]) & (c[1:-1] > c[2:])))


def timed(eng, fn, reps):
    fn()  # warm-up
    eng.set_profiling(False)
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    wall = (time.perf_counter() - t) / reps
    eng.set_profiling(True)
    fn()
    kt = {}
    for name, ms in eng.kernel_times():
        kt[name] = kt.get(name, 0.0) + ms
    eng.set_profiling(False)
    return wall, kt


def run_gpu(n, L, reps):
    from adapted_amd.detect import _c_llr, llr

    eng = _c_llr._engine()
    raw = base_raw(L)
    k = raw.shape[0]
    g, st, en, es = llr.calc_adapter_trace_batch(raw, np.full(k, L), 5, 5, 1, 0, 0, 0, 0, adapter_early_stopping=0, polya_early_stopping=0)
    x = np.empty((n, L))
    for r in range(n):
        x[r] = g[r % k]
    lens = np.full(n, L)
    sts, ens = st[np.arange(n) % k], en[np.arange(n) % k]
    maxima = float(np.mean([n_maxima(g[r], int(st[r]), int(en[r])) for r in range(k)]))
    dev = eng.dev_alloc(x.nbytes)
    out = dict(points=L, reads=n, reps=reps, local_maxima_per_read=maxima)
    try:
        eng.h2d(dev, x)
        ops = {
            "bounds": lambda: eng.llr_trace_bounds(dev, lens, np.full(n, 5), np.full(n, 5), 1, False, n=n, L=L),
            "adapter_end_from_trace": lambda: llr.adapter_end_from_trace_batch(dev, lens, sts, ens, PROM, REL, WIDTH, True, True, n=n, L=L),
            "find_peaks_in_trace": lambda: llr.find_peaks_in_trace_batch(dev, lens, sts, ens, WIDTH, PROM, REL, n=n, L=L),
            "spike": lambda: llr.detect_full_polya_trace_peak_with_spike_batch(dev, lens, n=n, L=L),
        }
        for name, fn in ops.items():
            wall, kt = timed(eng, fn, reps)
            out[name] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall, kernel_ms=kt)
        pk, cnt = llr.adapter_end_from_trace_batch(dev, lens, sts, ens, PROM, REL, WIDTH, True, True, n=n, L=L)
        out["adapter_end_peaks_per_read"] = float(cnt.mean())
    finally:
        eng.dev_free(dev)
    return out


def run_reference(L, reads):
    from oracle import ref_harness

    ref_harness.install()
    from adapted.detect import llr as ref

    raw = base_raw(L, min(reads, 64))
    traces = [ref.calc_adapter_trace(raw[r], 5, 5, 1, 0, 0, 0, 0, False, adapter_early_stopping=0, polya_early_stopping=0)
              for r in range(raw.shape[0])]
    t = time.perf_counter()
    for r in range(reads):
        ref.adapter_end_from_trace(traces[r % len(traces)], PROM, REL, WIDTH, True, True)
    wall = time.perf_counter() - t
    t = time.perf_counter()
    for r in range(reads):
        ref.detect_full_polya_trace_peak_with_spike(traces[r % len(traces)].signal)
    wall2 = time.perf_counter() - t
    return dict(points=L, reads=reads, adapter_end_from_trace_reads_per_s=reads / wall, spike_reads_per_s=reads / wall2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-reads", type=int, default=2000)
    a = ap.parse_args()
    if a.reference:
        res = [run_reference(L, a.ref_reads) for _, L in SHAPES]
    else:
        res = [run_gpu(n, L, a.reps) for n, L in SHAPES]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
