#!/usr/bin/env python3
"""Reads/s of the signal statistics modules' batch forms (adp_seg_stats, adp_real_range, adp_open_pores, adp_med_mad,
adp_normalize, adp_pool_mean: adapted_amd/csrc/sigstats_api.h) with float32 (or, --dtype float64, float64) reads resident in HBM,
at 16 000 and 200 000 samples; per-kernel times from adp_kernel_times (HIP events on the handle's stream).  For the partition
statistics and the whole-array normalisation also the bytes each kernel reads divided by its time.  --sweep: median / MAD of one
population of 2^12 .. 2^24 samples by one wave and by many workgroups -- what ADP_SS_GRID_MIN is set from.

  python tools/sigstats_module_speed.py [--reads N] [--reps R] [--dtype float32|float64] [--sweep] [--out FILE]
  python3.9 tools/sigstats_module_speed.py --reference [--out FILE]   (build container only: the reference's modules on one
                                                                       CPU core, on the same reads)"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sigstats_module_cases as M  # noqa: E402


def reads(n, L, seed=3):
    """float32 [n, L] (sixteen reads in turn), adapter end and poly(A) end per read"""
    rng = np.random.default_rng(seed)
    base = [M.read(100 + s, L, quantised=(s % 8 == 5)) for s in range(16)]
    x = np.empty((n, L), dtype=np.float32)
    ae = np.zeros(n, dtype=np.int64)
    pe = np.zeros(n, dtype=np.int64)
    for r in range(n):
        b, a, e = base[r % 16]
        x[r] = b
        ae[r], pe[r] = a + int(rng.integers(-40, 40)), e + int(rng.integers(-40, 40))
    return x, ae, pe


def _timed(eng, fn, reps):
    fn()  # warm-up
    eng.set_profiling(False)
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    wall = (time.perf_counter() - t) / reps
    eng.set_profiling(True)
    fn()
    kt = {}
    for k, ms in eng.kernel_times():
        kt[k] = kt.get(k, 0.0) + ms
    eng.set_profiling(False)
    return wall, kt


def device(n, L, reps, dtype=np.float32):
    from adapted_amd.config.schema import RealRangeConfig
    from adapted_amd.detect import anomalies, downscale, normalize, real_range
    from adapted_amd.detect._rows import _engine
    from adapted_amd.partition import signal_partitions as sp

    eng = _engine()
    x, ae, pe = reads(n, L)
    x = x.astype(dtype, copy=False)
    esz = x.dtype.itemsize
    lens = np.full(n, L, dtype=np.int32)
    zero = np.zeros(n, dtype=np.int64)
    out = dict(samples=L, reads=n, reps=reps, dtype=np.dtype(dtype).name, resident=True)
    n_out = -(-L // 10)
    d, d_out, d_pool = eng.dev_alloc(x.nbytes), eng.dev_alloc(x.nbytes), eng.dev_alloc(n * n_out * esz)
    try:
        eng.h2d(d, x)
        kw = dict(n=n, L=L, dtype=dtype)
        forms = {
            "partitions": lambda: sp.calc_partitions_from_vals_batch(d, lens, zero, ae, pe, **kw),
            "real_range": lambda: real_range.real_range_check_batch(d, lens, zero, ae, RealRangeConfig(), **kw),
            "open_pores": lambda: anomalies.find_open_pores_batch(d, lens, zero, ae, **kw),
            "med_mad_rows": lambda: normalize.med_mad_batch(d, lens, True, **kw),
            "normalize_rows": lambda: normalize.normalize_signal_batch(d, lens, 5.0, True, out=d_out, **kw),
            "pool_10": lambda: downscale.efficient_average_pooling_device(d, n, L, 10, dtype, out=d_pool),
            "normalize_whole": lambda: eng.normalize(d, None, 5.0, True, True, n=n, L=L, f64=esz == 8, out_ptr=d_out),
        }
        passes = 2 + 2 * esz  # (two sums, two selections of one pass per key byte)
        for name, fn in forms.items():
            wall, kt = _timed(eng, fn, reps)
            out[name] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall, kernel_ms=kt)
            if name == "partitions":
                out[name]["k_seg_stats_read_TB_per_s"] = passes * x.nbytes / (kt["k_seg_stats"] * 1e-3) / 1e12
            if name == "normalize_whole":
                out[name]["k_pop_hist_read_TB_per_s"] = 2 * esz * x.nbytes / (kt["k_pop_hist"] * 1e-3) / 1e12
                out[name]["k_clip_scale_read_TB_per_s"] = x.nbytes / (kt["k_clip_scale"] * 1e-3) / 1e12
    finally:
        for p in (d, d_out, d_pool):
            eng.dev_free(p)
    return out


def sweep(reps, dtype=np.float32):
    """median / MAD of one resident population: one wave against many workgroups"""
    from adapted_amd.detect._rows import _engine

    eng = _engine()
    rng = np.random.default_rng(5)
    rows = []
    for e in range(12, 25):
        N = 1 << e
        x = rng.normal(90.0, 12.0, N).astype(dtype).reshape(1, -1)
        d = eng.dev_alloc(x.nbytes)
        try:
            eng.h2d(d, x)
            row = dict(samples=N, dtype=np.dtype(dtype).name)
            for regime in ("wave", "grid"):
                if regime == "wave" and N > (1 << 22):
                    continue
                wall, kt = _timed(eng, lambda: eng.med_mad(d, None, True, True, n=1, L=N, f64=x.dtype.itemsize == 8, regime=regime), reps)
                row[regime + "_wall_ms"] = wall * 1e3
                row[regime + "_kernel_ms"] = sum(kt.values())
            rows.append(row)
        finally:
            eng.dev_free(d)
    return rows


def reference(n, L):
    from oracle import ref_harness

    ref_harness.install()
    from adapted.config.sig_proc import RealRangeConfig
    from adapted.detect.anomalies import find_open_pores
    from adapted.detect.downscale import downscale_signal
    from adapted.detect.normalize import normalize_signal
    from adapted.detect.real_range import real_range_check
    from adapted.partition.signal_partitions import calc_partitions_from_vals

    x, ae, pe = reads(n, L)
    out = dict(samples=L, reads=n, dtype="float32", where="the build container, one CPU core", numpy=np.__version__)
    warnings.simplefilter("ignore")
    for name, fn in (("partitions", lambda r: calc_partitions_from_vals(x[r], 0, int(ae[r]), int(pe[r]))),
                     ("real_range", lambda r: real_range_check(x[r, :ae[r]], RealRangeConfig(), True)),
                     ("open_pores", lambda r: find_open_pores(x[r, :ae[r]])),
                     ("normalize_rows", lambda r: normalize_signal(x[r], 5.0, True)),
                     ("pool_10", lambda r: downscale_signal(x[r:r + 1], 10))):
        t = time.perf_counter()
        for r in range(n):
            fn(r)
        wall = time.perf_counter() - t
        out[name] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall)
    t = time.perf_counter()
    normalize_signal(x, 5.0, True)
    wall = time.perf_counter() - t
    out["normalize_whole"] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reference:
        res = [reference(min(a.reads, 400), 16_000), reference(min(a.reads, 100), 200_000)]
    elif a.sweep:
        res = sweep(a.reps, np.dtype(a.dtype))
    else:
        res = [device(a.reads, 16_000, a.reps, np.dtype(a.dtype)), device(a.reads, 200_000, a.reps, np.dtype(a.dtype))]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
