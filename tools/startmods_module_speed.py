#!/usr/bin/env python3
"""Reads/s of the start-peak and adapter-start modules' batch forms (adp_start_peak, adp_adapter_start: adapted_amd/csrc/
startmods_api.h) with float32 (or, --dtype float64, float64) reads resident in HBM, at 16 000 and 200 000 samples; per-kernel
times from adp_kernel_times (HIP events on the handle's stream).  The reads: a high level, then the adapter's lower one, off
the 0.25 pA grid; a start peak in front.

  python tools/startmods_module_speed.py [--reads N] [--reps R] [--dtype float32|float64] [--out FILE]
  python3.9 tools/startmods_module_speed.py --reference [--out FILE]   (build container only: the reference's modules with the
                                                                        real bottleneck and pandas on one CPU core, same reads)"""
import argparse
import json
import os
import sys
import time
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import startmods_module_cases as M  # noqa: E402


def reads(n, L, seed=3):
    """float32 [n, L]: 16 base reads, each row with its own level change"""
    rng = np.random.default_rng(seed)
    base = [M.noisy_read(s, L, 0).astype(np.float32) for s in range(16)]
    x = np.empty((n, L), dtype=np.float32)
    for r in range(n):
        x[r] = base[r % 16]
        d = int(rng.integers(L // 8, L // 2))
        x[r, :d] += np.float32(42.0)
        x[r, 300:320] += np.float32(70.0)
    return x


def device(n, L, reps, dtype=np.float32):
    from adapted_amd.config.schema import MMAdapterStartConfig, RNAStartPeakConfig
    from adapted_amd.detect import adapter_start, start_peak
    from adapted_amd.detect._rows import _engine

    eng = _engine()
    x = reads(n, L).astype(dtype, copy=False)
    lens = np.full(n, L, dtype=np.int32)
    out = dict(samples=L, reads=n, reps=reps, dtype=np.dtype(dtype).name, resident=True)
    d = eng.dev_alloc(x.nbytes)
    try:
        eng.h2d(d, x)
        forms = {
            "adapter_start": lambda: adapter_start.moving_mean_adapter_start_detect_batch(d, lens, MMAdapterStartConfig(), n=n, L=L, dtype=dtype)[0],
            "start_peak": lambda: start_peak.detect_rna_start_peak_batch(d, lens, RNAStartPeakConfig(), n=n, m=L, dtype=dtype)["valid"],
        }
        for name, fn in forms.items():
            res = fn()  # warm-up
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
            out[name] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall, kernel_ms=kt, found=int((res > 0).sum()))
    finally:
        eng.dev_free(d)
    return out


def reference(n, L):
    from oracle import ref_harness

    ref_harness.install()
    import bottleneck
    import pandas
    from adapted.config.sig_proc import MMAdapterStartConfig, RNAStartPeakConfig
    from adapted.detect import adapter_start as ref_as
    from adapted.detect import start_peak as ref_sp

    x = reads(n, L)
    lens = np.full(n, L, dtype=np.int64)
    out = dict(samples=L, reads=n, dtype="float32", where="the build container, one CPU core", numpy=np.__version__,
               bottleneck=bottleneck.__version__, pandas=pandas.__version__)
    warnings.simplefilter("ignore")
    t = time.perf_counter()
    found = sum(int(ref_as.moving_mean_adapter_start_detect(x[r], MMAdapterStartConfig()) > 0) for r in range(n))
    wall = time.perf_counter() - t
    out["adapter_start"] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall, found=found)
    t = time.perf_counter()
    df = ref_sp.detect_rna_start_peak(x, lens, types.SimpleNamespace(rna_start_peak=RNAStartPeakConfig()))
    wall = time.perf_counter() - t
    out["start_peak"] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall, found=int(df.start_peak_idx.notna().sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reference:
        res = [reference(min(a.reads, 400), 16_000), reference(min(a.reads, 100), 200_000)]
    else:
        res = [device(a.reads, 16_000, a.reps, np.dtype(a.dtype)), device(a.reads, 200_000, a.reps, np.dtype(a.dtype))]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
