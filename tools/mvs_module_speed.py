#!/usr/bin/env python3
"""Reads/s of the MVS poly(A) module's batch forms (adp_mvs_check, adp_mvs_detect_at_loc, adp_mvs_detect:
adapted_amd/csrc/mvs_api.h) with float32 (or, --dtype float64, float64) reads resident in HBM, at 16 000 and 200 000 samples;
per-kernel times from adp_kernel_times (HIP events on the handle's stream).  check_whole: the check without windowed_stats, whose
mean and variance are numpy-ordered sums over the poly(A).  The reads: an adapter, a poly(A) at a depth of its own, RNA; every fifth
without a poly(A), so that the streaming walk runs to the read's end.

  python tools/mvs_module_speed.py [--reads N] [--reps R] [--dtype float32|float64] [--out FILE]
  python3.9 tools/mvs_module_speed.py --reference [--out FILE]   (build container only: the reference's mvs.py with the real
                                                                  bottleneck on one CPU core, on the same reads)"""
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
import mvs_module_cases as M  # noqa: E402


def reads(n, L, seed=3):
    """float32 [n, L], adapter end and poly(A) end per read"""
    rng = np.random.default_rng(seed)
    base = [M.pa_read(s, L, adapter=(3000, 3001), polya=(0, 1))[0].astype(np.float32) for s in range(16)]
    x = np.empty((n, L), dtype=np.float32)
    ae = np.zeros(n, dtype=np.int64)
    pe = np.zeros(n, dtype=np.int64)
    for r in range(n):
        x[r] = base[r % 16]
        d = int(rng.integers(3000, min(L - 3000, 12000))) if L > 16000 else int(rng.integers(3000, L - 3000))
        ae[r], pe[r] = d, d + 600
        if r % 5:
            x[r, d - 2000:d] = rng.normal(75.0, 6.0, 2000).astype(np.float32)
            x[r, d:d + 600] = rng.normal(110.0, 2.0, 600).astype(np.float32)
    return x, ae, pe


def device(n, L, reps, dtype=np.float32):
    from adapted_amd.config.schema import MVSPolyAConfig, StreamingConfig
    from adapted_amd.detect import mvs

    eng = mvs._engine()
    x, ae, pe = reads(n, L)
    x = x.astype(dtype, copy=False)
    lens = np.full(n, L, dtype=np.int32)
    out = dict(samples=L, reads=n, reps=reps, dtype=np.dtype(dtype).name, resident=True)
    d = eng.dev_alloc(x.nbytes)
    try:
        eng.h2d(d, x)
        kw = dict(n=n, L=L, dtype=dtype)
        forms = {
            "check": lambda: mvs.mean_var_shift_polyA_check_batch(d, lens, ae, pe, MVSPolyAConfig(), **kw),
            "check_whole": lambda: mvs.mean_var_shift_polyA_check_batch(d, lens, ae, pe, MVSPolyAConfig(), windowed_stats=False, **kw),
            "detect_at_loc": lambda: mvs.mean_var_shift_polyA_detect_at_loc_batch(d, lens, ae, MVSPolyAConfig(), **kw),
            "detect": lambda: mvs.mean_var_shift_polyA_detect_batch(d, lens, StreamingConfig(), **kw),
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
            out[name] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall, kernel_ms=kt)
            if name == "detect":
                out[name]["found"] = int((res > 0).sum())
    finally:
        eng.dev_free(d)
    return out


def reference(n, L):
    from oracle import ref_harness

    ref_harness.install()
    import bottleneck
    from adapted.config.sig_proc import MVSPolyAConfig, StreamingConfig
    from adapted.detect import mvs as ref

    x, ae, pe = reads(n, L)
    out = dict(samples=L, reads=n, dtype="float32", where="the build container, one CPU core", numpy=np.__version__,
               bottleneck=bottleneck.__version__)
    warnings.simplefilter("ignore")
    for name, fn in (("check", lambda r: ref.mean_var_shift_polyA_check(x[r], int(ae[r]), int(pe[r]), MVSPolyAConfig())),
                     ("detect_at_loc", lambda r: ref.mean_var_shift_polyA_detect_at_loc(x[r], int(ae[r]), MVSPolyAConfig())),
                     ("detect", lambda r: ref.mean_var_shift_polyA_detect(x[r], StreamingConfig()))):
        t = time.perf_counter()
        for r in range(n):
            fn(r)
        wall = time.perf_counter() - t
        out[name] = dict(wall_ms=wall * 1e3, reads_per_s=n / wall)
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
