#!/usr/bin/env python3
"""Segments/s of the event segmentation (adp_segment_events: adapted_amd/csrc/events_api.h) with float32 samples resident in HBM:
96 000 segments of 3 500 samples (one adapter per read of a detect call's batch) and 2 000 of 200 000 (whole reads at the long
window), one segment per row, default parameters.  Per-kernel times from adp_kernel_times (HIP events on the handle's stream; a call
runs its two kernels once per batch of slots, the times are summed), effective GB/s = the samples' bytes over the score kernel's time,
and beside them the numpy + scipy oracle (tests/events_oracle.py) on one CPU core over a few of the same segments.

  python tools/events_module_speed.py [--reps R] [--small] [--out FILE]     (default FILE: profiles/events_module_speed.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import events_oracle as eo  # noqa: E402


def rows(n, L, seed=3, distinct=64):
    """float32 [n, L]: `distinct` staircases (levels N(85, 12^2), dwells of 5 .. 40 samples, noise sd 2), repeated"""
    rng = np.random.default_rng(seed)
    base = np.stack([eo.staircase(rng, L) for _ in range(min(distinct, n))])
    return np.ascontiguousarray(np.resize(base, (n, L)))


def device(n, L, reps, oracle_segments):
    from adapted_amd.detect._rows import _engine
    from adapted_amd.polya_length import EventParams

    eng = _engine()
    x = rows(n, L)
    lens = np.full(n, L, dtype=np.int32)
    idx, starts, ends = np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int64), np.full(n, L, dtype=np.int64)
    p = EventParams()
    a = p.args()
    out = dict(samples=L, segments=n, reps=reps, dtype="float32", resident=True, window=p.window, min_distance=p.min_distance,
               threshold=p.threshold)
    d = eng.dev_alloc(x.nbytes)
    try:
        eng.h2d(d, x)

        def call():
            return eng.segment_events(d, lens, idx, starts, ends, a, cap=0, n=n, L=L)

        _, info, stats = call()  # warm-up
        eng.set_profiling(False)
        t = time.perf_counter()
        for _ in range(reps):
            call()
        wall = (time.perf_counter() - t) / reps
        eng.set_profiling(True)
        call()
        kt = {}
        for k, ms in eng.kernel_times():
            kt[k] = kt.get(k, 0.0) + ms
        eng.set_profiling(False)
    finally:
        eng.dev_free(d)
    kernels = sum(kt.values())
    out.update(wall_ms=wall * 1e3, kernel_ms=kt, kernels_ms=kernels, segments_per_s=n / wall, segments_per_s_kernels=n / (kernels * 1e-3),
               effective_gb_per_s_scores=x.nbytes / (kt["k_ev_scores"] * 1e-3) / 1e9, effective_gb_per_s_kernels=x.nbytes / (kernels * 1e-3) / 1e9,
               boundaries_mean=float(info[:, 0].mean()), median_gap_mean=float(np.nanmean(stats[:, 0])))
    # the oracle on one CPU core, and the device's answers beside it
    k = min(oracle_segments, n)
    t = time.perf_counter()
    want = [eo.segment(x[r], p.window, p.min_distance, p.threshold, p.var_floor) for r in range(k)]
    cpu = time.perf_counter() - t

    def same(u, v):
        return u == v or (u != u and v != v)

    out.update(oracle_segments=k, oracle_segments_per_s=k / cpu, speedup_vs_oracle=(n / wall) / (k / cpu),
               oracle_agrees=all(int(info[r, 0]) == want[r][0].size and same(stats[r, 0], want[r][2]) and same(stats[r, 1], want[r][3]) for r in range(k)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a hundredth of the segments (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_module_speed.json"))
    a = ap.parse_args()
    f = 100 if a.small else 1
    res = [device(96_000 // f, 3_500, a.reps, 200), device(2_000 // f, 200_000, a.reps, 8)]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
