#!/usr/bin/env python3
"""Rates of the adapter event fingerprints and their DTW barcode assignment (adp_event_levels, adp_dtw_assign:
adapted_amd/csrc/fingerprint_api.h), everything resident in HBM.

event_levels: 96 000 segments of 3 500 float32 samples at E = 110, and 2 000 of 200 000 at E = 512, with adp_segment_events timed
beside each in the same process: the difference is what k_ev_levels and the copies of the event tables add.
dtw_assign: 96 000 resident fingerprints of 110 events against 12 and against 96 templates of 110 events, band 0 and 10 -- cells/s,
and their share of what 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz would allow at about 6 float64 operations per cell (a YARDSTICK of
the issue rate, as DESIGN.md uses for k_gains, not a bar: the lanes' pipeline fill, the lane shifts and the band test are not in it).
Per-kernel times from adp_kernel_times (HIP events on the handle's stream, summed over a call's batches).  With --oracle the numpy
oracle (tests/fingerprint_oracle.py) on one CPU core over a few of the same segments and pairs, and whether it agrees.

  python tools/fingerprint_module_speed.py [--reps R] [--small] [--oracle] [--out FILE]   (default FILE: profiles/fingerprint_module_speed.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fingerprint_oracle as fo  # noqa: E402
from events_module_speed import rows  # noqa: E402

F64_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9
OPS_PER_CELL = 6


def timed(eng, call, reps):
    """-> (wall seconds per call, {kernel: ms} of one profiled call)"""
    call()  # warm-up
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
    return wall, kt


def levels(eng, n, L, E, reps, oracle_segments):
    from adapted_amd.polya_length import EventParams

    x = rows(n, L)
    lens = np.full(n, L, dtype=np.int32)
    idx, starts, ends = np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int64), np.full(n, L, dtype=np.int64)
    p = EventParams()
    a = p.args()
    out = dict(call="event_levels", samples=L, segments=n, max_events=E, reps=reps, dtype="float32", resident=True)
    d, fp_d, cnt_d = eng.dev_alloc(x.nbytes), eng.dev_alloc(n * E * 8), eng.dev_alloc(n * 4)
    try:
        eng.h2d(d, x)
        seg_wall, seg_kt = timed(eng, lambda: eng.segment_events(d, lens, idx, starts, ends, a, cap=0, n=n, L=L), reps)
        wall, kt = timed(eng, lambda: eng.event_levels(d, lens, idx, starts, ends, a, E, n=n, L=L), reps)
        dev_wall, _ = timed(eng, lambda: eng.event_levels(d, lens, idx, starts, ends, a, E, n=n, L=L, fp_ptr=fp_d, count_ptr=cnt_d), reps)
        got = eng.event_levels(d, lens, idx, starts, ends, a, E, n=n, L=L)
    finally:
        for ptr in (d, fp_d, cnt_d):
            eng.dev_free(ptr)
    out.update(wall_ms=wall * 1e3, wall_ms_fingerprints_left_on_device=dev_wall * 1e3, segment_events_wall_ms=seg_wall * 1e3,
               added_ms=(wall - seg_wall) * 1e3, kernel_ms=kt, segment_events_kernel_ms=seg_kt, segments_per_s=n / wall,
               events_mean=float(got["count"].mean()), boundaries_mean=float(got["info"][:, 0].mean()),
               status_counts={str(k): int((got["status"] == k).sum()) for k in np.unique(got["status"])})
    if oracle_segments:
        k = min(oracle_segments, n)
        t = time.perf_counter()
        want = [fo.levels(x[r], E, p.window, p.min_distance, p.threshold, p.var_floor) for r in range(k)]
        cpu = time.perf_counter() - t
        out.update(oracle_segments=k, oracle_segments_per_s=k / cpu, speedup_vs_oracle=(n / wall) / (k / cpu),
                   oracle_agrees=all(fo.same(got["fingerprints"][r], want[r]["fp"]) and fo.same(got["levels"][r], want[r]["levels"])
                                     and got["lengths"][r].tolist() == want[r]["lengths"].tolist() for r in range(k)))
    return out


def dtw(eng, nq, nt, E, band, reps, oracle_pairs):
    rng = np.random.default_rng(5)
    q = np.cumsum(rng.normal(0.0, 1.0, (nq, E)), axis=1) * 0.3 + rng.normal(0.0, 1.0, (nq, E))
    t = np.ascontiguousarray(q[rng.choice(nq, nt, replace=False)] + rng.normal(0.0, 0.1, (nt, E)))
    qc, tc = np.full(nq, E, dtype=np.int32), np.full(nt, E, dtype=np.int32)
    out = dict(call="dtw_assign", queries=nq, templates=nt, events=E, band=band, reps=reps, resident=True)
    q_d, qc_d = eng.dev_alloc(q.nbytes), eng.dev_alloc(qc.nbytes)
    try:
        eng.h2d(q_d, q)
        eng.h2d(qc_d, qc)
        wall, kt = timed(eng, lambda: eng.dtw_assign(q_d, qc_d, t, tc, band, nq=nq, Eq=E, want_dist=False), reps)
        k = min(oracle_pairs // nt + 1, nq) if oracle_pairs else 0
        dist, best, _ = eng.dtw_assign(q[:max(k, 1)], qc[:max(k, 1)], t, tc, band)
    finally:
        eng.dev_free(q_d)
        eng.dev_free(qc_d)
    # (k_dtw visits every cell of a pair and masks those outside the band: the rate counts the cells visited)
    cells = nq * nt * E * E
    in_band = nq * nt * (E * E if band == 0 else sum(min(E, i + band) - max(1, i - band) + 1 for i in range(1, E + 1)))
    rate = cells / (kt["k_dtw"] * 1e-3)
    out.update(wall_ms=wall * 1e3, kernel_ms=kt, pairs_per_s=nq * nt / wall, cells=cells, cells_in_band=in_band, cells_per_s_kernel=rate,
               share_of_f64_issue_yardstick=rate * OPS_PER_CELL / F64_LANE_OPS_PER_S)
    if k:
        t0 = time.perf_counter()
        want = fo.dtw(q[:k], qc[:k], t, tc, band)
        cpu = time.perf_counter() - t0
        out.update(oracle_pairs=k * nt, oracle_pairs_per_s=k * nt / cpu, speedup_vs_oracle=(nq * nt / wall) / (k * nt / cpu),
                   oracle_agrees=bool(fo.same(dist, want) and fo.same(best, fo.assign(want)[0])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a hundredth of the segments and queries (a quick look)")
    ap.add_argument("--oracle", action="store_true", help="also the numpy oracle on one CPU core, on a few hundred segments / pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fingerprint_module_speed.json"))
    a = ap.parse_args()
    from adapted_amd.detect._rows import _engine

    eng = _engine()
    f = 100 if a.small else 1
    res = [levels(eng, 96_000 // f, 3_500, 110, a.reps, 200 if a.oracle else 0), levels(eng, 2_000 // f, 200_000, 512, a.reps, 4 if a.oracle else 0)]
    for nt in (12, 96):
        for band in (0, 10):
            res.append(dtw(eng, 96_000 // f, nt, 110, band, a.reps, 300 if a.oracle else 0))
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
