#!/usr/bin/env python3
"""Rates of the template building (adp_dtw_align, adp_dba_step: adapted_amd/csrc/dtw_align_api.h), the fingerprints resident in HBM.

align: 96 000 fingerprints of 110 events, warped noisy copies of 12 base sequences, each against the template of its own label --
k_dtw_align's cells/s beside k_dtw's on the SAME pairs in the same process (adp_dtw_assign per label with that label's one
template; the queries are sorted by label, so a label's queries are one slice of the resident array).  The ratio is what the
direction codes, the serial walk back and the run sums cost.  Per-kernel times from adp_kernel_times (HIP events on the handle's
stream, summed over a call's batches).
build: one whole barcode_templates.dba_templates over 12 labels x 8 000 members, 10 iterations at the most, init_sample 256: wall
time, and the part of it in the medoids' start.

  python tools/dtw_align_speed.py [--reps R] [--small] [--out FILE]   (default FILE: profiles/dtw_align_speed.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fingerprint_module_speed import timed  # noqa: E402


def copies(labels, per, E, seed=5):
    """-> (fingerprints [labels * per, E] NaN beyond counts, counts, label of every row): sorted by label"""
    rng = np.random.default_rng(seed)
    fp = np.full((labels * per, E), np.nan)
    counts = np.zeros(labels * per, dtype=np.int32)
    for k in range(labels):
        base = 2.0 * rng.standard_normal(int(E * 0.7))
        for r in range(k * per, (k + 1) * per):
            x = np.repeat(base, rng.integers(1, 3, base.size))[:E]
            fp[r, :x.size] = x + 0.3 * rng.standard_normal(x.size)
            counts[r] = x.size
    return fp, counts, np.repeat(np.arange(labels), per)


def align(eng, labels, per, E, band, reps):
    fp, counts, lab = copies(labels, per, E)
    nq = fp.shape[0]
    first = [k * per for k in range(labels)]
    t, tc = np.where(np.isnan(fp[first]), 0.0, fp[first]), counts[first].copy()
    which = lab.astype(np.int32)
    out = dict(call="dtw_align", queries=nq, templates=labels, events=E, band=band, reps=reps, resident=True)
    q_d, qc_d = eng.dev_alloc(fp.nbytes), eng.dev_alloc(counts.nbytes)
    try:
        eng.h2d(q_d, fp)
        eng.h2d(qc_d, counts)
        wall, kt = timed(eng, lambda: eng.dtw_align(q_d, qc_d, which, t, tc, band, nq=nq, Eq=E, want_path=False), reps)
        wall_path, _ = timed(eng, lambda: eng.dtw_align(q_d, qc_d, which, t, tc, band, nq=nq, Eq=E), reps)
        step_wall, step_kt = timed(eng, lambda: eng.dba_step(q_d, qc_d, which, t, tc, band, nq=nq, Eq=E), reps)
        got = eng.dtw_align(q_d, qc_d, which, t, tc, band, nq=nq, Eq=E, want_path=False)

        def assign_same_pairs():
            return [eng.dtw_assign(q_d + k * per * E * 8, qc_d + k * per * 4, t[k:k + 1], tc[k:k + 1], band, nq=per, Eq=E)[0][:, 0] for k in range(labels)]

        # (adp_kernel_times reports the last call: the labels' calls are profiled one by one)
        assign_wall, _ = timed(eng, assign_same_pairs, reps)
        k_dtw_ms = 0.0
        for k in range(labels):
            _, one = timed(eng, lambda: eng.dtw_assign(q_d + k * per * E * 8, qc_d + k * per * 4, t[k:k + 1], tc[k:k + 1], band, nq=per, Eq=E), 1)
            k_dtw_ms += one["k_dtw"]
        same = bool(np.array_equal(np.concatenate(assign_same_pairs()).view(np.uint64), got["dist"].view(np.uint64)))
    finally:
        eng.dev_free(q_d)
        eng.dev_free(qc_d)
    # (both kernels visit every cell of the rows 1 .. n over the width of the template's lanes: the rate counts n x m)
    cells = int((counts.astype(np.int64) * tc[which]).sum())
    out.update(wall_ms=wall * 1e3, wall_ms_with_paths_copied=wall_path * 1e3, kernel_ms=kt, cells=cells,
               cells_per_s_k_dtw_align=cells / (kt["k_dtw_align"] * 1e-3), k_dtw_ms_same_pairs=k_dtw_ms, assign_wall_ms_same_pairs=assign_wall * 1e3,
               cells_per_s_k_dtw=cells / (k_dtw_ms * 1e-3), k_dtw_align_over_k_dtw_time=kt["k_dtw_align"] / k_dtw_ms,
               distances_equal_adp_dtw_assign=same, dba_step_wall_ms=step_wall * 1e3, dba_step_kernel_ms=step_kt,
               status_counts={str(s): int((got["status"] == s).sum()) for s in np.unique(got["status"])})
    return out


def build(labels, per, E, band, iters):
    from adapted_amd import barcode_templates as bt

    fp, counts, lab = copies(labels, per, E, seed=6)
    names = np.asarray(["bc%02d" % k for k in lab])
    bt.dba_templates(fp[::per // 4], counts[::per // 4], names[::per // 4], band=band, iters=1, init_sample=4)  # warm-up
    t0 = time.perf_counter()
    bt.dba_templates(fp, counts, names, band=band, iters=0, init_sample=256)
    start = time.perf_counter() - t0
    t0 = time.perf_counter()
    tm, info = bt.dba_templates(fp, counts, names, band=band, iters=iters, init_sample=256)
    wall = time.perf_counter() - t0
    tot = info["inertia"].sum(axis=1)
    return dict(call="dba_templates", labels=labels, members_per_label=per, events=E, band=band, iters_allowed=iters, init_sample=256,
                iterations=int(info["iterations"]), wall_s=wall, start_medoids_wall_s=start, per_iteration_ms=(wall - start) / max(info["iterations"], 1) * 1e3,
                inertia_first=float(tot[0]), inertia_last=float(tot[-1]), members=info["members"].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a hundredth of the members (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_align_speed.json"))
    a = ap.parse_args()
    from adapted_amd.detect._rows import _engine

    eng = _engine()
    per = 80 if a.small else 8_000
    res = [align(eng, 12, per, 110, band, a.reps) for band in (0, 10)] + [build(12, per, 110, 0, 10)]
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
