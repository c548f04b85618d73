#!/usr/bin/env python3
"""Times of the k-nearest-neighbour search under DTW (adp_dtw_knn: adapted_amd/csrc/dtw_knn_api.h).

12288 references (12 groups x 1024) of E = 110 events, counts ragged over 60 .. 110, and 4096 queries of the same model
(tools/dtw_cluster_speed.py::fingerprints); band 0; k = 5 and k = 1.  Three ways to the same answer, asserted bit-identical here:
  (a) dtw_knn, pairs abandoned behind the lower bounds;
  (b) dtw_knn with ADP_KNN_NO_PRUNE: every pair to the end;
  (c) what there was before the call: dtw_distances in chunks of 4096 references -- the [nq, nr] matrix brought to the host -- and
      np.lexsort((index, distance)) per query there.
All run in ONE process, alternated, after a warm-up of each; the medians of the wall times (host clock around calls that complete
before they return, host to host) are reported, and the kernels' own times (HIP events, one profiled call each).  With them: the
share of the pairs abandoned and of the DP steps made, and the kernel's time at other periods of the abandon test
(ADP_KNN_CHECK_PERIOD) and other segment lengths (ADP_KNN_SEGMENT_REFS) -- the figures the defaults were chosen by.

  python tools/dtw_knn_speed.py [--reps R] [--nr N] [--nq N] [--out FILE]   (default FILE: profiles/dtw_knn_speed.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dtw_cluster_speed import fingerprints, kernel_ms  # noqa: E402


def by_matrix(eng, q, qc, r, rc, k, kt=None):
    """(c): the distance matrix in chunks of 4096 references, then the k least of every row by np.lexsort.  ``kt``: a dict the
    kernels' times of every chunk's call are added into (the engine keeps the last call's only)"""
    from adapted_amd.fingerprint import dtw_distances

    chunks = []
    for a in range(0, r.shape[0], 4096):
        chunks.append(dtw_distances(q, qc, r[a:a + 4096], rc[a:a + 4096], 0, engine=eng))
        if kt is not None:
            for name, ms in eng.kernel_times():
                kt[name] = kt.get(name, 0.0) + ms
    D = np.concatenate(chunks, axis=1)
    index = np.arange(D.shape[1])
    idx = np.stack([np.lexsort((index, row))[:k] for row in D]).astype(np.int32)
    return idx, np.take_along_axis(D, idx.astype(np.int64), axis=1)


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)))


def with_env(name, value, call):
    old = os.environ.get(name)
    os.environ[name] = str(value)
    try:
        return call()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def measure(eng, q, qc, r, rc, k, reps):
    calls = {"dtw_knn_pruned": lambda: eng.dtw_knn(q, qc, r, rc, k),
             "dtw_knn_no_prune": lambda: eng.dtw_knn(q, qc, r, rc, k, prune=False),
             "dtw_distances_lexsort": lambda: by_matrix(eng, q, qc, r, rc, k)}
    answers = {name: c() for name, c in calls.items()}  # warm-up
    assert same(answers["dtw_knn_pruned"], answers["dtw_knn_no_prune"]) and same(answers["dtw_knn_pruned"], answers["dtw_distances_lexsort"])
    walls = {name: [] for name in calls}
    for _ in range(reps):  # alternated
        for name, c in calls.items():
            t = time.perf_counter()
            got = c()
            walls[name].append(time.perf_counter() - t)
            assert same(got, answers[name])
    kt = {name: kernel_ms(eng, c) for name, c in calls.items() if name != "dtw_distances_lexsort"}
    kt["dtw_distances_lexsort"] = {}
    eng.set_profiling(True)
    by_matrix(eng, q, qc, r, rc, k, kt["dtw_distances_lexsort"])
    eng.set_profiling(False)
    work = eng.dtw_knn(q, qc, r, rc, k, want_work=True)[2].sum(axis=0)
    full = eng.dtw_knn(q, qc, r, rc, k, prune=False, want_work=True)[2].sum(axis=0)
    assert full[1] == 0 and work[0] + work[1] == full[0]
    med = {name: float(np.median(w)) for name, w in walls.items()}
    out = dict(call="dtw_knn", k=k, nq=int(q.shape[0]), nr=int(r.shape[0]), events=int(r.shape[1]), counts=[int(rc.min()), int(rc.max())], band=0,
               reps=reps, wall_ms_median=dict((n, v * 1e3) for n, v in med.items()),
               wall_ms_all=dict((n, [x * 1e3 for x in v]) for n, v in walls.items()), kernel_ms=kt,
               pruned_over_matrix_wall=med["dtw_knn_pruned"] / med["dtw_distances_lexsort"],
               no_prune_over_matrix_wall=med["dtw_knn_no_prune"] / med["dtw_distances_lexsort"],
               pruned_over_no_prune_kernel=kt["dtw_knn_pruned"]["k_dtw_knn"] / kt["dtw_knn_no_prune"]["k_dtw_knn"],
               k_dtw_knn_pruned_over_k_dtw=kt["dtw_knn_pruned"]["k_dtw_knn"] / kt["dtw_distances_lexsort"]["k_dtw"],
               pairs=int(full[0]), pairs_abandoned=int(work[1]), share_pairs_abandoned=float(work[1]) / float(full[0]),
               dp_steps_full=int(full[2]), dp_steps_made=int(work[2]), share_dp_steps_made=float(work[2]) / float(full[2]), bits_equal=True)
    # the two knobs: the kernel's time and the steps made (the answer asserted the same)
    sweeps = {"ADP_KNN_CHECK_PERIOD": [1, 2, 4, 8, 16, 32], "ADP_KNN_SEGMENT_REFS": [256, 1024, 4096, int(r.shape[0])]}
    for name, values in sweeps.items():
        rows = []
        for v in values:
            def call():
                got = eng.dtw_knn(q, qc, r, rc, k, want_work=True)
                assert same(got[:2], answers["dtw_knn_pruned"])
                return got[2].sum(axis=0)

            w = with_env(name, v, call)
            ms = with_env(name, v, lambda: kernel_ms(eng, lambda: eng.dtw_knn(q, qc, r, rc, k)))
            rows.append(dict(value=v, k_dtw_knn_ms=ms["k_dtw_knn"], k_knn_merge_ms=ms["k_knn_merge"], share_dp_steps_made=float(w[2]) / float(full[2]),
                             share_pairs_abandoned=float(w[1]) / float(full[0])))
        out["sweep_" + name] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nr", type=int, default=12288)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_knn_speed.json"))
    a = ap.parse_args()
    from adapted_amd.detect._rows import _engine

    eng = _engine()
    x, c = fingerprints(a.nr + a.nq, 110, 60)
    r, rc, q, qc = x[:a.nr], c[:a.nr], x[a.nr:], c[a.nr:]
    results = []
    for k in (5, 1):
        results.append(measure(eng, q, qc, r, rc, k, a.reps))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
