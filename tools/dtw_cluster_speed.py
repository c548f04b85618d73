#!/usr/bin/env python3
"""Times of the clustering of fingerprints without labels (adp_dtw_pairwise, adp_kmedoids_build, adp_kmedoids, adp_silhouette:
adapted_amd/csrc/dtw_cluster_api.h).

pairwise: n = 4096 fingerprints of E = 110 events, counts ragged over 60 .. 110.  The baseline is the same matrix through
dtw_distances(q, q) -- adp_dtw_assign with the fingerprints as their own templates, every pair twice, the matrix brought to the
host.  Both run in ONE process, alternated, after a warm-up of each; the medians of the wall times (host clock around calls that
complete before they return) are reported, host to host for both, and the pairwise call with the matrix left on the device.  The
kernels' own times (HIP events, one profiled call each) stand beside them.  The two matrices are compared bit for bit.
sweep: BUILD to 24, then k-medoids and the silhouette for K = 2 .. 24, on the matrix resident on the device: wall time at n = 4096;
the same sweep on the numpy oracle (tests/dtw_cluster_oracle.py) at the first --oracle_n rows only (its explicit order of sums costs
minutes at 4096), beside the GPU on the same rows, the results compared.

  python tools/dtw_cluster_speed.py [--reps R] [--n N] [--oracle_n M] [--out FILE]   (default FILE: profiles/dtw_cluster_speed.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fingerprints(n, E, lo, seed=7, groups=12):
    """n warped noisy copies of ``groups`` base sequences, counts in [lo, E], zeros beyond"""
    rng = np.random.default_rng(seed)
    bases = 2.0 * rng.standard_normal((groups, E))
    q = np.zeros((n, E))
    counts = rng.integers(lo, E + 1, n).astype(np.int32)
    for p in range(n):
        b = bases[p % groups]
        x = np.repeat(b, rng.integers(1, 3, E))[:counts[p]]
        q[p, :counts[p]] = x + 0.3 * rng.standard_normal(counts[p])
    return q, counts


def kernel_ms(eng, call):
    eng.set_profiling(True)
    call()
    kt = {}
    for k, ms in eng.kernel_times():
        kt[k] = kt.get(k, 0.0) + ms
    eng.set_profiling(False)
    return kt


def pairwise(eng, n, E, lo, reps):
    from adapted_amd.fingerprint import dtw_distances

    q, counts = fingerprints(n, E, lo)
    out_d = eng.dev_alloc(n * n * 8)
    try:
        calls = {"dtw_distances_q_q": lambda: dtw_distances(q, counts, q, counts, 0, engine=eng),
                 "dtw_pairwise": lambda: eng.dtw_pairwise(q, counts, 0),
                 "dtw_pairwise_out_device": lambda: eng.dtw_pairwise(q, counts, 0, out_ptr=out_d)}
        for c in calls.values():  # warm-up
            c()
        walls = {name: [] for name in calls}
        for _ in range(reps):  # alternated
            for name, c in calls.items():
                t = time.perf_counter()
                c()
                walls[name].append(time.perf_counter() - t)
        kt = {name: kernel_ms(eng, c) for name, c in calls.items()}
        base, mine = calls["dtw_distances_q_q"](), calls["dtw_pairwise"]()
        left = np.zeros((n, n))
        eng.d2h(left, out_d)
    finally:
        eng.dev_free(out_d)
    med = {name: float(np.median(w)) for name, w in walls.items()}
    same = bool(np.array_equal(base.view(np.uint64), mine.view(np.uint64)) and np.array_equal(mine.view(np.uint64), left.view(np.uint64)))
    cells = int((counts.astype(np.int64)[:, None] * counts.astype(np.int64)[None, :]).sum())
    return dict(call="dtw_pairwise", n=n, events=E, counts=[int(counts.min()), int(counts.max())], band=0, reps=reps,
                wall_ms_median=dict((k, v * 1e3) for k, v in med.items()), wall_ms_all=dict((k, [x * 1e3 for x in v]) for k, v in walls.items()),
                kernel_ms=kt, pairwise_over_baseline_wall=med["dtw_pairwise"] / med["dtw_distances_q_q"],
                pairwise_out_device_over_baseline_wall=med["dtw_pairwise_out_device"] / med["dtw_distances_q_q"],
                k_dtw_pairs_over_k_dtw_kernel=kt["dtw_pairwise"]["k_dtw_pairs"] / kt["dtw_distances_q_q"]["k_dtw"],
                cells_all_ordered_pairs=cells, bits_equal=same), q, counts


def gpu_sweep(eng, D_ptr, n, kmin, kmax, iters):
    start, _ = eng.kmedoids_build(D_ptr, kmax, n=n)
    rows = []
    for K in range(kmin, kmax + 1):
        r = eng.kmedoids(D_ptr, start[:K], iters, n=n)
        sil = eng.silhouette(D_ptr, r["assign"], K, n=n)
        rows.append((K, float(r["cost"][-1]), float(np.mean(sil)), r["iters"], r["assign"]))
    return rows


def oracle_sweep(D, kmin, kmax, iters):
    import dtw_cluster_oracle as co

    start, _ = co.build(D, kmax)
    rows = []
    for K in range(kmin, kmax + 1):
        r = co.kmedoids(D, start[:K], iters)
        sil = co.silhouette(D, r["assign"], K)
        rows.append((K, float(r["cost"][-1]), float(np.mean(sil)), r["iters"], r["assign"]))
    return rows


def sweep(eng, q, counts, oracle_n, reps, kmin=2, kmax=24, iters=50):
    n = q.shape[0]
    out = dict(call="k_sweep", n=n, k=[kmin, kmax], max_iter=iters, reps=reps)
    D_d = eng.dev_alloc(n * n * 8)
    try:
        eng.dtw_pairwise(q, counts, 0, out_ptr=D_d)
        gpu_sweep(eng, D_d, n, kmin, kmax, iters)  # warm-up
        walls = []
        for _ in range(reps):
            t = time.perf_counter()
            rows = gpu_sweep(eng, D_d, n, kmin, kmax, iters)
            walls.append(time.perf_counter() - t)
        out.update(gpu_wall_ms_median=float(np.median(walls)) * 1e3, gpu_wall_ms_all=[w * 1e3 for w in walls],
                   iterations=[int(r[3]) for r in rows], silhouette_mean=[r[2] for r in rows])
    finally:
        eng.dev_free(D_d)
    m = min(oracle_n, n)
    D = eng.dtw_pairwise(q[:m], counts[:m], 0)
    gpu_sweep(eng, D, m, kmin, kmax, iters)  # warm-up
    t = time.perf_counter()
    got = gpu_sweep(eng, D, m, kmin, kmax, iters)
    gpu_s = time.perf_counter() - t
    t = time.perf_counter()
    want = oracle_sweep(D, kmin, kmax, iters)
    oracle_s = time.perf_counter() - t
    same = all(g[:4] == w[:4] and g[4].tolist() == w[4].tolist() for g, w in zip(got, want))
    out.update(oracle_n=m, oracle_wall_s=oracle_s, gpu_wall_s_same_rows_host_matrix=gpu_s, oracle_over_gpu=oracle_s / gpu_s, equal_to_oracle=bool(same))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--oracle_n", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_cluster_speed.json"))
    a = ap.parse_args()
    from adapted_amd.detect._rows import _engine

    eng = _engine()
    first, q, counts = pairwise(eng, a.n, 110, 60, a.reps)
    print(json.dumps(first), flush=True)
    second = sweep(eng, q, counts, a.oracle_n, a.reps)
    print(json.dumps(second), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump([first, second], fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
