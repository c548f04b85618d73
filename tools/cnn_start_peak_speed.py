#!/usr/bin/env python3
"""Time adp_detect_cnn without and with the start-peak overlay (ADP_WITH_START_PEAK) on resident synthetic reads (GPU box): the
step bench.py times for --primary cnn (detect_rows_device over the resident batch, rows copied to a device row buffer).  Three
modes ALTERNATE in one process per workload -- flag off, the fused form (K1 riding k_cnn_pool), ADP_SP_FUSED=0 (k_start_peak on
the side stream) -- then one profiled step per mode for the per-kernel HIP-event times of k_cnn_pool, k_sp_head, k_sp_tail and
k_start_peak.  The driver starts one worker process per workload under a time limit of its own and stops at the first that fails.
usage: python tools/cnn_start_peak_speed.py [--reads 4000] [--minibatch 1000] [--steps 6] [--warmup 2] [--seed 2024] [--limit 240]
prints one JSON line per workload (200 k window / default window)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"200k_full": 200000, "default_full": None}
MODES = ("off", "fused", "side_stream")
KERNELS = ("k_cnn_pool", "k_sp_head", "k_sp_tail", "k_start_peak")


def worker(name, a):
    import numpy as np
    import torch

    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.detect import cnn

    torch.cuda.init()
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = False, True
    if WORKLOADS[name]:
        spc.core.max_obs_trace = WORKLOADS[name]
    spc.update_primary_method()
    spc.update_sig_preload_size()
    m, R, mb = spc.sig_preload_size, a.reads, a.minibatch
    dev = torch.device("cuda", 0)
    eng = lib.Engine(spc, R, m, device=0)
    lens = np.full(R, m, dtype=np.int32)
    sig_t = torch.empty((R, m), dtype=torch.float32, device=dev)
    len_t = torch.from_numpy(lens).to(dev)
    rows_t = torch.empty((R, lib.ROW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.synth_fill(sig_t.data_ptr(), len_t.data_ptr(), R, seed=a.seed, first_read=0, decorate=True)

    def step(mode):
        os.environ["ADP_SP_FUSED"] = "0" if mode == "side_stream" else "1"  # (read by the library at every call)
        fn = cnn.detect_rows_device if mode == "off" else cnn.detect_rows_device_start_peak
        rows = fn(eng, sig_t.data_ptr(), len_t.data_ptr(), R, lens, None, spc, minibatch=mb)
        eng.h2d(rows_t.data_ptr(), rows)
        return rows

    for _ in range(a.warmup):
        for mode in MODES:
            step(mode)
    ms = {k: [] for k in MODES}
    rows = {}
    for _ in range(a.steps):
        for mode in MODES:  # alternated: all see the same placement of the signal buffer's pages
            t0 = time.perf_counter()
            rows[mode] = step(mode)
            ms[mode].append((time.perf_counter() - t0) * 1e3)
    digest, kernel_ms = {}, {}
    for mode in MODES:
        r = rows[mode].copy()
        r["open_pores_more"] = 0
        digest[mode] = hashlib.sha256(r.tobytes()).hexdigest()
        eng.set_profiling(True)
        step(mode)
        t = {}
        for k, v in eng.kernel_times():
            if k in KERNELS:
                t[k] = round(t.get(k, 0.0) + v, 3)
        t["all_kernels"] = round(sum(v for _, v in eng.kernel_times()), 3)
        kernel_ms[mode] = t
        eng.set_profiling(False)
    sp_cols = [lib.COLS.index(c) for c in ("start_peak_idx", "start_peak_pa", "start_peak_next_max_idx", "start_peak_next_max_pa", "start_peak_open_pore_idx")]
    bare = rows["fused"].copy()
    bare["col"][:, sp_cols] = 0.0
    bare["present"] &= ~np.uint64(sum(1 << c for c in sp_cols))
    bare["start_peak_type"] = 0
    bare["open_pores_more"] = 0
    off0 = rows["off"].copy()
    off0["open_pores_more"] = 0
    out = dict(workload=name, m=int(m), reads=R, minibatch=mb, steps=a.steps,
               ms={k: [round(x, 3) for x in v] for k, v in ms.items()},
               ms_median={k: round(float(np.median(v)), 3) for k, v in ms.items()},
               rows_sha256=digest, forms_equal=bool(digest["fused"] == digest["side_stream"]),
               other_bytes_equal_flag_off=bool(bare.tobytes() == off0.tobytes()),
               rows_with_fields=int(((rows["fused"]["present"] >> np.uint64(sp_cols[0])) & np.uint64(1)).sum()),
               flagged=int((rows["fused"]["start_peak_type"] != 0).sum()), kernel_ms=kernel_ms)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--limit", type=int, default=240, help="seconds a workload's process may take")
    ap.add_argument("--only", type=str, default=None, help="comma-separated workload names")
    ap.add_argument("--workload", type=str, default=None, help="(the worker: run this workload in this process)")
    a = ap.parse_args()
    if a.workload:
        worker(a.workload, a)
        return 0
    for name in WORKLOADS:
        if a.only and name not in a.only.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", name] + [x for k in ("reads", "minibatch", "steps", "warmup", "seed")
                                                                                 for x in ("--" + k, str(getattr(a, k)))]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:  # a workload that failed or ran out of time: nothing more is started on the device
            print(json.dumps({"workload": name, "failed": rc}), flush=True)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
