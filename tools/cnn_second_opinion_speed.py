#!/usr/bin/env python3
"""Time adp_detect_cnn with and without the LLR second opinion (ADP_CNN_SECOND_LLR) on resident synthetic reads (GPU box): the
step bench.py times for --primary cnn (detect_rows_device over the resident batch, rows copied to a device row buffer), flag off
and on ALTERNATED in one process, then one profiled step with the flag on (per-kernel HIP-event times, the four counts).
usage: python tools/cnn_second_opinion_speed.py [--reads 4000] [--minibatch 1000] [--steps 6] [--warmup 2] [--seed 2024]
prints one JSON line per workload (200 k window / default window x full-length / Pareto lengths)"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adapted_amd import lib, synth  # noqa: E402
from adapted_amd.config import get_chemistry_specific_config  # noqa: E402
from adapted_amd.detect import cnn  # noqa: E402


def make_spc(max_obs_trace):
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = False, True
    if max_obs_trace:
        spc.core.max_obs_trace = max_obs_trace
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


def workload(name, max_obs_trace, pareto, a):
    spc = make_spc(max_obs_trace)
    m, R, mb = spc.sig_preload_size, a.reads, a.minibatch
    dev = torch.device("cuda", 0)
    eng = lib.Engine(spc, R, m, device=0)
    lens = np.full(R, m, dtype=np.int32)
    if pareto:
        lens = np.array([synth.pareto_length(a.seed, i) for i in range(R)], dtype=np.int32)
    sig_t = torch.empty((R, m), dtype=torch.float32, device=dev)
    len_t = torch.from_numpy(lens).to(dev)
    rows_t = torch.empty((R, lib.ROW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.synth_fill(sig_t.data_ptr(), len_t.data_ptr(), R, seed=a.seed, first_read=0, decorate=True)
    fns = {False: cnn.detect_rows_device, True: cnn.detect_rows_device_second_opinion}

    def step(flag):
        rows = fns[flag](eng, sig_t.data_ptr(), len_t.data_ptr(), R, lens, None, spc, minibatch=mb)
        eng.h2d(rows_t.data_ptr(), rows)
        return rows

    for _ in range(a.warmup):
        for flag in (False, True):
            step(flag)
    ms = {False: [], True: []}
    digest, counts, rows = {}, None, {}
    for _ in range(a.steps):
        for flag in (False, True):  # alternated: both see the same placement of the signal buffer's pages
            t0 = time.perf_counter()
            rows[flag] = step(flag)
            ms[flag].append((time.perf_counter() - t0) * 1e3)
    for flag in (False, True):
        r = rows[flag].copy()
        r["open_pores_more"] = 0
        digest[flag] = hashlib.sha256(r.tobytes()).hexdigest()
    counts = eng.debug_cnn_second_opinion()
    eng.set_profiling(True)
    step(True)
    times = {}
    for k, v in eng.kernel_times():
        times[k] = round(times.get(k, 0.0) + v, 3)
    eng.set_profiling(False)
    on, off = rows[True], rows[False]
    marked = (on["reserved_"] & lib.ROW_FROM_SECOND_LLR) != 0
    keep = ~marked
    on0, off0 = on.copy(), off.copy()
    on0["open_pores_more"] = 0
    off0["open_pores_more"] = 0
    out = dict(workload=name, m=int(m), reads=R, minibatch=mb, steps=a.steps,
               ms_off=[round(x, 3) for x in ms[False]], ms_on=[round(x, 3) for x in ms[True]],
               ms_off_median=round(float(np.median(ms[False])), 3), ms_on_median=round(float(np.median(ms[True])), 3),
               rows_sha256_off=digest[False], rows_sha256_on=digest[True],
               pass_off=int(off["success"].sum()), pass_on=int(on["success"].sum()), marked=int(marked.sum()),
               unmarked_rows_equal=bool(on0[keep].tobytes() == off0[keep].tobytes()),
               counts=dict(zip(("selected", "replaced", "still_failing", "minibatches_without"), counts)), kernel_ms_on=times)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--only", type=str, default=None, help="comma-separated workload names")
    a = ap.parse_args()
    torch.cuda.init()
    for name, mot, pareto in (("200k_full", 200000, False), ("200k_pareto", 200000, True), ("default_full", None, False), ("default_pareto", None, True)):
        if a.only and name not in a.only.split(","):
            continue
        print(json.dumps(workload(name, mot, pareto, a)), flush=True)


if __name__ == "__main__":
    main()
