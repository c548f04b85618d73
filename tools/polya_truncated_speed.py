#!/usr/bin/env python3
"""Time adp_detect_llr with and without the truncation look (ADP_FLAG_TRUNCATED) on resident synthetic reads (GPU box): the step
bench.py times for the LLR primary (detect_llr_rows over the resident batch into a device row buffer, start-peak columns on,
ADP_TAILS_NAN), flag off and on ALTERNATED in one process, then one profiled step with the flag on.
Workloads: bench.py's headline (200 k window) and llr_default_window (max_obs_trace 16 000), each with the benchmark's own
lengths (full_len == m: no read is eligible, the look is the eligibility test alone) and with full_len = m + 1 (every read with an
adapter is eligible: the tail test T1 runs on all of them; the synthetic reads end in RNA, so none passes it and T2 never runs).
usage: python tools/polya_truncated_speed.py [--reads 96000] [--minibatch 1000] [--steps 6] [--warmup 1] [--seed 2024] [--only names]
prints one JSON line per workload"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adapted_amd import lib  # noqa: E402
from adapted_amd.config import get_chemistry_specific_config  # noqa: E402


def make_spc(max_obs_trace):
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.core.max_obs_trace = max_obs_trace
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


def workload(name, max_obs_trace, beyond, a):
    spc = make_spc(max_obs_trace)
    m, R, mb = spc.sig_preload_size, a.reads, a.minibatch
    dev = torch.device("cuda", 0)
    eng = lib.Engine(spc, R, m, device=0)
    sig_t = torch.empty((R, m), dtype=torch.float32, device=dev)
    len_t = torch.from_numpy(np.full(R, m, dtype=np.int32)).to(dev)
    rows_t = torch.empty((R, lib.ROW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.synth_fill(sig_t.data_ptr(), len_t.data_ptr(), R, seed=a.seed, first_read=0, decorate=True)
    if beyond:  # the same samples, the reads going on behind the window
        len_t += beyond
        torch.cuda.synchronize()

    def step(flag):
        eng.detect_llr_rows(sig_t.data_ptr(), len_t.data_ptr(), R, mb, with_start_peak=True, device_ptrs=True, rows_dev=rows_t.data_ptr(),
                            tails_nan=True, flag_truncated=flag)

    for _ in range(a.warmup):
        for flag in (False, True):
            step(flag)
    ms = {False: [], True: []}
    rows = {}
    for _ in range(a.steps):
        for flag in (False, True):  # alternated: both see the same placement of the signal buffer's pages
            t0 = time.perf_counter()
            step(flag)
            ms[flag].append((time.perf_counter() - t0) * 1e3)
            rows[flag] = rows_t.cpu().numpy().view(lib.ROW_DTYPE).reshape(-1).copy()
    counts = eng.debug_truncated()
    eng.set_profiling(True)
    step(True)
    times = {}
    for k, v in eng.kernel_times():
        times[k] = round(times.get(k, 0.0) + v, 3)
    eng.set_profiling(False)
    on, off = rows[True].copy(), rows[False].copy()
    digest_off = hashlib.sha256(off.tobytes()).hexdigest()
    looked = bool(((on["reserved_"] & lib.ROW_TRUNC_LOOKED) != 0).all())
    on["reserved_"] &= ~lib.ROW_TRUNC_LOOKED
    keep = (on["reserved_"] & lib.ROW_POLYA_TRUNCATED) == 0
    out = dict(workload=name, m=int(m), reads=R, minibatch=mb, steps=a.steps, full_len=int(m + beyond),
               ms_off=[round(x, 3) for x in ms[False]], ms_on=[round(x, 3) for x in ms[True]],
               ms_off_median=round(float(np.median(ms[False])), 3), ms_on_median=round(float(np.median(ms[True])), 3),
               rows_sha256_off=digest_off, pass_off=int(off["success"].sum()), pass_on=int(on["success"].sum()),
               every_row_marked_looked=looked, unflagged_rows_equal=bool(on[keep].tobytes() == off[keep].tobytes()),
               counts=dict(zip(("eligible", "t1_passed", "replaced"), counts)),
               kernel_ms_on={k: v for k, v in times.items() if k.startswith("k_pt_")}, kernel_ms_on_total=round(sum(times.values()), 3))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=96000)
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--only", type=str, default=None, help="comma-separated workload names")
    a = ap.parse_args()
    torch.cuda.init()
    for name, mot, beyond in (("headline", 200000, 0), ("headline_beyond", 200000, 1), ("llr_default_window", 16000, 0),
                              ("llr_default_window_beyond", 16000, 1)):
        if a.only and name not in a.only.split(","):
            continue
        print(json.dumps(workload(name, mot, beyond, a)), flush=True)


if __name__ == "__main__":
    main()
