#!/usr/bin/env python3
"""Time adp_detect_llr with and without the re-segmentation (ADP_LLR_RESEGMENT) on resident synthetic reads (GPU box): the step
bench.py times for the LLR primary at the default window (max_obs_trace 16 000: detect_llr_rows over the resident batch into a
device row buffer, start-peak columns on, ADP_TAILS_NAN), flag off and on ALTERNATED in one process, then one profiled step with
the flag on.  The batch is the benchmark's generator with every sixth read (r % 6 == 1) given the low stall of
tests/resegment_cases.py's kind 1: 55 + 2 N(0, 1) on [0, 1800 + 100 (r % 7)).
usage: python tools/resegment_speed.py [--reads 96000] [--minibatch 1000] [--steps 6] [--warmup 1] [--seed 2024] [--out FILE.json]
prints one JSON line: the added time per step, the time per selected read, the three counts"""
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


def make_spc():
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.core.max_obs_trace = 16000
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=96000)
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    torch.cuda.init()
    spc = make_spc()
    m, R, mb = spc.sig_preload_size, a.reads, a.minibatch
    dev = torch.device("cuda", 0)
    eng = lib.Engine(spc, R, m, device=0)
    sig_t = torch.empty((R, m), dtype=torch.float32, device=dev)
    len_t = torch.from_numpy(np.full(R, m, dtype=np.int32)).to(dev)
    rows_t = torch.empty((R, lib.ROW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.synth_fill(sig_t.data_ptr(), len_t.data_ptr(), R, seed=a.seed, first_read=0, decorate=True)
    eng.lib.adp_synchronize(eng._h)  # (the generator ran on the engine's stream; the stalls are written on torch's)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    for k in range(7):  # reads with r % 6 == 1 and r % 7 == k share a stall length
        r = torch.arange(R, device=dev)
        pick = r[(r % 6 == 1) & (r % 7 == k)]
        e = 1800 + 100 * k
        sig_t[pick, :e] = 55.0 + 2.0 * torch.randn((pick.numel(), e), generator=gen, device=dev, dtype=torch.float32)
    torch.cuda.synchronize()

    def step(flag):
        eng.detect_llr_rows(sig_t.data_ptr(), len_t.data_ptr(), R, mb, with_start_peak=True, device_ptrs=True, rows_dev=rows_t.data_ptr(),
                            tails_nan=True, resegment=flag)

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
    counts = eng.debug_resegment()
    eng.set_profiling(True)
    step(True)
    times = {}
    for k, v in eng.kernel_times():
        times[k] = round(times.get(k, 0.0) + v, 3)
    eng.set_profiling(False)
    on, off = rows[True], rows[False]
    keep = (on["reserved_"] & lib.ROW_RESEGMENTED) == 0
    added = float(np.median(ms[True]) - np.median(ms[False]))
    phase = {k: v for k, v in times.items() if "resegment" in k or k.startswith("k_rs_")}
    # (the validation of the subset runs under the first pass's kernel names: the profiled step lists each twice)
    out = dict(workload="llr_default_window, every sixth read stalled", m=int(m), reads=R, minibatch=mb, steps=a.steps,
               ms_off=[round(x, 3) for x in ms[False]], ms_on=[round(x, 3) for x in ms[True]],
               ms_off_median=round(float(np.median(ms[False])), 3), ms_on_median=round(float(np.median(ms[True])), 3),
               added_ms_per_step=round(added, 3), added_us_per_selected_read=round(1e3 * added / max(counts[0], 1), 3),
               counts=dict(zip(("eligible", "p2_found", "replaced"), counts)),
               pass_off=int(off["success"].sum()), pass_on=int(on["success"].sum()),
               rows_sha256_off=hashlib.sha256(off.tobytes()).hexdigest(), unreplaced_rows_equal=bool(on[keep].tobytes() == off[keep].tobytes()),
               kernel_ms_phase=phase, kernel_ms_on_total=round(sum(times.values()), 3))
    eng.close()
    text = json.dumps(out)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
