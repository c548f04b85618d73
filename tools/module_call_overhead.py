#!/usr/bin/env python3
"""Host time of one small call of the module entry points (adapted_amd/csrc/modules.hip): 3 reads of 256 samples, so that the call's
fixed cost -- checks, workspace pieces, copies in, launches, copies out, one synchronise -- is all there is.  Median and 10th / 90th
percentile of the host clock around the C call, in microseconds, after a warm-up.  For an A/B of two library builds set
ADAPTED_HIP_LIB and alternate the runs in one session on one device.

  python tools/module_call_overhead.py [--calls N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.config.schema import StreamingConfig
    from adapted_amd.detect import mvs

    spc = get_chemistry_specific_config("RNA004")
    eng = lib.Engine(spc, 4, spc.sig_preload_size)
    n, L, ns = 3, 256, 4
    rng = np.random.default_rng(1)
    sig = (np.where((np.arange(L) // 16) % 2 == 0, 80.0, 110.0)[None, :] + rng.normal(0.0, 2.0, (n, L))).astype(np.float32)
    sig64 = sig.astype(np.float64)
    lens = np.array([L, 131, L], dtype=np.int32)
    segs = np.zeros(ns, dtype=lib.SEG_DTYPE)
    segs["row"], segs["start"], segs["end"] = [1, 2, 1, 2], [8, 100, 50, 0], [120, 400, 50, 256]
    h, X = eng._h, eng.lib
    m_args, e_args = mvs._args(None, StreamingConfig()), lib.AdpEventArgs(4.0, 1e-3, 8, 8)
    sp_args, as_args = lib.AdpStartPeakArgs(200.0, 2, 100, 5, 5), lib.AdpAdapterStartArgs(5.0, 90.0, 10, 50)
    i8, i8b, f8, f8b, i4 = (np.zeros(4096, dtype=np.int64), np.zeros(4096, dtype=np.int64), np.zeros(4096), np.zeros(4096),
                            np.zeros(4096, dtype=np.int32))
    q, qc = rng.normal(0.0, 1.0, (3, 4)), np.full(3, 4, dtype=np.int32)
    t, tc = rng.normal(0.0, 1.0, (2, 4)), np.full(2, 4, dtype=np.int32)
    calls = {
        "adp_mvs_detect": lambda: X.adp_mvs_detect(h, sig, lens, n, L, C.byref(m_args), 0, i8),
        "adp_seg_stats": lambda: X.adp_seg_stats(h, sig, lens, n, L, segs, ns, 0, f8, i8),
        "adp_med_mad": lambda: X.adp_med_mad(h, sig, lens, n, L, 0, f8),
        "adp_pool_mean": lambda: X.adp_pool_mean(h, sig, n, L, 3, 0, f8),
        "adp_start_peak": lambda: X.adp_start_peak(h, sig, lens, n, L, C.byref(sp_args), 0, i4, f8),
        "adp_adapter_start": lambda: X.adp_adapter_start(h, sig, lens, n, L, C.byref(as_args), 0, i4, i8, i8b, f8),
        "adp_c_llr_detect": lambda: X.adp_c_llr_detect(h, sig64, lens, n, L, 20, 5, 10, lib.ADP_CLLR_POLYA, i8, i8b, f8),
        "adp_segment_events": lambda: X.adp_segment_events(h, sig, lens, n, L, segs, ns, C.byref(e_args), 0, 3, i8, i8b, f8),
        "adp_dtw_assign": lambda: X.adp_dtw_assign(h, q, qc, 3, 4, t, tc, 2, 4, 1, 0, f8, i4, f8b),
    }
    res = {"calls": args.calls, "library": os.environ.get("ADAPTED_HIP_LIB", "in-tree"), "us": {}}
    for name, fn in calls.items():
        for _ in range(300):
            assert fn() == 0, (name, X.adp_last_error())
        ts = np.empty(args.calls)
        for i in range(args.calls):
            t0 = time.perf_counter_ns()
            fn()
            ts[i] = (time.perf_counter_ns() - t0) * 1e-3
        res["us"][name] = {"median": round(float(np.median(ts)), 2), "p10": round(float(np.percentile(ts, 10)), 2),
                           "p90": round(float(np.percentile(ts, 90)), 2)}
    eng.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
