#!/usr/bin/env python3
"""Time the CNN primary on resident raw int16 reads both ways (GPU box): the float32 route -- adp_calibrate_i16 into a float32
matrix, then adp_detect_cnn on it (detect_rows_device), the calibration pass INCLUDED in the time -- against the native route,
adp_detect_cnn_i16 (detect_rows_device_i16), which reads the int16 rows in every pass.  Synthetic reads are made on the device and
quantised there once (scale ~ U(0.14, 0.2), offset ~ U(-20, 20) per read).  Four modes ALTERNATE in one process per workload --
f32_a, i16_a, f32_b, i16_b: each route twice, so that the difference between a route's two medians is the spread a difference
between the routes has to exceed -- after a warm-up, the host clock around calls that end with the stream synchronised; then one
profiled step per route for the per-kernel HIP-event times.  The driver starts one worker process per workload under a time limit
of its own and stops at the first that fails.
usage: python tools/cnn_i16_speed.py [--steps 20] [--warmup 2] [--minibatch 1000] [--seed 2024] [--limit 500] [--only 200k,default]
prints one JSON line per workload (24 000 reads at the 200 k window / 96 000 at the default window)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"200k": (200000, 24000), "default": (None, 96000)}  # window (None: the preset's), reads
MODES = ("f32_a", "i16_a", "f32_b", "i16_b")


def worker(name, a):
    import numpy as np
    import torch

    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.detect import cnn

    torch.cuda.init()
    window, R = WORKLOADS[name]
    R = a.reads or R
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = False, True
    if window:
        spc.core.max_obs_trace = window
    spc.update_primary_method()
    spc.update_sig_preload_size()
    m, mb = spc.sig_preload_size, a.minibatch
    assert m % 4 == 0
    dev = torch.device("cuda", 0)
    eng = lib.Engine(spc, R, m, device=0)
    lens = np.full(R, m, dtype=np.int32)
    sig_t = torch.empty((R, m), dtype=torch.float32, device=dev)  # the synthetic pA first, then the float32 route's matrix
    raw_t = torch.empty((R * m + 64,), dtype=torch.int16, device=dev)
    len_t = torch.from_numpy(lens).to(dev)
    g = torch.Generator(device="cpu").manual_seed(a.seed)
    scale = (0.14 + 0.06 * torch.rand(R, generator=g)).to(torch.float32)
    offset = (-20.0 + 40.0 * torch.rand(R, generator=g)).to(torch.float32)
    cal_t = torch.cat([scale, offset]).to(dev)
    torch.cuda.synchronize()
    eng.synth_fill(sig_t.data_ptr(), len_t.data_ptr(), R, seed=a.seed, first_read=0, decorate=True)
    raw2 = raw_t[:R * m].view(R, m)
    for r0 in range(0, R, 1000):  # (in pieces: the temporaries stay small)
        r1 = min(R, r0 + 1000)
        q = torch.nan_to_num(sig_t[r0:r1], nan=108.0) / cal_t[r0:r1, None] - cal_t[R + r0:R + r1, None]
        raw2[r0:r1] = torch.clamp(torch.round(q), -32768, 32767).to(torch.int16)
    del q
    torch.cuda.synchronize()
    d_raw, d_len, d_sc, d_of, d_f32 = raw_t.data_ptr(), len_t.data_ptr(), cal_t.data_ptr(), cal_t.data_ptr() + R * 4, sig_t.data_ptr()

    def step(mode):
        if mode.startswith("f32"):
            eng.calibrate_i16(d_raw, d_len, d_sc, d_of, R, d_f32)
            return cnn.detect_rows_device(eng, d_f32, d_len, R, lens, None, spc, minibatch=mb)
        return cnn.detect_rows_device_i16(eng, d_raw, d_len, d_sc, d_of, R, lens, None, spc, minibatch=mb)

    for _ in range(a.warmup):
        for mode in MODES:
            step(mode)
    ms = {k: [] for k in MODES}
    rows = {}
    for _ in range(a.steps):
        for mode in MODES:  # alternated: all see the same state of the device
            t0 = time.perf_counter()
            rows[mode] = step(mode)
            ms[mode].append((time.perf_counter() - t0) * 1e3)
    digest, kernel_ms = {}, {}
    for mode in ("f32_a", "i16_a"):
        r = rows[mode].copy()
        r["open_pores_more"] = 0
        digest[mode[:3]] = hashlib.sha256(r.tobytes()).hexdigest()
        eng.set_profiling(True)
        step(mode)
        t = {}
        for k, v in eng.kernel_times():
            t[k] = round(t.get(k, 0.0) + v, 3)
        t["all_kernels"] = round(sum(v for _, v in eng.kernel_times()), 3)
        kernel_ms[mode[:3]] = t
        eng.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    f32, i16 = float(np.median(ms["f32_a"] + ms["f32_b"])), float(np.median(ms["i16_a"] + ms["i16_b"]))
    spread = max(abs(med["f32_a"] - med["f32_b"]), abs(med["i16_a"] - med["i16_b"]))
    out = dict(workload=name, m=int(m), reads=R, minibatch=mb, steps=a.steps, ms_median={k: round(v, 3) for k, v in med.items()},
               ms_min={k: round(min(v), 3) for k, v in ms.items()}, f32_ms=round(f32, 3), i16_ms=round(i16, 3), spread_ms=round(spread, 3),
               native_slower_beyond_spread=bool(i16 - f32 > spread), rows_equal=bool(digest["f32"] == digest["i16"]),
               passing=int(rows["i16_a"]["success"].sum()), resident_bytes_per_sample={"f32_route": 6, "native": 2},
               resident_gb={"f32_route": round(R * m * 6 / 1e9, 2), "native": round(R * m * 2 / 1e9, 2)}, kernel_ms=kernel_ms)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=0, help="reads per step (default: the workload's)")
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--limit", type=int, default=500, help="seconds a workload's process may take")
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
