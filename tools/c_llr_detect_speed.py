#!/usr/bin/env python3
"""Reads/s of the batched best-split segmenter (adp_c_llr_detect, adapted_amd/csrc/llr_detect_api.h) with the reads resident in
HBM, at 200 k and 16 k samples, float32 input, poly(A) variant; per-kernel times from adp_kernel_times (HIP events on the
handle's stream).  Prints one JSON object per size, and compares the split searches with the float64 issue bound DESIGN.md
sections 4/5 use for k_gains: ~85 float64 operations per split point, at the chip's float64 vector issue rate.  Usage: python tools/c_llr_detect_speed.py [--reads N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adapted_amd import lib  # noqa: E402
from adapted_amd.config import get_chemistry_specific_config  # noqa: E402
from adapted_amd.synth import synth_read  # noqa: E402

F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9  # MI355X: 256 CUs x 4 SIMDs x 16 float64 lanes per clock at 2.4 GHz (an FMA is one op)
OPS_PER_POINT = 85  # two logarithms (log_cr.h), the two variances and the gain (k_gains)


def run(eng, L, n, reps, mo=300, bt=20, mpo=50):
    base = np.stack([synth_read(7, k, L, L) for k in range(min(n, 64))])
    x = np.empty((n, L), dtype=np.float32)
    for r in range(n):
        x[r] = np.roll(base[r % base.shape[0]], (r // base.shape[0]) * 4099)
    lens = np.full(n, L, dtype=np.int32)
    dev = eng.dev_alloc(x.nbytes)
    try:
        eng.h2d(dev, x)
        rows = eng.c_llr_detect(dev, lens, mo, bt, mpo, polya=True, n=n, L=L, float32=True)  # warm-up
        eng.set_profiling(False)
        t = time.perf_counter()
        for _ in range(reps):
            eng.c_llr_detect(dev, lens, mo, bt, mpo, polya=True, n=n, L=L, float32=True)
        wall = (time.perf_counter() - t) / reps
        eng.set_profiling(True)
        eng.c_llr_detect(dev, lens, mo, bt, mpo, polya=True, n=n, L=L, float32=True)
        kt = {}
        for name, ms in eng.kernel_times():
            kt[name] = kt.get(name, 0.0) + ms
        eng.set_profiling(False)
    finally:
        eng.dev_free(dev)
    # split points searched: level 1 ~L, level 2 ~L (head + tail), poly(A) ~(L - adapter_end)
    pts = 2.0 * L + float(np.mean(L - rows[:, 1]))
    bound_ms = n * pts * OPS_PER_POINT / F64_OPS_PER_S * 1e3
    split_ms = kt.get("k_split_part", 0.0)
    return dict(samples=L, reads=n, reps=reps, wall_ms=wall * 1e3, reads_per_s=n / wall, kernel_ms=kt,
                split_points_per_read=pts, f64_issue_bound_ms=bound_ms,
                split_share_of_bound=(bound_ms / split_ms if split_ms else None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spc = get_chemistry_specific_config("RNA004")
    eng = lib.Engine(spc, 1, spc.sig_preload_size)
    res = [run(eng, 200_000, a.reads, a.reps), run(eng, 16_000, a.reads, a.reps)]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
