#!/usr/bin/env python3
"""Time of the adapter-front post-pass (adp_adapter_front / adp_adapter_front_i16: adapted_amd/csrc/adapter_front.h) beside the
detect step of the same engine, for 24 000 default-window reads (RNA004, LLR primary, m = sig_preload_size) resident in HBM, as
float32 pA and as raw int16.  The reads: the 64 synthetic reads of seed 11 with their first 400 samples raised by 70 pA (a lead
the detector finds on most passing reads), repeated; minibatches of 1000.  Host clock around calls that end in a device
synchronise, and per-kernel times from adp_kernel_times (HIP events on the handle's stream) in a call of their own.

  python tools/adapter_front_speed.py [--reads N] [--reps R] [--revalidate] [--out profiles/adapter_front_speed.json]

--revalidate: also the re-validating forms (adp_adapter_front_revalidate / _i16: adapted_amd/csrc/adapter_front_revalidate.h) on
host rows, beside the plain pass and the detect step (profiles/adapter_front_revalidate_speed.json).

There is no gate: the figures say what the pass costs next to the detect call and next to that call's k_validate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(eng, fn, reps):
    """-> (wall ms per call with profiling off, {kernel: ms} of one profiled call, the last result)"""
    fn()  # warm-up
    eng.set_profiling(False)
    t = time.perf_counter()
    for _ in range(reps):
        res = fn()
    wall = (time.perf_counter() - t) / reps
    eng.set_profiling(True)
    fn()
    kt = {}
    for k, ms in eng.kernel_times():
        kt[k] = kt.get(k, 0.0) + ms
    eng.set_profiling(False)
    return wall * 1e3, kt, res


def measure(n, reps, revalidate=False):
    from adapted_amd import lib, synth
    from adapted_amd.adapter_front import AdapterFrontParams
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.update_primary_method()
    spc.update_sig_preload_size()
    m, mb = spc.sig_preload_size, 1000
    base, blens = synth.synth_batch(11, 0, 64, m)
    base = base.copy()
    base[:, :400] += np.float32(70.0)
    idx = np.arange(n) % 64
    lens = np.ascontiguousarray(blens[idx], dtype=np.int32)
    rng = np.random.default_rng(8)
    scale, offset = rng.uniform(0.14, 0.2, 64).astype(np.float32), rng.uniform(-20.0, 20.0, 64).astype(np.float32)
    raw = np.clip(np.rint(np.nan_to_num(base, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
    args = AdapterFrontParams(min_adapter_len=int(spc.core.min_obs_adapter)).args()
    eng = lib.Engine(spc, n, m, device=0)
    out = dict(reads=n, samples=m, minibatch=mb, reps=reps, window=args.window, min_obs_adapter=args.min_obs_adapter, resident=True)
    d_sig, d_raw, d_len, d_cal = eng.dev_alloc(n * m * 4), eng.dev_alloc(n * m * 2 + 64), eng.dev_alloc(n * 4), eng.dev_alloc(2 * n * 4)
    d_rows = eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
    try:
        eng.h2d(d_sig, base[idx])
        eng.h2d(d_raw, raw[idx])
        eng.h2d(d_len, lens)
        eng.h2d(d_cal, np.concatenate([scale[idx], offset[idx]]))
        for name, detect, front, reval in (
                ("float32", lambda: eng.detect_llr_rows(d_sig, d_len, n, mb, device_ptrs=True, tails_nan=True)[0],
                 lambda rows: eng.adapter_front(d_sig, None, rows, args, n=n, m=m),
                 lambda rows: eng.adapter_front_revalidate(d_sig, d_len, rows, args, n=n, m=m)),
                ("int16", lambda: eng.detect_llr_rows_i16(d_raw, d_len, d_cal, d_cal + n * 4, n, mb)[0],
                 lambda rows: eng.adapter_front_i16(d_raw, d_len, d_cal, d_cal + n * 4, rows, args, n=n, m=m),
                 lambda rows: eng.adapter_front_revalidate_i16(d_raw, d_len, d_cal, d_cal + n * 4, rows, args, n=n, m=m))):
            d_wall, d_kt, rows = _timed(eng, detect, reps)
            # (every timed call starts from the detect call's rows: a patched row would be looked at from its new start)
            f_wall, f_kt, side = _timed(eng, lambda: front(rows.copy()), reps)
            eng.h2d(d_rows, rows)
            r_wall, _, _ = _timed(eng, lambda: (eng.h2d(d_rows, rows), front(d_rows))[1], reps)
            front_ms, validate_ms = sum(f_kt.values()), d_kt.get("k_validate", float("nan"))
            out[name] = dict(detect_wall_ms=d_wall, detect_kernel_ms=sum(d_kt.values()), k_validate_ms=validate_ms,
                             front_wall_ms_host_rows=f_wall, front_wall_ms_device_rows_incl_row_upload=r_wall, front_kernel_ms=f_kt,
                             front_kernels_over_detect_kernels=front_ms / sum(d_kt.values()), front_wall_over_detect_wall=f_wall / d_wall,
                             front_kernels_over_k_validate=front_ms / validate_ms, passing=int((rows["success"] == 1).sum()),
                             patched=int(side[0][:, 3].sum()), value_error=int((side[0][:, 0] == 2).sum()))
            if revalidate:
                v_wall, v_kt, v_side = _timed(eng, lambda: reval(rows.copy()), reps)
                v_ms = sum(v_kt.values())
                out[name].update(revalidate_wall_ms_host_rows=v_wall, revalidate_kernel_ms=v_kt, revalidate_kernels_over_detect_kernels=v_ms / sum(d_kt.values()),
                                 revalidate_wall_over_detect_wall=v_wall / d_wall, revalidate_wall_over_front_wall=v_wall / f_wall,
                                 revalidate_kernels_over_k_validate=v_ms / validate_ms, kept=int((v_side[4][:, 0] == 1).sum()),
                                 rejected=int((v_side[4][:, 0] == 0).sum()))
    finally:
        for p in (d_sig, d_raw, d_len, d_cal, d_rows):
            eng.dev_free(p)
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--revalidate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reads, a.reps, a.revalidate)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
