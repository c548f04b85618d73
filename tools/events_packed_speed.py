#!/usr/bin/env python3
"""The packed forms of the event calls beside the matrix form (adp_event_levels_packed / adp_event_levels: adapted_amd/csrc/events_api.h,
fingerprint_api.h), host to host, on the same 4 096 synthetic adapters of 3 000 .. 6 000 samples -- what `adapted events` moves per
batch against what a detect call holds resident: event_levels on the padded float32 matrix [4096, 6000], event_levels_packed on the
float32 slices back to back, event_levels_packed on the raw int16 slices with a calibration per slice (the float32 values ARE the
calibrated raw ones, so the three answers are the same bytes, which is checked).  Medians of R alternated calls in one process (a
round calls the three forms in turn), wall time of the whole call -- staging copy, three kernels, copies back --, and k_ev_scores'
device time in the three forms from adp_kernel_times in R more alternated rounds.  Nothing here gates anything.

  python tools/events_packed_speed.py [--reps R] [--small] [--out FILE]     (default FILE: profiles/events_packed_speed.json)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import events_oracle as eo  # noqa: E402


def adapters(n, lo=3000, hi=6000, seed=3, distinct=64):
    """-> (raw int16 slices, scale, offset float32 [n], sizes): `distinct` staircases (levels N(85, 12^2), dwells of 5 .. 40 samples,
    noise sd 2) of `hi` samples, quantised with a calibration per adapter and cut to sizes uniform in [lo, hi]"""
    rng = np.random.default_rng(seed)
    base = [eo.staircase(rng, hi) for _ in range(min(distinct, n))]
    sizes = rng.integers(lo, hi + 1, size=n)
    scale, offset = rng.uniform(0.14, 0.2, n).astype(np.float32), rng.uniform(-20.0, 20.0, n).astype(np.float32)
    raw = [np.clip(np.rint(base[g % len(base)][:sizes[g]] / scale[g] - offset[g]), -32768, 32767).astype(np.int16) for g in range(n)]
    return raw, scale, offset, sizes


def measure(n, reps, E):
    from adapted_amd.detect._rows import _engine
    from adapted_amd.polya_length import EventParams

    eng = _engine()
    raw, scale, offset, sizes = adapters(n)
    pa = [(scale[g] * (raw[g].astype(np.float32) + offset[g])).astype(np.float32) for g in range(n)]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    L = int(sizes.max())
    matrix = np.full((n, L), np.nan, dtype=np.float32)
    for g in range(n):
        matrix[g, :sizes[g]] = pa[g]
    packed_f32, packed_i16 = np.concatenate(pa), np.concatenate(raw)
    lens, idx, starts = sizes.astype(np.int32), np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    a = EventParams().args()
    forms = {"matrix_f32": lambda: eng.event_levels(matrix, lens, idx, starts, sizes.astype(np.int64), a, E),
             "packed_f32": lambda: eng.event_levels_packed(packed_f32, offsets, a, E),
             "packed_i16": lambda: eng.event_levels_packed(packed_i16, offsets, a, E, scale=scale, offset=offset)}
    first = {k: f() for k, f in forms.items()}  # warm-up; the three answers are the same bytes
    equal = all(first[k][key].tobytes() == first["matrix_f32"][key].tobytes() for k in forms for key in first[k])
    wall = {k: [] for k in forms}
    eng.set_profiling(False)
    for _ in range(reps):
        for k, f in forms.items():
            t = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t) * 1e3)
    kernels = {k: {} for k in forms}
    eng.set_profiling(True)
    try:
        for _ in range(reps):
            for k, f in forms.items():
                f()
                kt = {}
                for name, ms in eng.kernel_times():
                    kt[name] = kt.get(name, 0.0) + ms
                for name, ms in kt.items():
                    kernels[k].setdefault(name, []).append(ms)
    finally:
        eng.set_profiling(False)

    def stats(v):
        return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))

    out = dict(segments=n, samples_min=int(sizes.min()), samples_max=L, samples_total=int(sizes.sum()), max_events=E, reps=reps,
               outputs_equal=bool(equal), host_bytes={"matrix_f32": int(matrix.nbytes), "packed_f32": int(packed_f32.nbytes),
                                                      "packed_i16": int(packed_i16.nbytes + scale.nbytes + offset.nbytes)},
               wall_ms={k: stats(v) for k, v in wall.items()},
               kernel_ms={k: {name: stats(v) for name, v in kt.items()} for k, kt in kernels.items()})
    out["segments_per_s"] = {k: n / (out["wall_ms"][k]["median"] * 1e-3) for k in forms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a sixteenth of the adapters (a quick look)")
    ap.add_argument("--max_events", type=int, default=110)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_packed_speed.json"))
    a = ap.parse_args()
    res = measure(4096 // (16 if a.small else 1), a.reps, a.max_events)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
