#!/usr/bin/env python3
"""Time adp_detect_cnn's second opinion with and without the re-segmentation behind it (ADP_CNN_SECOND_RESEGMENT) on resident
synthetic reads (GPU box): the step bench.py times for --primary cnn at the default window (the rows into a device row buffer),
second_opinion "llr" and "llr_resegment" ALTERNATED in one process, medians of --steps (at least 5), then one profiled step with the
flag on.  The batch is the benchmark's generator with a QUARTER of the reads edited as tests/resegment_cases.py edits ``main``:
r % 8 == 1 gets the low stall of kind 1, 55 + 2 N(0, 1) on [0, 1800 + 100 (r % 7)); r % 8 == 5 the high stall of kind 4, 120 + 3 N(0, 1)
on [0, 2200).  Measured, ungated.
usage: python tools/second_resegment_speed.py [--reads 32000] [--minibatch 1000] [--steps 6] [--warmup 1] [--seed 2024] [--out FILE.json]
prints one JSON line and writes it to --out (profiles/second_resegment_speed.json): the added time per step, the time per selected read,
the counts of both phases"""
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
from adapted_amd.detect import cnn  # noqa: E402


def make_spc():
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = False, True
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=32000)
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "second_resegment_speed.json"))
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: medians of at least 5")
    torch.cuda.init()
    spc = make_spc()
    m, R, mb = spc.sig_preload_size, a.reads, a.minibatch
    dev = torch.device("cuda", 0)
    eng = lib.Engine(spc, R, m, device=0)
    cnn.ensure_weights(eng, None, spc)
    sig_t = torch.empty((R, m), dtype=torch.float32, device=dev)
    len_t = torch.from_numpy(np.full(R, m, dtype=np.int32)).to(dev)
    rows_t = torch.empty((R, lib.ROW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.synth_fill(sig_t.data_ptr(), len_t.data_ptr(), R, seed=a.seed, first_read=0, decorate=True)
    eng.lib.adp_synchronize(eng._h)  # (the generator ran on the engine's stream; the stalls are written on torch's)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    r = torch.arange(R, device=dev)
    for k in range(7):  # reads with r % 8 == 1 and r % 7 == k share a stall length
        pick = r[(r % 8 == 1) & (r % 7 == k)]
        e = 1800 + 100 * k
        sig_t[pick, :e] = 55.0 + 2.0 * torch.randn((pick.numel(), e), generator=gen, device=dev, dtype=torch.float32)
    pick = r[r % 8 == 5]
    sig_t[pick, :2200] = 120.0 + 3.0 * torch.randn((pick.numel(), 2200), generator=gen, device=dev, dtype=torch.float32)
    torch.cuda.synchronize()

    def step(choice):
        eng.detect_cnn_rows(sig_t.data_ptr(), len_t.data_ptr(), R, mb, device_ptrs=True, rows_dev=rows_t.data_ptr(), want_bounds=False,
                            fallback=True, second_opinion=choice)

    choices = ("llr", "llr_resegment")
    for _ in range(a.warmup):
        for c in choices:
            step(c)
    ms = {c: [] for c in choices}
    rows, so = {}, {}
    for _ in range(a.steps):
        for c in choices:  # alternated: both see the same placement of the signal buffer's pages
            t0 = time.perf_counter()
            step(c)
            ms[c].append((time.perf_counter() - t0) * 1e3)
            rows[c] = rows_t.cpu().numpy().view(lib.ROW_DTYPE).reshape(-1).copy()
            so[c] = eng.debug_cnn_second_opinion()
    counts = eng.debug_second_resegment()
    eng.set_profiling(True)
    step("llr_resegment")
    times = {}
    for k, v in eng.kernel_times():
        times[k] = round(times.get(k, 0.0) + v, 3)
    eng.set_profiling(False)
    on, off = rows["llr_resegment"], rows["llr"]
    keep = (on["reserved_"] & lib.ROW_RESEGMENTED) == 0
    added = float(np.median(ms["llr_resegment"]) - np.median(ms["llr"]))
    phase = {k: v for k, v in times.items() if "resegment" in k or k.startswith("k_csr_") or k == "k_rs_bounds"}
    # (the validation of the subset runs under the first pass's kernel names: the profiled step lists each more than once)
    out = dict(workload="cnn_default_window, a quarter of the reads stalled (r % 8 == 1 low, r % 8 == 5 high)", edited_share=0.25, m=int(m), reads=R,
               minibatch=mb, steps=a.steps, ms_off=[round(x, 3) for x in ms["llr"]], ms_on=[round(x, 3) for x in ms["llr_resegment"]],
               ms_off_median=round(float(np.median(ms["llr"])), 3), ms_on_median=round(float(np.median(ms["llr_resegment"])), 3),
               added_ms_per_step=round(added, 3), added_us_per_selected_read=round(1e3 * added / max(counts[0], 1), 3),
               second_opinion_counts=dict(zip(("selected", "replaced", "still_failing", "minibatches_without"), so["llr_resegment"])),
               second_opinion_counts_equal=bool(so["llr"] == so["llr_resegment"]),
               counts=dict(zip(("eligible", "p2_found", "replaced"), counts)),
               pass_off=int(off["success"].sum()), pass_on=int(on["success"].sum()),
               rows_sha256_off=hashlib.sha256(off.tobytes()).hexdigest(), unreplaced_rows_equal=bool(on[keep].tobytes() == off[keep].tobytes()),
               kernel_ms_phase=phase, kernel_ms_on_total=round(sum(times.values()), 3))
    eng.close()
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
