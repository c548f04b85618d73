"""A/B of pass 2's window (llr_stream.h, peaks.h; ADP_G2_WINDOW): the headline workload of bench.py (96 000 synthetic RNA004 reads
of the 200 k window, resident in HBM, minibatch 1000) in ONE process, the detect call repeated with ADP_G2_WINDOW cycling through
the given settings from call to call (the library reads it per call; 0: the whole trace, the stand-in for the code before the
window).  Per call: the HIP-event times of k_gains<2>, k_polya_peak and their redo scopes, the call's wall time, the reads decided
inside the window and the reads sent to the redo list (debug counters 78 / 79), and the rows' digest (all settings must agree).
At the end, per setting, mean / min / max of the wall time, and the drop against setting 0 beside the larger of the two spreads.
Usage: python tools/g2_window_ab.py [--reads N] [--calls K] [--settings 0,1024] [--out profiles/g2_window_ab.txt]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCOPES = ("k_gains<2>", "k_polya_peak", "k_gains<2> redo", "k_polya_peak redo")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=96000)
    ap.add_argument("--calls", type=int, default=6, help="calls per setting (after one warm-up call each)")
    ap.add_argument("--settings", default="0,1024", help="values of ADP_G2_WINDOW, cycled from call to call ('default': unset)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g2_window_ab.txt"))
    a = ap.parse_args()
    import torch

    import bench
    from adapted_amd import lib

    settings = a.settings.split(",")
    spc = bench.make_spc(200000)
    m, R, mb = spc.sig_preload_size, a.reads, 1000
    dev = torch.device("cuda", 0)
    eng = lib.Engine(spc, R, m, device=0)
    sig = torch.empty((R, m), dtype=torch.float32, device=dev)
    lens = torch.from_numpy(np.full(R, m, dtype=np.int32)).to(dev)
    rows = torch.empty((R, lib.ROW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.synth_fill(sig.data_ptr(), lens.data_ptr(), R, seed=2024, first_read=0, decorate=True)

    def call(setting):
        os.environ.pop("ADP_G2_WINDOW", None)
        if setting != "default":
            os.environ["ADP_G2_WINDOW"] = setting
        c0 = eng.debug_counters(80)
        t0 = time.perf_counter()
        eng.detect_llr_rows(sig.data_ptr(), lens.data_ptr(), R, mb, with_start_peak=True, device_ptrs=True, rows_dev=rows.data_ptr(), tails_nan=True)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        c1 = eng.debug_counters(80)
        per = {}
        for name, ms in eng.kernel_times():
            per[name] = per.get(name, 0.0) + ms
        return [per.get(s, 0.0) for s in SCOPES], wall, int(c1[78] - c0[78]), int(c1[79] - c0[79]), hashlib.sha256(rows.cpu().numpy().tobytes()).hexdigest()

    for s in settings:
        call(s)
    eng.set_profiling(True)
    lines = ["# ADP_G2_WINDOW cycling through %s between calls, %d reads x %d samples, minibatch %d; ms per call" % (settings, R, m, mb),
             "# call setting k_gains<2> k_polya_peak k_gains<2>_redo k_polya_peak_redo wall decided_in_window redone rows_sha256[:12]"]
    rec = {s: [] for s in settings}
    sha = set()
    for k in range(len(settings) * a.calls):
        s = settings[k % len(settings)]
        ks, wall, dec, red, dig = call(s)
        rec[s].append(ks + [wall, dec, red])
        sha.add(dig)
        lines.append("%2d %7s %8.3f %8.3f %8.3f %8.3f %8.2f %6d %6d %s" % (k, s, ks[0], ks[1], ks[2], ks[3], wall, dec, red, dig[:12]))
    eng.set_profiling(False)
    stat = {}
    for s in settings:
        v = np.array(rec[s], dtype=np.float64)
        stat[s] = (v[:, 4].mean(), v[:, 4].max() - v[:, 4].min())
        lines.append("# setting %7s: k_gains<2> + redo %.3f  k_polya_peak + redo %.3f  wall mean %.2f min %.2f max %.2f (spread %.2f)  redone per call %.1f"
                     % (s, (v[:, 0] + v[:, 2]).mean(), (v[:, 1] + v[:, 3]).mean(), v[:, 4].mean(), v[:, 4].min(), v[:, 4].max(), stat[s][1], v[:, 6].mean()))
    if "0" in stat:
        for s in settings:
            if s != "0":
                drop, spread = stat["0"][0] - stat[s][0], max(stat["0"][1], stat[s][1])
                lines.append("# setting %7s against 0: wall drops by %.2f ms (%.1f %%), %.1f times the larger spread (%.2f ms)"
                             % (s, drop, 100.0 * drop / stat["0"][0], drop / spread if spread > 0 else float("inf"), spread))
    lines.append("# rows equal over all calls: %s (%s)" % (len(sha) == 1, ", ".join(sorted(d[:12] for d in sha))))
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
