"""A/B of k_gains' fast body for interior tiles (llr_stream.h): the headline workload of bench.py (96 000 synthetic RNA004 reads
of the 200 k window, resident in HBM, minibatch 1000) in ONE process, the detect call repeated with ADP_GAINS_TILE_FAST flipped
between calls (the library reads it per call).  Per call: the HIP-event times of k_gains<1> and k_gains<2> and the whole call's
wall time; at the end the rows' digest per setting (they must agree) and, per setting, mean / min / max of the two passes' sum.
Usage: python tools/gains_tile_fast_ab.py [--reads N] [--calls K] [--out profiles/gains_tile_fast_ab.txt]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=96000)
    ap.add_argument("--calls", type=int, default=6, help="calls per setting (after two warm-up calls)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gains_tile_fast_ab.txt"))
    a = ap.parse_args()
    import torch

    import bench
    from adapted_amd import lib

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
        os.environ["ADP_GAINS_TILE_FAST"] = setting
        t0 = time.perf_counter()
        eng.detect_llr_rows(sig.data_ptr(), lens.data_ptr(), R, mb, with_start_peak=True, device_ptrs=True, rows_dev=rows.data_ptr(), tails_nan=True)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        per = {}
        for name, ms in eng.kernel_times():
            per[name] = per.get(name, 0.0) + ms
        return per.get("k_gains<1>", float("nan")), per.get("k_gains<2>", float("nan")), wall, hashlib.sha256(rows.cpu().numpy().tobytes()).hexdigest()

    for s in ("1", "0"):
        call(s)
    eng.set_profiling(True)
    lines = ["# ADP_GAINS_TILE_FAST alternating between calls, %d reads x %d samples, minibatch %d; ms per call" % (R, m, mb),
             "# call setting k_gains<1> k_gains<2> sum wall rows_sha256[:12]"]
    rec = {"1": [], "0": []}
    sha = {"1": set(), "0": set()}
    c0 = eng.debug_counters(80)
    for k in range(2 * a.calls):
        s = "1" if k % 2 == 0 else "0"
        g1, g2, wall, dig = call(s)
        rec[s].append((g1, g2, wall))
        sha[s].add(dig)
        lines.append("%2d %s %8.3f %8.3f %8.3f %8.2f %s" % (k, s, g1, g2, g1 + g2, wall, dig[:12]))
    c1 = eng.debug_counters(80)
    eng.set_profiling(False)
    for s in ("0", "1"):
        v = np.array(rec[s])
        tot = v[:, 0] + v[:, 1]
        lines.append("# setting %s: k_gains<1> %.3f  k_gains<2> %.3f  sum mean %.3f min %.3f max %.3f (spread %.3f)  wall mean %.2f"
                     % (s, v[:, 0].mean(), v[:, 1].mean(), tot.mean(), tot.min(), tot.max(), tot.max() - tot.min(), v[:, 2].mean()))
    m0 = np.array(rec["0"])[:, :2].sum(axis=1).mean()
    m1 = np.array(rec["1"])[:, :2].sum(axis=1).mean()
    lines.append("# drop of the two passes' sum: %.3f ms (%.1f %%); tiles committed by the fast body %d, run again %d; rows equal: %s"
                 % (m0 - m1, 100.0 * (m0 - m1) / m0, int(c1[76] - c0[76]), int(c1[77] - c0[77]), sha["0"] == sha["1"] and len(sha["0"]) == 1))
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
