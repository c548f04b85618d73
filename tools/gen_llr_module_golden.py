#!/usr/bin/env python3
"""Golden vectors of the reference's LLR trace module (adapted/detect/llr.py), produced by the REAL reference (its llr.py with
scipy's find_peaks and linregress; its Cython module compiled by pyximport outside the repository, oracle/ref_harness.py) in the
build container -- run with the reference's interpreter (numpy 1.26, scipy 1.7):  python3.9 tools/gen_llr_module_golden.py
tests/golden/llr_module.npz holds, per case of tests/llr_module_cases.py, what the reference returns: the LLRTrace state
(start, end, early_stop, the interpolated trace of the cases marked `store`), find_peaks_in_trace, adapter_end_from_trace with the
four flag combinations (dtypes as returned), the poly(A) traces' state and ends, the two corrections on their own and the spike
test; plus the names and signatures the module defines.  TEST INFRASTRUCTURE."""
import inspect
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402

ref_harness.install()
from adapted.detect import llr as ref  # noqa: E402
from scipy.signal import find_peaks  # noqa: E402

import llr_module_cases as M  # noqa: E402

out = {}
names = sorted(k for k, v in vars(ref).items() if (inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == ref.__name__)
out["names"] = np.array(names)
funcs = [k for k in names if inspect.isfunction(getattr(ref, k))]
out["sig_names"] = np.array(funcs)
out["signatures"] = np.array([str(inspect.signature(getattr(ref, k))) for k in funcs])


def state(t):
    return np.array([t.start, t.end, int(bool(t.early_stop))], dtype=np.int64)


def peaks_of(key, t, fp, ae):
    out[key + ".fp"] = ref.find_peaks_in_trace(t, fp[0], fp[1], fp[2])
    for a in (0, 1):
        for b in (0, 1):
            out["%s.ae%d%d" % (key, a, b)] = ref.adapter_end_from_trace(t, ae[0], ae[1], ae[2], bool(a), bool(b))


for case in M.SIGNAL_CASES:
    nm = "sig." + case["name"]
    raw = M.raw_of(case)
    w = case["win"]
    t = ref.calc_adapter_trace(raw, case["oh"], case["ot"], case["stride"], w[0], w[1], w[2], w[3], True,
                               adapter_early_stopping=case["aes"], polya_early_stopping=case["pes"])
    out[nm + ".bounds"] = state(t)
    if case["store"]:
        out[nm + ".signal"] = t.signal
    peaks_of(nm, t, case["fp"], case["ae"])
    ae = out[nm + ".ae11"]
    a_end = int(ae[0]) if ae.size else raw.size // 4
    pt = ref.calc_polya_trace(t.c, t.c2, a_end, t.end, 50, case["stride"])
    out[nm + ".pbounds"] = state(pt)
    ft = ref.calc_full_polya_trace(raw, a_end)
    out[nm + ".fbounds"] = state(ft)
    out[nm + ".spike"] = np.array([ref.detect_full_polya_trace_peak_with_spike(ft.signal[a_end:])], dtype=np.int64)
    print("%-24s bounds %s  peaks %-30s ae11 %s  spike %d" % (nm, out[nm + ".bounds"].tolist(), out[nm + ".fp"].tolist()[:6],
                                                             ae.tolist()[:6], out[nm + ".spike"][0]))

for case in M.TRACE_CASES:
    nm = "tr." + case["name"]
    y = M.trace_of(case["trace"])
    try:
        t = ref.LLRTrace(signal=y.copy(), stride=case["stride"], min_obs=case["min_obs"], tail_trim=case["tail_trim"])
    except ValueError as e:
        out[nm + ".error"] = np.array(str(e))
        print("%-24s ValueError %s" % (nm, e))
        continue
    out[nm + ".bounds"] = state(t)
    if case["store"]:
        out[nm + ".signal"] = t.signal
    peaks_of(nm, t, case["fp"], case["ae"])
    print("%-24s bounds %s  peaks %-30s ae11 %s (%s)" % (nm, out[nm + ".bounds"].tolist(), out[nm + ".fp"].tolist()[:6],
                                                        out[nm + ".ae11"].tolist()[:6], out[nm + ".ae11"].dtype))

for k, (tn, peak, s, t_, window, prom) in enumerate(M.CORRECTION_CASES):
    y = M.trace_of(M.by_name(M.TRACE_CASES, tn)["trace"])
    a = ref.correct_for_plateau(y, peak, s, t_, window)
    b = ref.correct_for_split_peak(y, peak, s, t_, window, prom)
    out["cor%d" % k] = np.array([a, b], dtype=np.int64)
    print("correction %-10s %5d s=%d t=%.2f w=%d p=%.1f -> %d %d" % (tn, peak, s, t_, window, prom, a, b))

for case in M.SPIKE_CASES:
    nm = "spk." + case["name"]
    y = M.trace_of(case["trace"])
    thr = case["r2"]
    if isinstance(thr, str):
        pk, _ = find_peaks(np.nan_to_num(y, nan=0), distance=case["d"], prominence=case["prom"], width=case["width"], rel_height=0.5)
        r2 = M.r2_of(y, int(pk[0]), int(pk[1]))
        thr = r2 - 1e-9 if thr == "above" else r2 + 1e-9
    out[nm + ".thr"] = np.array(thr)
    r = ref.detect_full_polya_trace_peak_with_spike(y, case["d"], case["prom"], case["width"], case["ratio"], thr)
    out[nm] = np.array(r, dtype=np.int64)
    print("%-24s -> %d (r2 threshold %.12g)" % (nm, r, thr))

np.savez_compressed(os.path.join(ROOT, "tests", "golden", "llr_module.npz"), **out)
import adapted  # noqa: E402
import scipy  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "PROVENANCE_llr_module.txt"), "w") as f:
    f.write("generated by tools/gen_llr_module_golden.py (cases: tests/llr_module_cases.py)\n")
    f.write("python %s\nnumpy %s\nscipy %s\n" % (sys.version.split()[0], np.__version__, scipy.__version__))
    f.write("reference ADAPTed %s, adapted/detect/llr.py (adapted/detect/_c_llr.pyx compiled by pyximport)\n" % getattr(adapted, "__version__", "?"))
print("wrote tests/golden/llr_module.npz")
