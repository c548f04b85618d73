#!/usr/bin/env python3
"""Golden results of the re-segmentation (ADP_LLR_RESEGMENT, include/adapted_hip_resegment.h), produced by the REAL reference
(oracle/ref_harness.py; the real bottleneck 1.3.2) in the build container -- run with the reference's interpreter (numpy 1.26):
python3.9 tools/gen_resegment_golden.py [--check]
The batches of tests/resegment_cases.py go to combined_detect_llr2 one minibatch at a time, for every (batch, minibatch size) of
resegment_cases.RUNS.  Then the rule, with the reference's own functions: for every eligible read c, the trace of
calc_adapter_trace(s_, 1, 1, trace_start = c, c = trace.c, c2 = trace.c2) on the minibatch's normalised, pooled signal,
detect_full_polya_trace_peak_with_spike, p2, and validate_boundaries from adapter_start = the first adapter end.
tests/golden/resegment_<batch>_mb<size>.npz holds per read the first row, eligibility, c, p2, the second validation's DetectResults
field by field and a sha256 of the signal's bytes; no signals.  The run ASSERTS that the batches reach everything
resegment_cases.REQUIRED names.  With --check nothing is written: the run's outputs are compared with the stored fixtures.
TEST INFRASTRUCTURE."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402

ref_harness.install()
import bottleneck  # noqa: E402
from adapted.config.sig_proc import get_chemistry_specific_config  # noqa: E402
from adapted.container_types import Boundaries, DetectResults  # noqa: E402
from adapted.detect.combined import combined_detect_llr2, validate_boundaries  # noqa: E402
from adapted.detect.downscale import downscale_signal  # noqa: E402
from adapted.detect.llr import calc_adapter_trace, detect_full_polya_trace_peak_with_spike  # noqa: E402
from adapted.detect.normalize import normalize_signal  # noqa: E402

import resegment_cases as R  # noqa: E402

assert "slow" not in bottleneck.move_mean.__module__, "the real bottleneck is required"
warnings.simplefilter("ignore")


def plain(res):
    d = dict(vars(res))
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            d[k] = v.tolist()
    return d


def ref_spc():
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.rna_start_peak.detect_rna_start_peak = False
    spc.update_primary_method()
    spc.update_sig_preload_size()
    assert spc.primary_method == "llr" and spc.sig_preload_size == R.M
    return spc


def trace(s_, start, sums=None):
    head = 5 if sums is None else 1
    return calc_adapter_trace(signal=s_, offset_head=head, offset_tail=head, stride=1, early_stop1_window=0, early_stop1_stride=0,
                              early_stop2_window=0, early_stop2_stride=0, return_c_c2=sums is None, trace_start=start,
                              adapter_early_stopping=0, polya_early_stopping=0, c=None if sums is None else sums[0],
                              c2=None if sums is None else sums[1])


def run(name, mb, spc):
    sig, lens = R.batch(name)
    n = sig.shape[0]
    co = spc.core
    first, second = [None] * n, [None] * n
    elig, cs, p2s = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for a in range(0, n, mb):
        s, l = np.array(sig[a:a + mb]), np.array(lens[a:a + mb])
        try:
            rows = combined_detect_llr2(s, l, spc)
        except Exception as e:  # the reference drops the minibatch
            print("%s mb %d: minibatch at read %d dropped: %s" % (name, mb, a, e))
            continue
        down = downscale_signal(normalize_signal(s[:, :co.max_obs_trace], outlier_thresh=co.sig_norm_outlier_thresh, with_nan=True)[:, co.min_obs_adapter:],
                                co.downscale_factor)
        n_nan = np.isnan(down).sum(axis=1)
        for i, res in enumerate(rows):
            r = a + i
            first[r] = plain(res)
            if not R.eligible(first[r]):
                continue
            a1, p1 = int(res.llr_adapter_end), int(res.llr_polya_end)
            elig[r] = True
            assert (p1 - co.min_obs_adapter) % co.downscale_factor == 0
            c = (p1 - co.min_obs_adapter) // co.downscale_factor
            s_ = down[i][:down.shape[1] - n_nan[i]]
            t0 = trace(s_, 0)
            p = int(detect_full_polya_trace_peak_with_spike(trace(s_, c, (t0.c, t0.c2)).signal))
            cs[r] = c
            p2s[r] = p * co.downscale_factor + co.min_obs_adapter if p > 0 else 0
            if p2s[r] == 0:
                continue
            bd = Boundaries(adapter_start=a1, adapter_end=p1, polya_end=int(p2s[r]), polya_end_topk=np.array([int(p2s[r])]))
            second[r] = plain(validate_boundaries(s[i][:l[i]], bd, spc, int(l[i])))
    return R.pack(first, elig, cs, p2s, second, sig, plain(DetectResults(success=False)))


spc = ref_spc()
files = {}
for name, mb in R.RUNS:
    out = run(name, mb, spc)
    fn = os.path.basename(R.golden_path(name, mb))
    files[fn] = out
    g = dict(eligible=out["eligible"], c=out["c"], p2=out["p2"])
    for key in ("first", "second"):
        g[key] = [r if ok else None for r, ok in zip(R.rc.decode(out, key + "."), out[key + ".given"])]
    exp, counts, kinds = R.expected(g)
    cov = R.coverage(name, g)
    print("%s, minibatch %d: eligible / p2 > 0 / kept = %s; %s" % (name, mb, counts, {k: kinds.count(k) for k in sorted(set(kinds))}))
    for r, kind in enumerate(kinds):
        if kind not in ("ineligible", "dropped") or (g["first"][r] is not None and not g["first"][r]["success"]):
            f = g["first"][r] or {}
            s2 = g["second"][r]
            print("  read %2d %-13s first %-42s (%s, %s)  c %d p2 %d%s" % (r, kind, f.get("fail_reason"), f.get("llr_adapter_end"), f.get("llr_polya_end"),
                  out["c"][r], out["p2"][r], "" if s2 is None else "  second: %s %s" % (s2["success"], s2["fail_reason"])))
    missing = [k for k in R.REQUIRED[name] if k not in cov]
    assert not missing, "%s, minibatch %d: the batch does not reach %s" % (name, mb, missing)
    if (name, mb) == ("main", 48):
        assert counts[0] == 24 and counts[2] == 21, counts

if "--check" in sys.argv:
    for fn, out in files.items():
        have = np.load(os.path.join(R.GOLD, fn))
        assert sorted(have.files) == sorted(out), "%s holds other keys" % fn
        bad = [k for k in out if have[k].shape != np.asarray(out[k]).shape
               or not (np.array_equal(have[k], out[k], equal_nan=True) if have[k].dtype.kind == "f" else have[k].tolist() == np.asarray(out[k]).tolist())]
        assert not bad, "%s differs from the fixture: %s" % (fn, bad[:5])
    print("python %s numpy %s: equal to the fixtures" % (sys.version.split()[0], np.__version__))
    sys.exit(0)
for fn, out in files.items():
    np.savez_compressed(os.path.join(R.GOLD, fn), **out)
    print("wrote tests/golden/%s (%d bytes)" % (fn, os.path.getsize(os.path.join(R.GOLD, fn))))
import adapted  # noqa: E402

with open(os.path.join(R.GOLD, "PROVENANCE_resegment.txt"), "w") as f:
    f.write("generated by tools/gen_resegment_golden.py (cases: tests/resegment_cases.py)\n")
    f.write("python %s\nnumpy %s\nbottleneck %s\n" % (sys.version.split()[0], np.__version__, bottleneck.__version__))
    f.write("reference ADAPTed %s: combined_detect_llr2 per minibatch, then calc_adapter_trace / detect_full_polya_trace_peak_with_spike "
            "from the first poly(A) end and validate_boundaries from the first adapter end\n" % getattr(adapted, "__version__", "?"))
    f.write("RNA004 preset, LLR primary; runs (batch, minibatch): %s\n" % ", ".join("%s/%d" % r for r in R.RUNS))
