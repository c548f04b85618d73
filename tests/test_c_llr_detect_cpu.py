"""The best-split segmenters of the reference's `_c_llr` (adapted/detect/_c_llr.pyx:40-64, :239-433): the CPU restatement
(tests/c_llr_detect_restated.py, on the oracle's gains) against the vectors the REAL reference produced
(tests/golden/c_llr_detect.npz, tools/gen_c_llr_detect_golden.py), the paths the cases cover, and the drop-in's names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import c_llr_detect_restated as R
from c_llr_detect_cases import CASES, SPLITS, by_name, signal_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "c_llr_detect.npz")
NAMES = ["_best_split", "_gains", "_gains_w_early_stop", "_gains_w_polya_early_stop", "c_llr_trace_gains", "c_llr_trace",
         "c_llr_detect_adapter", "c_llr_detect_adapter_polya", "c_llr_detect_adapter_trace", "c_llr_detect_adapter_polya_trace",
         "c_llr_boundary_traces", "c_llr_detect_adapter_batch", "c_llr_detect_adapter_polya_batch", "best_split_batch"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_reference(oracle_mod, gold, case):
    x = signal_of(case)
    nm = case["name"]
    a = R.detect(oracle_mod, x, case["mo"], case["bt"])["result"]
    p = R.detect(oracle_mod, x, case["mo"], case["bt"], case["mpo"])["result"]
    assert a == tuple(gold[nm + ".adapter"].tolist())
    assert p == tuple(gold[nm + ".polya"].tolist())
    if case["trace"]:
        for key, got in (("trace", R.traces(oracle_mod, x, case["mo"], case["bt"])),
                         ("ptrace", R.traces(oracle_mod, x, case["mo"], case["bt"], case["mpo"])),
                         ("btrace", R.traces(oracle_mod, x, case["mo"], case["bt"]))):
            for k, g in enumerate(got):
                assert np.array_equal(g, gold["%s.trace%d" % (nm, k)], equal_nan=True), key


@pytest.mark.parametrize("k", range(len(SPLITS)))
def test_restated_best_split_equals_the_reference(oracle_mod, gold, k):
    nm, s, e, oh, ot = SPLITS[k]
    x = signal_of(by_name(nm))
    c, c2 = np.cumsum(x), np.cumsum(np.multiply(x, x))
    xs, g = R.best_split(oracle_mod, s, e, c, c2, oh, ot)
    want = gold["split%d" % k]
    assert xs == int(want[0])
    assert g == want[1] or (np.isinf(g) and g == want[1])


def test_the_cases_cover_every_path(oracle_mod):
    branches, flags = set(), set()
    for case in CASES:
        x = signal_of(case)
        d = R.detect(oracle_mod, x, case["mo"], case["bt"])
        dp = R.detect(oracle_mod, x, case["mo"], case["bt"], case["mpo"])
        branches.add(d["branch"])
        flags |= d["flags"] | dp["flags"]
        # both fallbacks in ONE read
        if {"head_fallback", "tail_fallback"} <= d["flags"]:
            flags.add("both_fallbacks")
    assert branches == {"full_adapter", "partial_adapter", "first_split_is_adapter_start", "none_by_decision", "no_first_split"}
    assert {"head_fallback", "tail_fallback", "both_fallbacks", "polya_not_found"} <= flags
    sizes = {signal_of(c).size for c in CASES}
    assert {1, 2, 3, 199996} <= sizes
    assert any(c["mo"] == 0 and c["bt"] == 0 for c in CASES)


def test_quirk_two_tuple_from_the_polya_variant(gold):
    # x_first = -1: the poly(A) variant returns the 2-tuple (0, 0); a decision for "no adapter" returns (0, 0, 0)
    assert gold["constant.polya"].tolist() == [0, 0]
    assert gold["none_by_decision.polya"].tolist() == [0, 0, 0]


def test_the_module_has_every_name():
    from adapted_amd.detect import _c_llr

    missing = [n for n in NAMES if not callable(getattr(_c_llr, n, None))]
    assert not missing


def test_rejects_what_the_reference_would_read_outside_its_arrays():
    from adapted_amd.detect import _c_llr

    c = np.arange(10.0)
    with pytest.raises(ValueError):
        _c_llr._best_split(0, 11, c, c, 1, 1)
    with pytest.raises(ValueError):
        _c_llr._best_split(5, 4, c, c, 1, 1)
    with pytest.raises(ValueError):
        _c_llr._best_split(0, 10, c, c, -1, 1)
    with pytest.raises(ValueError):
        _c_llr.c_llr_detect_adapter(np.zeros(0), 5, 5)
    with pytest.raises(ValueError):
        _c_llr.c_llr_detect_adapter_polya(np.ones(10), 5, -1, 5)
    with pytest.raises(ValueError):
        _c_llr.c_llr_detect_adapter_trace(np.zeros(0), 5, 5)
    with pytest.raises(ValueError):
        _c_llr.c_llr_detect_adapter_batch(np.ones((2, 10)), [10, 0], 5, 5)


def _reference_available():
    from oracle import ref_harness

    return ref_harness.available()


@pytest.mark.reference
@pytest.mark.skipif(not _reference_available(), reason="the reference is not present")
def test_the_real_module_on_the_cases(gold):
    """the reference's own module, called directly (in a child process: the harness installs import shims)"""
    code = """
import json, sys
sys.path[:0] = [%r, %r]
from oracle import ref_harness
ref_harness.install()
import adapted.detect.llr
from adapted.detect import _c_llr as ref
from c_llr_detect_cases import CASES, signal_of
out = {}
for c in CASES:
    x = signal_of(c)
    out[c["name"]] = [list(ref.c_llr_detect_adapter(x, c["mo"], c["bt"])), list(ref.c_llr_detect_adapter_polya(x, c["mo"], c["bt"], c["mpo"]))]
print(json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for case in CASES:
        a, p = got[case["name"]]
        assert a == gold[case["name"] + ".adapter"].tolist()
        assert p == gold[case["name"] + ".polya"].tolist()
