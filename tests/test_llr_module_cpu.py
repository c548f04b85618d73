"""The reference's LLR trace module (adapted/detect/llr.py): the CPU restatement (tests/llr_module_restated.py, on the oracle) against
the vectors the REAL reference produced (tests/golden/llr_module.npz, tools/gen_llr_module_golden.py) bit for bit, and the drop-in's
names, signatures and imports."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import llr_module_cases as M
import llr_module_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "llr_module.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _same(got, want):
    got = np.asarray(got)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=True), (got, want)


def _state(st):
    return np.array([st["start"], st["end"], int(st["early_stop"])], dtype=np.int64)


def _peaks(orc, gold, key, sig, start, end, fp, ae):
    _same(R.find_peaks_in_trace(orc, sig, start, end, *fp), gold[key + ".fp"])
    for a in (0, 1):
        for b in (0, 1):
            got = R.adapter_end_from_trace(orc, sig, start, end, ae[0], ae[1], ae[2], bool(a), bool(b))
            _same(got, gold["%s.ae%d%d" % (key, a, b)])


@pytest.mark.parametrize("case", M.SIGNAL_CASES, ids=[c["name"] for c in M.SIGNAL_CASES])
def test_signal_cases(oracle_mod, gold, case):
    nm = "sig." + case["name"]
    raw = M.raw_of(case)
    n, w = raw.size, case["win"]
    g, c, c2 = oracle_mod.c_llr_trace(raw, 0, n - 1, case["oh"], case["ot"], case["stride"], case["aes"], w[0], w[1], case["pes"], w[2], w[3],
                                      return_c_c2=1)
    st = R.trace_state(g, case["stride"], case["oh"], case["ot"])
    _same(_state(st), gold[nm + ".bounds"])
    if case["store"]:
        _same(st["signal"], gold[nm + ".signal"])
    _peaks(oracle_mod, gold, nm, st["signal"], st["start"], st["end"], case["fp"], case["ae"])
    ae = gold[nm + ".ae11"]
    a_end = int(ae[0]) if ae.size else n // 4
    pg = oracle_mod.c_llr_trace(None, a_end, n - 1, 50, n - st["end"], case["stride"], sums=(c, c2))
    _same(_state(R.trace_state(pg, case["stride"], 50 + a_end, n - 1 - st["end"])), gold[nm + ".pbounds"])
    fg = oracle_mod.c_llr_trace(raw, a_end, n - 1, 1, 1, 1, 0, 0, 0, 0, 0, 0)
    _same(_state(R.trace_state(fg, 1, 1, 1)), gold[nm + ".fbounds"])
    assert R.spike(oracle_mod, fg[a_end:]) == int(gold[nm + ".spike"][0])


@pytest.mark.parametrize("case", M.TRACE_CASES, ids=[c["name"] for c in M.TRACE_CASES])
def test_trace_cases(oracle_mod, gold, case):
    nm = "tr." + case["name"]
    y = M.trace_of(case["trace"])
    if nm + ".error" in gold:
        with pytest.raises(ValueError):
            R.trace_state(y, case["stride"], case["min_obs"], case["tail_trim"])
        return
    st = R.trace_state(y, case["stride"], case["min_obs"], case["tail_trim"])
    _same(_state(st), gold[nm + ".bounds"])
    if case["store"]:
        _same(st["signal"], gold[nm + ".signal"])
    _peaks(oracle_mod, gold, nm, st["signal"], st["start"], st["end"], case["fp"], case["ae"])


@pytest.mark.parametrize("k", range(len(M.CORRECTION_CASES)))
def test_corrections(oracle_mod, gold, k):
    tn, peak, s, t, window, prom = M.CORRECTION_CASES[k]
    y = M.trace_of(M.by_name(M.TRACE_CASES, tn)["trace"])
    got = [R.correct_for_plateau(y, peak, s, t, window), R.correct_for_split_peak(oracle_mod, y, peak, s, t, window, prom)]
    assert got == gold["cor%d" % k].tolist()


@pytest.mark.parametrize("case", M.SPIKE_CASES, ids=[c["name"] for c in M.SPIKE_CASES])
def test_spike_cases(oracle_mod, gold, case):
    nm = "spk." + case["name"]
    y = M.trace_of(case["trace"])
    got = R.spike(oracle_mod, y, case["d"], case["prom"], case["width"], case["ratio"], float(gold[nm + ".thr"]))
    assert got == int(gold[nm])


def test_cases_cover_the_branches(gold):
    # both outcomes of the r**2 test, the ratio test, no peak; empty float64 and integer results of adapter_end_from_trace
    spk = {c["name"]: int(gold["spk." + c["name"]]) for c in M.SPIKE_CASES}
    assert spk["linear_rise"] > 0 and spk["linear_rise_below"] == 0 and spk["curved_rise_above"] > 0 and spk["none"] == 0
    dts = {str(gold[k].dtype) for k in gold.files if k.endswith(".ae11") or k.endswith(".ae00")}
    assert {"float64", "int64"} <= dts
    assert any(gold[k].size > 3 for k in gold.files if k.endswith(".ae11"))


def test_names_and_signatures(gold):
    from adapted_amd.detect import llr

    assert sorted(M.NAMES) == sorted(gold["names"].tolist())
    for nm in gold["names"].tolist():
        assert hasattr(llr, nm), nm
    for nm, sig in zip(gold["sig_names"].tolist(), gold["signatures"].tolist()):
        got = inspect.signature(getattr(llr, nm))
        # parameter names, kinds and defaults as the reference's (annotations aside)
        want = [p.strip().split(":")[0].split("=")[0].strip() for p in sig.strip("()").split(",")] if sig != "()" else []
        want = [p.split(" ")[0] for p in sig[1:sig.rindex(")")].split(", ")] if want else []
        assert [p.name for p in got.parameters.values()] == [w.split(":")[0].split("=")[0] for w in want], nm
        defaults = [w.split("=")[1].strip() if "=" in w else None for w in sig[1:sig.rindex(")")].split(", ")] if want else []
        for p, d in zip(got.parameters.values(), defaults):
            if d is None:
                assert p.default is inspect.Parameter.empty, (nm, p.name)
            else:
                assert repr(p.default) == d, (nm, p.name, p.default, d)
    t_params = list(inspect.signature(llr.LLRTrace).parameters)
    assert t_params == ["signal", "c", "c2", "trace_start", "trace_end", "stride", "min_obs", "tail_trim"]


def test_module_imports_neither_scipy_nor_torch_nor_attrs():
    code = ("import sys, json; import adapted_amd.detect.llr; "
            "print(json.dumps(sorted(m for m in ('scipy', 'torch', 'attrs', 'attr') if m in sys.modules)))")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert json.loads(out.stdout.strip().splitlines()[-1]) == []
