"""The LLR trace module drop-in (adapted_amd/detect/llr.py -> adp_llr_trace_bounds / adp_llr_trace_peaks / adp_llr_spike_peak,
adapted_amd/csrc/trace_peaks_api.h) against the vectors of the REAL reference (tests/golden/llr_module.npz and the per-read stage
dumps tests/golden/*.stages.npz) and, on many synthetic traces, against the CPU restatement (tests/llr_module_restated.py).

Traces the device computes from raw signals may differ from glibc-based ones in the last bit.  Where such
a trace gives another peak index than the reference, the difference is allowed only when the restatement, run on the DEVICE's
trace, gives the device's answer and the two traces agree to 1e-9 of their scale: the index then follows from the last bits.
Those cases are counted and reported; the expectation is none.  Traces given as arrays must give the reference's results exactly."""
import glob
import os

import numpy as np
import pytest

import llr_module_cases as M
import llr_module_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "llr_module.npz")
MARGIN = []


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def L():
    from adapted_amd.detect import llr

    return llr


def _state(t):
    return np.array([t.start, t.end, int(bool(t.early_stop))], dtype=np.int64)


def _close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)) or not np.array_equal(got == 0, want == 0):
        return False
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin], want[~fin], equal_nan=True):
        return False
    # (the tolerance of test_gpu_trace_api.py: a gain is a difference of large terms)
    return not fin.any() or float(np.max(np.abs(got[fin] - want[fin]))) <= 1e-9 * max(1.0, float(np.max(np.abs(want[fin]))))


def _same(got, want, explain=None, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return
    # a margin case: the restatement on the device's own trace gives the device's result
    assert explain is not None and explain(), (what, got, want)
    MARGIN.append(what)


def _peaks(oracle_mod, gold, L, key, t, fp, ae, exact):
    got = L.find_peaks_in_trace(t, fp[0], fp[1], fp[2])
    ex = None if exact else (lambda: np.array_equal(R.find_peaks_in_trace(oracle_mod, t.signal, t.start, t.end, *fp), got))
    _same(got, gold[key + ".fp"], ex, key + ".fp")
    for a in (0, 1):
        for b in (0, 1):
            got = L.adapter_end_from_trace(t, ae[0], ae[1], ae[2], bool(a), bool(b))
            ex = None if exact else (lambda: np.array_equal(
                R.adapter_end_from_trace(oracle_mod, t.signal, t.start, t.end, ae[0], ae[1], ae[2], bool(a), bool(b)), got))
            _same(got, gold["%s.ae%d%d" % (key, a, b)], ex, "%s.ae%d%d" % (key, a, b))


@pytest.mark.parametrize("case", M.SIGNAL_CASES, ids=[c["name"] for c in M.SIGNAL_CASES])
def test_signal_cases(oracle_mod, gold, L, case):
    nm = "sig." + case["name"]
    raw = M.raw_of(case)
    n, w = raw.size, case["win"]
    t = L.calc_adapter_trace(raw, case["oh"], case["ot"], case["stride"], w[0], w[1], w[2], w[3], True,
                             adapter_early_stopping=case["aes"], polya_early_stopping=case["pes"])
    assert isinstance(t, L.LLRTrace) and type(t.start) is int and type(t.end) is int and type(t.early_stop) is bool
    assert t.stride_interp is (True if case["stride"] > 1 else None)
    _same(_state(t), gold[nm + ".bounds"], None, nm + ".bounds")
    if case["store"]:
        assert _close(t.signal, gold[nm + ".signal"])
    _peaks(oracle_mod, gold, L, nm, t, case["fp"], case["ae"], exact=False)
    ae = gold[nm + ".ae11"]
    a_end = int(ae[0]) if ae.size else n // 4
    pt = L.calc_polya_trace(t.c, t.c2, a_end, t.end, 50, case["stride"])
    _same(_state(pt), gold[nm + ".pbounds"], None, nm + ".pbounds")
    ft = L.calc_full_polya_trace(raw, a_end)
    _same(_state(ft), gold[nm + ".fbounds"], None, nm + ".fbounds")
    got = L.detect_full_polya_trace_peak_with_spike(ft.signal[a_end:])
    _same(np.array([got], dtype=np.int64), gold[nm + ".spike"], lambda: R.spike(oracle_mod, ft.signal[a_end:]) == got, nm + ".spike")


@pytest.mark.parametrize("case", M.TRACE_CASES, ids=[c["name"] for c in M.TRACE_CASES])
def test_trace_cases(oracle_mod, gold, L, case):
    nm = "tr." + case["name"]
    y = M.trace_of(case["trace"])
    if nm + ".error" in gold:
        with pytest.raises(ValueError):
            L.LLRTrace(signal=y.copy(), stride=case["stride"], min_obs=case["min_obs"], tail_trim=case["tail_trim"])
        return
    t = L.LLRTrace(signal=y.copy(), stride=case["stride"], min_obs=case["min_obs"], tail_trim=case["tail_trim"])
    _same(_state(t), gold[nm + ".bounds"], None, nm + ".bounds")
    assert bool(t.early_stop) == bool(t.end < t.max_len_no_early_stop)
    if case["store"]:
        assert np.array_equal(t.signal, gold[nm + ".signal"], equal_nan=True)  # (bit for bit: np.interp's formula)
    _peaks(oracle_mod, gold, L, nm, t, case["fp"], case["ae"], exact=True)


@pytest.mark.parametrize("k", range(len(M.CORRECTION_CASES)))
def test_corrections(gold, L, k):
    tn, peak, s, t, window, prom = M.CORRECTION_CASES[k]
    y = M.trace_of(M.by_name(M.TRACE_CASES, tn)["trace"])
    a = L.correct_for_plateau(y, peak, s, t, window)
    b = L.correct_for_split_peak(y, peak, s, t, window, prom)
    assert [int(a), int(b)] == gold["cor%d" % k].tolist()
    assert type(a) is int or isinstance(a, np.integer)


@pytest.mark.parametrize("case", M.SPIKE_CASES, ids=[c["name"] for c in M.SPIKE_CASES])
def test_spike_cases(gold, L, case):
    nm = "spk." + case["name"]
    y = M.trace_of(case["trace"])
    got = L.detect_full_polya_trace_peak_with_spike(y, case["d"], case["prom"], case["width"], case["ratio"], float(gold[nm + ".thr"]))
    assert got == int(gold[nm])
    if int(gold[nm]) == 0:
        assert type(got) is int
    else:
        assert isinstance(got, np.integer)


def test_fixture_cases_stacked_through_the_batch_forms(gold, L):
    """every trace case (and every spike case) in one padded batch: the batch forms give the per-read results"""
    cases = [c for c in M.TRACE_CASES if "tr.%s.error" % c["name"] not in gold and c["stride"] == 1]
    ys = [M.trace_of(c["trace"]) for c in cases]
    Lmax = max(y.size for y in ys)
    x = np.full((len(ys), Lmax), np.nan)
    for r, y in enumerate(ys):
        x[r, :y.size] = y
    lens = np.array([y.size for y in ys])
    eng = L._engine()
    st, en, es = eng.llr_trace_bounds(x.copy(), lens, [c["min_obs"] for c in cases], [c["tail_trim"] for c in cases], 1, False)
    for r, c in enumerate(cases):
        assert [st[r], en[r], es[r] & 1] == gold["tr.%s.bounds" % c["name"]].tolist(), c["name"]
    for a in (0, 1):
        for b in (0, 1):
            # one parameter set per call: group the cases by (prominence, rel_height, width)
            for ae in sorted({c["ae"] for c in cases}):
                idx = [r for r, c in enumerate(cases) if c["ae"] == ae]
                pk, cnt = L.adapter_end_from_trace_batch(x[idx], lens[idx], st[idx], en[idx], ae[0], ae[1], ae[2], bool(a), bool(b), cap=2)
                for j, r in enumerate(idx):
                    want = gold["tr.%s.ae%d%d" % (cases[r]["name"], a, b)]
                    assert pk[j, :cnt[j]].tolist() == want.astype(np.int64).tolist(), (cases[r]["name"], a, b)
                    assert (pk[j, cnt[j]:] == -1).all()
    sp = [c for c in M.SPIKE_CASES if c["d"] == 10 and c["prom"] == 1.0 and c["width"] == 10 and c["ratio"] == 0.5 and c["r2"] == 0.99]
    ys = [M.trace_of(c["trace"]) for c in sp]
    x = np.zeros((len(ys), max(y.size for y in ys)))
    for r, y in enumerate(ys):
        x[r, :y.size] = y
    got = L.detect_full_polya_trace_peak_with_spike_batch(x, [y.size for y in ys])
    assert got.dtype == np.int64
    assert got.tolist() == [int(gold["spk." + c["name"]]) for c in sp]


def _stage_files():
    return sorted(f for f in glob.glob(os.path.join(HERE, "golden", "*.stages.npz")) if "down_" in " ".join(np.load(f).files))


def test_reference_stage_dumps(oracle_mod, L):
    """the per-read dumps of the reference (oracle/gen_golden.py:183-197): down -> g1 / t1 (calc_adapter_trace), g1 -> p1
    (find_peaks_in_trace) and cands (adapter_end_from_trace), g2 -> p4 (detect_full_polya_trace_peak_with_spike)"""
    from golden_cases import CASES
    from util import make_spc

    files = _stage_files()
    assert files
    nread = 0
    for f in files:
        name = os.path.basename(f)[: -len(".stages.npz")]
        spc = make_spc(CASES[name])
        lb = spc.llr_boundaries
        w = lb.adapter_peak_width // spc.core.downscale_factor
        d = np.load(f)
        for k in d["dump_idx"].tolist():
            if "down_%d" % k not in d.files:
                continue
            nread += 1
            s_ = d["down_%d" % k].astype(np.float64)
            tr = L.calc_adapter_trace(s_, 5, 5, 1, 0, 0, 0, 0, True, 0, None, 0, 0, None, None)
            assert _close(tr.signal, d["g1_%d" % k]), (name, k)
            assert [tr.start, tr.end] == d["t1_%d" % k].tolist(), (name, k)
            # the reference's trace as the input: exact
            t1 = L.LLRTrace(signal=d["g1_%d" % k].copy(), stride=1, min_obs=5, tail_trim=5)
            p1 = L.find_peaks_in_trace(t1, w, lb.adapter_peak_prominence, lb.adapter_peak_rel_height)
            assert p1.tolist() == d["p1_%d" % k].tolist(), (name, k)
            cands = L.adapter_end_from_trace(t1, lb.adapter_peak_prominence, lb.adapter_peak_rel_height, w, True, True)
            assert np.asarray(cands, dtype=np.int64).tolist() == d["cands_%d" % k].tolist(), (name, k)
            # and the device's own trace
            p1d = L.find_peaks_in_trace(tr, w, lb.adapter_peak_prominence, lb.adapter_peak_rel_height)
            if p1d.tolist() != d["p1_%d" % k].tolist():
                assert p1d.tolist() == R.find_peaks_in_trace(oracle_mod, tr.signal, tr.start, tr.end, w, lb.adapter_peak_prominence,
                                                             lb.adapter_peak_rel_height).tolist()
                MARGIN.append("%s.p1_%d" % (name, k))
            if "g2_%d" % k in d.files:
                tr2 = L.calc_adapter_trace(s_, 1, 1, 1, 0, 0, 0, 0, False, int(d["cands_%d" % k][0]), None, 0, 0, tr.c, tr.c2)
                assert _close(tr2.signal, d["g2_%d" % k]), (name, k)
                assert L.detect_full_polya_trace_peak_with_spike(d["g2_%d" % k]) == int(d["p4_%d" % k][0]), (name, k)
                got = L.detect_full_polya_trace_peak_with_spike(tr2.signal)
                if got != int(d["p4_%d" % k][0]):
                    assert got == R.spike(oracle_mod, tr2.signal)
                    MARGIN.append("%s.p4_%d" % (name, k))
    assert nread >= 20
    print("stage dumps: %d reads, margin cases so far: %d %s" % (nread, len(MARGIN), MARGIN))


def _mixed_traces(n, seed=11, Lmax=30_000):
    """n synthetic reads (adapted_amd/synth.py) of mixed lengths with NaN holes, constant runs and quantised rows, pooled-like
    (scaled to pA and cut to <= Lmax), through the DEVICE's calc_adapter_trace_batch (offsets 5 / 5, stride 1)"""
    from adapted_amd.detect import llr
    from adapted_amd.synth import synth_read

    rng = np.random.default_rng(seed)
    lens = rng.integers(2, Lmax, n)
    lens[:4] = (1, 2, 3, 250)
    raw = np.zeros((n, int(lens.max())))
    for r in range(n):
        m = int(lens[r])
        x = synth_read(seed, r, m, m).astype(np.float64)
        kind = r % 5
        if kind == 1 and m > 20:
            x[int(rng.integers(0, m))] = np.nan
        elif kind == 2 and m > 20:
            a = int(rng.integers(0, m // 2))
            x[a: a + m // 3] = x[a]
        elif kind == 3:
            x = np.round(x * 2.0) / 2.0
        raw[r, :m] = x
    g, st, en, es, c, c2 = llr.calc_adapter_trace_batch(raw, lens, 5, 5, 1, 0, 0, 0, 0, True, adapter_early_stopping=0,
                                                        polya_early_stopping=0)
    return g, lens, st, en


def _check_batch_against_restatement(oracle_mod, L, g, lens, st, en, width, prom, rel):
    pk, cnt = L.adapter_end_from_trace_batch(g, lens, st, en, prom, rel, width, True, True)
    fp, fcnt = L.find_peaks_in_trace_batch(g, lens, st, en, width, prom, rel)
    spk = L.detect_full_polya_trace_peak_with_spike_batch(g, lens)
    walked = 0
    for r in range(g.shape[0]):
        y = g[r, :lens[r]]
        want = R.adapter_end_from_trace(oracle_mod, y, int(st[r]), int(en[r]), prom, rel, width, True, True)
        assert pk[r, :cnt[r]].tolist() == np.asarray(want, dtype=np.int64).tolist(), r
        wf = R.find_peaks_in_trace(oracle_mod, y, int(st[r]), int(en[r]), width, prom, rel)
        assert fp[r, :fcnt[r]].tolist() == wf.tolist(), r
        assert int(spk[r]) == R.spike(oracle_mod, y), r
        # the bounds the batch gave are LLRTrace's
        s = R.trace_state(y, 1, 5, 5) if y.size else None
        if s is not None:
            assert (s["start"], s["end"]) == (int(st[r]), int(en[r])), r
        walked += int(fcnt[r])
    return walked


def test_mixed_synthetic_reads(oracle_mod, L):
    g, lens, st, en = _mixed_traces(2000)
    n_peaks = _check_batch_against_restatement(oracle_mod, L, g, lens, st, en, 20, 1.0, 0.5)
    n_peaks += _check_batch_against_restatement(oracle_mod, L, g, lens, st, en, 200, 0.3, 1.0)
    print("mixed reads: 2000, peaks compared: %d" % n_peaks)


def test_window_batch_2000x20150(oracle_mod, L):
    """the 200 k window pooled by 10: 2000 traces of 20 150 points"""
    from adapted_amd.synth import synth_read

    n, m = 2000, 20150
    raw = np.zeros((n, m))
    for r in range(n):
        raw[r] = synth_read(5, r, 10 * m, 10 * m).astype(np.float64).reshape(m, 10).mean(axis=1)
    g, st, en, es = L.calc_adapter_trace_batch(raw, np.full(n, m), 5, 5, 1, 0, 0, 0, 0, adapter_early_stopping=0, polya_early_stopping=0)
    _check_batch_against_restatement(oracle_mod, L, g, np.full(n, m), st, en, 200, 1.0, 1.0)


def test_cap_overflow_equals_uncapped(L):
    ys = [M.trace_of(M.by_name(M.TRACE_CASES, nm)["trace"]) for nm in ("multi_many", "multi", "split", "no_peaks")]
    x = np.zeros((len(ys), max(y.size for y in ys)))
    for r, y in enumerate(ys):
        x[r, :y.size] = y
    lens = np.array([y.size for y in ys])
    st = np.array([int(np.argmin(y <= 0)) for y in ys])
    en = np.array([int(y.size - np.argmin(y[::-1] <= 0) - 1) for y in ys])
    for fix in (False, True):
        p1, c1 = L.adapter_end_from_trace_batch(x, lens, st, en, 0.1, 0.5, 5, fix, fix, cap=1)
        p64, c64 = L.adapter_end_from_trace_batch(x, lens, st, en, 0.1, 0.5, 5, fix, fix, cap=64)
        assert c1.tolist() == c64.tolist() and c1.max() > 1
        for r in range(len(ys)):
            assert p1[r, :c1[r]].tolist() == p64[r, :c64[r]].tolist()


def test_device_pointer_path(L):
    from adapted_amd.detect import _c_llr

    eng = _c_llr._engine()
    ys = [M.trace_of(M.by_name(M.TRACE_CASES, nm)["trace"]) for nm in ("multi", "strided10", "split", "plateau")]
    Lm = max(y.size for y in ys)
    x = np.zeros((len(ys), Lm))
    for r, y in enumerate(ys):
        x[r, :y.size] = y
    lens = np.array([y.size for y in ys])
    d = eng.dev_alloc(x.nbytes)
    try:
        eng.h2d(d, x)
        st, en, es = eng.llr_trace_bounds(d, lens, [5] * 4, [5] * 4, 10, True, n=len(ys), L=Lm)
        hx = x.copy()
        hst, hen, hes = eng.llr_trace_bounds(hx, lens, [5] * 4, [5] * 4, 10, True)
        assert st.tolist() == hst.tolist() and en.tolist() == hen.tolist() and es.tolist() == hes.tolist()
        back = np.zeros_like(x)
        eng.d2h(back, d)
        assert np.array_equal(back, hx, equal_nan=True)  # (interpolated in place on the device)
        pk, cnt = L.adapter_end_from_trace_batch(d, lens, st, en, 0.5, 0.5, 20, True, True, n=len(ys), L=Lm, cap=1)
        hpk, hcnt = L.adapter_end_from_trace_batch(hx, lens, st, en, 0.5, 0.5, 20, True, True, cap=1)
        assert cnt.tolist() == hcnt.tolist() and pk.tolist() == hpk.tolist()
        s = L.detect_full_polya_trace_peak_with_spike_batch(d, lens, n=len(ys), L=Lm)
        assert s.tolist() == L.detect_full_polya_trace_peak_with_spike_batch(hx, lens).tolist()
    finally:
        eng.dev_free(d)


def test_report_margin_cases():
    print("margin cases (an index explained by the trace's last bits): %d %s" % (len(MARGIN), MARGIN))
