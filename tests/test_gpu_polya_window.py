"""Pass 2 over a window of the trace (llr_stream.h, peaks.h; ADP_G2_WINDOW): k_gains<2> computes x[0 .. wend) only, k_polya_peak
decides from it where it can, the other reads go to a device-side redo list and through both kernels again on the whole trace.
Per case of polya_window_cases.py (geometry "tall": L = 4100, five 1024-point tiles; 64 reads):
  * poly(A) index and final rows (with start peak) are byte-equal between the default and ADP_G2_WINDOW=0, and the oracle's;
  * with the variable set for the staged call, wend is the restated one, and trace, bmax / bmin, npk / pk / pkv on [0, wend) are
    the whole-trace call's, bit for bit;
  * the tallies (debug counters 78 / 79: reads decided inside the window / sent to the redo list) and the redo list itself are
    what the rule restated in numpy predicts, and what the case was made for: ordinary reads -- nothing redone; poly(A) longer than
    the window, poly(A) end on a window seam -- every read redone; a candidate so late that the window covers the trace -- the
    read is a whole-trace read and counts as NEITHER (it never meets the window's code).
One grouped-execution setting: rows equal the ungrouped call's, window on."""
import os

import numpy as np
import pytest

import llr_stream_cases as lc
import llr_stream_oracle as so
import polya_window_cases as pw
import test_gpu_llr_stream as ts
from util import row_diffs

pytestmark = pytest.mark.gpu

SWITCH = "ADP_G2_WINDOW"


def _with_window(value, fn, extra=None):
    keys = [SWITCH] + list(extra or {})
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        if value is not None:
            os.environ[SWITCH] = str(value)
        os.environ.update(extra or {})
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engine():
    from adapted_amd import lib

    eng = lib.Engine(lc.spc_of(pw.GEOM), pw.N, lc.geom_of(pw.GEOM).m, device=0)
    yield eng
    eng.close()


def _tallies(eng):
    c = eng.debug_counters(80)
    return int(c[78]), int(c[79])


def _staged(eng, b, n):
    """the decoy, then the batch up to pass 2 and up to the poly(A) index -> the buffers behind each, and the tallies' growth"""
    ts._run(eng, b, 6)
    out = {"aidx": eng.debug_fetch(4, n), "trace": eng.debug_fetch(3, n), "bmax": eng.debug_fetch(15, n), "bmin": eng.debug_fetch(16, n),
           "npk": eng.debug_fetch(18, n), "pk": eng.debug_fetch(19, n), "pkv": eng.debug_fetch(20, n), "wend": eng.debug_fetch(22, n)}
    t0 = _tallies(eng)
    eng.debug_llr_upto(b.sig, b.lens, n, b.minibatch, 7)
    t1 = _tallies(eng)
    out["polya"] = eng.debug_fetch(5, n)
    out["wend7"] = eng.debug_fetch(22, n)
    out["redo"] = eng.debug_fetch(23, n)
    out["tally"] = (t1[0] - t0[0], t1[1] - t0[1])
    return out


def _oracle_rows(oracle, b):
    out = []
    for m0 in range(0, b.sig.shape[0], b.minibatch):
        sig, lens = b.sig[m0: m0 + b.minibatch], b.lens[m0: m0 + b.minibatch]
        try:
            out += oracle.detect_llr(sig, lens, lc.spc_of(b.geom), with_start_peak=True)
        except ValueError:
            out += [None] * sig.shape[0]     # a dropped minibatch: its rows are the exception's
    return out


@pytest.mark.parametrize("name", pw.KINDS)
def test_windowed_pass2(engine, oracle_mod, name):
    from adapted_amd import lib

    eng = engine
    b = pw.batch(name, oracle_mod)
    ref = lc.reference(oracle_mod, b)
    n, win = len(ref), pw.window_of(name)
    pred = pw.predict(ref, win)
    live = [r for r in range(n) if pred[r] is not None]
    want_redo = sorted(r for r in live if not pred[r][1])
    want_decided = sorted(r for r in live if pred[r][1] and pred[r][0] < ref[r]["n_valid"])

    # ---- the staged calls: whole traces (the variable unset), then the window
    whole = _with_window(None, lambda: _staged(eng, b, n))
    assert whole["tally"] == (0, 0)
    w = _with_window(win, lambda: _staged(eng, b, n))
    for r in live:
        s = ref[r]
        k, we = s["n_valid"], pred[r][0]
        assert int(whole["aidx"][r]) == int(w["aidx"][r]) == s["cand"]
        assert int(whole["wend"][r]) == int(whole["wend7"][r]) == k
        # (a read of the redo list ends with its whole trace: the windowed buffers are those behind stage 6, before any redo)
        assert int(w["wend"][r]) == we and int(w["wend7"][r]) == (k if r in want_redo else we), ("wend", r, int(w["wend"][r]), int(w["wend7"][r]), we, k)
    w6 = w
    for r in live:
        s = ref[r]
        k, we = s["n_valid"], pred[r][0]
        nb = (we + so.SUMBLK - 1) // so.SUMBLK
        assert ts._same(w6["trace"][r, :we], whole["trace"][r, :we]), ("trace", r, we)
        assert ts._same(w6["bmax"][r, :nb], whole["bmax"][r, :nb]) and ts._same(w6["bmin"][r, :nb], whole["bmin"][r, :nb]), ("summaries", r, we)
        idx, h, plateau = so.maxima(whole["trace"][r, :we], we, k - 2)
        assert (int(w6["npk"][r]) == -1) == plateau, ("npk", r, int(w6["npk"][r]), plateau)
        if not plateau:
            assert int(w6["npk"][r]) == idx.size and w6["pk"][r, : idx.size].tolist() == idx.tolist(), ("pk", r, we)
            assert ts._same(w6["pkv"][r, : idx.size], h), ("pkv", r, we)
            if int(whole["npk"][r]) >= 0:    # the whole list's front
                assert w6["pk"][r, : idx.size].tolist() == whole["pk"][r, : idx.size].tolist() and ts._same(w6["pkv"][r, : idx.size], whole["pkv"][r, : idx.size])

    # ---- the paths taken
    n_redo = int(w["redo"][0])
    got_redo = sorted(int(v) for v in w["redo"][1: 1 + n_redo])
    print("%-10s window %4d: wend %s; decided in the window %d, redone %d (restated rule: %d, %d)"
          % (name, win, sorted({pred[r][0] for r in live}), w["tally"][0], w["tally"][1], len(want_decided), len(want_redo)))
    assert got_redo == want_redo and w["tally"] == (len(want_decided), len(want_redo)), (got_redo, want_redo, w["tally"])
    if name == "ordinary":
        assert n_redo <= 0.02 * len(live) and w["tally"][0] == len(live) == pw.N
    elif name in ("long_polya", "seam1024", "seam2048"):
        assert got_redo == live and w["tally"] == (0, len(live))
    elif name == "late":       # wend == n: a whole-trace read inside a windowed call, counted as neither
        assert w["tally"] == (0, 0) and all(pred[r][0] == ref[r]["n_valid"] for r in live)
    elif name == "plateau":    # the recount inside the window
        assert sum(int(w6["npk"][r]) == -1 for r in live) >= 8 and n_redo <= len(live) // 4
    elif name == "mixed":
        assert w["tally"][0] >= 14 and w["tally"][1] >= 14

    # ---- results: the poly(A) index and the final rows
    for r, s in enumerate(ref):
        if s is not None:
            exp = max(s["polya_idx"], 0) if s["cand"] >= 0 else 0
            assert int(whole["polya"][r]) == int(w["polya"][r]) == exp, ("polya_idx", r, int(whole["polya"][r]), int(w["polya"][r]), exp)
    t0 = _tallies(eng)
    rows_d, mbs_d = _with_window(None, lambda: eng.detect_llr_rows(b.sig, b.lens, n, b.minibatch, with_start_peak=True))
    t1 = _tallies(eng)
    rows_0, mbs_0 = _with_window(0, lambda: eng.detect_llr_rows(b.sig, b.lens, n, b.minibatch, with_start_peak=True))
    t2 = _tallies(eng)
    assert t2 == t1                                   # ADP_G2_WINDOW=0: the window's code is not met
    if win == 1024:                                   # the default window is the case's
        assert (t1[0] - t0[0], t1[1] - t0[1]) == w["tally"]
    assert rows_d.tobytes() == rows_0.tobytes() and mbs_d.tobytes() == mbs_0.tobytes()
    exp = _oracle_rows(oracle_mod, b)
    pub = [None if e is None else {k: v for k, v in e.items() if not k.startswith("_")} for e in exp]
    bad = [(r, row_diffs(g, e)[:4]) for r, (g, e) in enumerate(zip(lib.rows_to_results(rows_d, "llr"), pub)) if e is not None and row_diffs(g, e)]
    assert not bad, bad[:4]


def test_grouped_execution_with_the_window(engine, oracle_mod):
    b = pw.batch("mixed", oracle_mod)
    n = b.lens.size
    plain, _ = _with_window(None, lambda: engine.detect_llr_rows(b.sig, b.lens, n, 8, with_start_peak=True))
    t0 = _tallies(engine)
    grouped, _ = _with_window(None, lambda: engine.detect_llr_rows(b.sig, b.lens, n, 8, with_start_peak=True), {"ADP_GROUPS": "6", "ADP_LANES": "3"})
    t1 = _tallies(engine)
    assert t1[0] - t0[0] >= 8 and t1[1] - t0[1] >= 8       # the groups ran the window and its redo
    assert plain.tobytes() == grouped.tobytes()
