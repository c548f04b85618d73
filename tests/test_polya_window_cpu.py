"""The three-valued decision rule of the windowed pass 2 (peaks.h, find_peaks.h), restated in numpy by polya_window_cases.py, against
the oracle's find_peaks on the whole trace: whatever the rule decides from x[0:wend) is what the whole trace gives -- on pass-2 traces
of the synthetic generator, on hand-made traces that drive every branch, and on the batches of tests/test_gpu_polya_window.py, whose
preconditions (which reads the window settles, which it cannot) are asserted here without a GPU."""
import numpy as np
import pytest

import llr_stream_cases as lc
import llr_stream_oracle as so
import polya_window_cases as pw


def _check(oracle, g, wends, what):
    """decided => the whole trace's survivors and result; -> {wend: decided?}"""
    g = np.asarray(g, dtype=np.float64)
    want = pw.whole(oracle, g)
    assert pw.decide(g, len(g)) == want, (what, "the rule on the whole trace is find_peaks", pw.decide(g, len(g)), want)
    out = {}
    for we in wends:
        got = pw.decide(g, we)
        out[we] = got is not None
        if got is not None:
            assert got == want and pw.step5(g, *got) == pw.step5(g, *want), (what, we, got, want)
    return out


# ---------------------------------------------------------------- traces of the generator
def test_generator_traces_decided_means_the_whole_traces_answer(oracle_mod):
    """256 reads at geometry "pad" (L = 2049): window ends from a few dozen points behind the candidate up to the whole trace"""
    b = lc.make("pad", "pw_gen", [lc.geom_of("pad").L] * 256)
    ref = lc.reference(oracle_mod, b)
    n_dec = {w: 0 for w in (64, 128, 256, 512, 1024)}
    n_cand = 0
    for r, s in enumerate(ref):
        if s["cand"] < 0:
            continue
        n_cand += 1
        n, g = s["n_valid"], s["g2"]
        assert pw.step5(g, *pw.whole(oracle_mod, g)) == max(s["polya_idx"], 0), ("step 5 restated", r)
        wends = {w: min(n, s["cand"] + 1 + w) for w in n_dec}
        dec = _check(oracle_mod, g, sorted(set(wends.values()) | {1024, 2048}), ("pad", r))
        for w, we in wends.items():
            n_dec[w] += dec[we]
    print("reads with a candidate %d; decided inside a window of w points behind it: %s" % (n_cand, n_dec))
    assert n_cand >= 250
    assert n_dec[1024] >= 0.98 * n_cand and n_dec[64] < n_dec[1024]   # the window pays, and a short one does not settle everything


# ---------------------------------------------------------------- hand-made traces
def _tri(x, p, height, half):
    k = np.arange(-half, half + 1)
    x[p + k] += height * (1.0 - np.abs(k) / float(half))


def _base(n=800, slope=-0.01):
    return slope * np.arange(n, dtype=np.float64)


def _hand_made():
    """name -> (trace, {wend: decided?}, branches of the rule that must be met at the first wend)"""
    out = {}
    x = _base(); _tri(x, 100, 50.0, 15)                                   # noqa: E702
    out["one_peak_only"] = (x, {300: False, 800: True}, {"open_exact"})
    x = _base(); _tri(x, 100, 50.0, 15); _tri(x, 450, 30.0, 15)          # noqa: E702
    out["second_peak_beyond_the_window"] = (x, {300: False, 600: True, 800: True}, {"open_exact"})
    x = _base(); _tri(x, 100, 50.0, 15); _tri(x, 295, 30.0, 15)          # noqa: E702
    out["peak_on_the_seam"] = (x, {300: False, 400: True}, {"open_exact"})
    x = _base(); _tri(x, 100, 50.0, 15); _tri(x, 200, 30.0, 15)          # noqa: E702
    out["two_peaks_falling_base"] = (x, {300: True, 256: True}, {"open_exact"})
    x = _base(slope=0.01); _tri(x, 100, 50.0, 15); _tri(x, 200, 30.0, 15)   # noqa: E702
    out["two_peaks_rising_base"] = (x, {300: True}, {"bounds_pass"})
    x = _base(slope=0.01); _tri(x, 60, 60.0, 3); _tri(x, 100, 50.0, 15); _tri(x, 200, 30.0, 15)   # noqa: E702
    out["narrow_spike_first"] = (x, {300: True}, {"bounds_fail", "bounds_pass"})
    x = _base(slope=0.01); _tri(x, 100, 50.0, 15); _tri(x, 285, 5.0, 100)   # noqa: E702
    out["broad_peak_cut_by_the_window"] = (x, {300: False, 500: True}, {"bounds_pass", "bounds_unknown"})
    x = _base(slope=0.0); _tri(x, 100, 50.0, 15); x[200:] += 0.6 * np.arange(600)   # noqa: E702
    out["rise_through_the_windows_end"] = (x, {300: False}, {"exact"})
    x = _base(); _tri(x, 100, 50.0, 15); _tri(x, 200, 30.0, 15); x[296:306] = 5.0   # noqa: E702
    out["plateau_across_the_seam"] = (x, {300: False, 400: True}, set())
    x = _base(); _tri(x, 100, 50.0, 15); _tri(x, 200, 30.0, 15)          # noqa: E702
    x[20] = np.nan; x[60] = -np.inf; x[400] = np.inf
    out["nan_and_infinities"] = (x, {300: True, 512: True}, set())
    x = _base(); _tri(x, 100, 50.0, 15); _tri(x, 200, 30.0, 15); x[105] = x[100]   # noqa: E702
    out["equal_heights_within_the_distance"] = (x, {300: True}, set())
    x = _base(slope=0.02); x[::2] += 0.3; _tri(x, 100, 50.0, 15); _tri(x, 200, 30.0, 15)   # noqa: E702
    out["noise_on_a_rise"] = (x, {300: True}, {"reject_left"})
    x = _base(slope=0.0); _tri(x, 50, 0.5, 5); _tri(x, 100, 50.0, 15); _tri(x, 230, 30.0, 40); x[205] += 1.2   # noqa: E702
    out["bumps_below_the_prominence"] = (x, {300: True}, {"reject_left", "exact_prom_fail"})   # (one on the flat, one on the second peak's flank)
    return out


HAND = _hand_made()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_traces(oracle_mod, name):
    x, outcome, branches = HAND[name]
    dec = _check(oracle_mod, x, sorted(outcome), name)
    assert dec == outcome, (name, dec, outcome)
    why = []
    pw.decide(x, min(outcome), why)
    assert branches <= set(why), (name, branches, set(why))
    if name == "equal_heights_within_the_distance":
        assert pw.decide(x, 300) == (105, 200)        # the later of two equal maxima within the distance is the one kept
    if name == "nan_and_infinities":
        assert pw.decide(x, 300) == (100, 200)


def test_every_branch_of_the_rule_is_met():
    met = set()
    for x, outcome, _ in HAND.values():
        for we in outcome:
            pw.decide(x, we, why := [])
            met |= set(why)
    # (exact_prom_width_unknown guards values no finite trace of ordinary size produces: a height that rounding puts at or below
    # the right minimum, a NaN width)
    assert {"reject_left", "exact", "open_exact", "exact_prom_fail", "bounds_pass", "bounds_fail", "bounds_unknown"} <= met, met


# ---------------------------------------------------------------- the GPU test's batches
@pytest.mark.parametrize("name", pw.KINDS)
def test_gpu_batches_are_what_they_were_made_for(oracle_mod, name):
    b = pw.batch(name, oracle_mod)
    ref = lc.reference(oracle_mod, b)
    win = pw.window_of(name)
    pred = pw.predict(ref, win)
    live = [r for r, p in enumerate(pred) if p is not None]
    for r in live:
        _check(oracle_mod, ref[r]["g2"], [pred[r][0]], (name, r))
    redo = [r for r in live if not pred[r][1]]
    wends = {pred[r][0] for r in live}
    print("%-10s window %4d: %d reads with a candidate, window ends %s, %d undecided" % (name, win, len(live), sorted(wends), len(redo)))
    L = lc.geom_of(pw.GEOM).L
    if name == "ordinary":
        assert len(live) == pw.N and not redo and wends == {2048}
        _, n_cand, n_und = pw.ordinary_reads(oracle_mod)
        assert n_cand >= 90 and n_und <= 0.02 * n_cand, (n_cand, n_und)   # the pool itself: at most 2 % would be redone
    elif name in ("long_polya", "seam1024", "seam2048"):
        assert len(live) >= pw.N - 8 and redo == live and wends == {1024 if name == "seam1024" else 2048}
        if name != "long_polya":     # the poly(A) ends (the whole trace's first survivor) lie within 10 points of the seam, give or take the peak's own scatter
            seam = int(name[4:])
            ends = [pw.whole(oracle_mod, ref[r]["g2"])[0] for r in live]
            near = [e for e in ends if seam - 14 <= e <= seam + 14]    # (a read or two has a survivor in front of its poly(A) end)
            assert len(near) >= len(live) - 4 and len(set(near)) >= 15, ends
    elif name == "late":
        assert len(live) >= pw.N - 8 and wends == {L} and not redo
    elif name == "plateau":
        flat = [r for r in live if so.maxima(ref[r]["g2"], ref[r]["n_valid"], ref[r]["n_valid"] - 2)[2]]
        assert len(flat) >= 8 and wends == {2048}
        assert all(ref[r]["cand"] + 3 < 2048 for r in flat)      # the plateau lies inside the window
    elif name == "holes":
        holed = [r for r in live if np.isnan(ref[r]["g2"][: pred[r][0]]).any() or np.isnan(ref[r]["down"][: pred[r][0]]).any()]
        assert len(holed) >= 15 and wends == {2048}
    elif name == "shared":
        assert b.minibatch == 2 and all(ref[r] is None for r in range(pw.N) if r % 4 >= 2)
        none = [r for r in range(1, pw.N, 4) if ref[r]["cand"] < 0]
        assert len(none) >= 12 and len(live) >= 12, (len(none), len(live))
    else:
        assert {2048, 3072, L} <= wends
        per_group = [{pred[r][0] if pred[r] else None for r in range(q, q + 4)} for q in range(0, pw.N, 4)]
        assert sum(len(s - {None}) >= 3 for s in per_group) >= 12
        assert all(not pred[r][1] for r in range(3, pw.N, 4) if pred[r]) and sum(pred[r][1] for r in range(0, pw.N, 4) if pred[r]) >= 14
