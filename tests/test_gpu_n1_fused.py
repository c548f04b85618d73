"""The single-pass N1 (adapted_amd/csrc/n1_fused.h) outcome by outcome: the cases of tests/n1_fused_cases.py forced through it
(ADP_N1_FUSED_MIN=1) with only N1 running (debug_llr_upto stage 1, so tallies 17..19 are N1's), and everything it leaves behind
(Engine.debug_n1_fused) held to the numpy restatement: the brackets bit for bit, the heavy keys' counts, the outcome the
predictor derives from them against the tallies and the `fused` flag, and the N1 parameters against the oracle -- settled or
declined, they are numpy's."""
import time

import numpy as np
import pytest

import n1_fused_cases as N

pytestmark = pytest.mark.gpu

FIELDS = ("med_s", "A0", "A1", "eps", "D0w", "D1w")


@pytest.fixture(scope="module")
def hip():
    from adapted_amd import lib

    L = lib.load()
    assert L.adp_device_count() >= 1, L.adp_last_error()
    return lib


def _bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def check_minibatch(x, Te, c, st, params, oracle_mod, want):
    """one minibatch's fetched state `st` against the restatement -> the prediction made from the device's keys and band"""
    T = c["T"]
    fs = N.brackets(x, Te, T, c["mb"], c["vec"])
    for k in FIELDS:
        assert _bits(st[k]) == _bits(fs[k]), (c["name"], k, st[k], fs[k])
    assert (st["ok"], st["wide_ok"]) == (fs["ok"], fs["wide_ok"]), (c["name"], st["ok"], st["wide_ok"], fs)
    nh = st["nh"]
    wide = bool(nh > 0 and fs["wide_ok"] and _bits(st["D0"]) == _bits(fs["D0w"]))
    fu = N.use_band(fs, wide)
    assert (_bits(st["D0"]), _bits(st["D1"])) == (_bits(fu["D0"]), _bits(fu["D1"])), (c["name"], st["D0"], st["D1"], fu)
    keys, counts = st["keys"][:nh], st["counts"][:nh]
    assert nh <= N.N1H_MAX and (np.diff(keys.astype(np.int64)) > 0).all(), keys
    assert not st["counts"][nh:].any()
    if fs["ok"]:
        zc = N.zone_counts(x, Te, T, fu)
        assert [zc.get(int(k), 0) for k in keys] == counts.tolist(), (c["name"], keys, counts)
    else:
        assert nh == 0
    p = N.predict(x, Te, T, c["mb"], keys, wide, f=fs, vec=c["vec"])
    if want is not None:
        assert p["outcome"] == want, (c["name"], p["outcome"], p["why"])
    assert st["fused"] == int(p["outcome"] == "settled"), (c["name"], st["fused"], p["outcome"], p["why"])
    ref = list(N.oracle_params(oracle_mod, x, T))
    assert list(params) == ref or (np.isnan(ref[0]) and np.isnan(params[0])), (c["name"], list(params), ref)
    if p["outcome"] == "settled":
        assert [float(p[k]) for k in ("med", "mad", "lo", "hi")] == ref, (c["name"], p, ref)
        assert st["status"] == (1 if p["mad_zero"] else 0)
    p["wide"] = wide
    return p


def run_case(hip, oracle_mod, c, tails=None):
    tails = c["tails"] if tails is None else tails
    n_mb = (c["n"] + c["mb"] - 1) // c["mb"]
    eng = hip.Engine(N.make_spc(c["T"]), c["n"], c["m"], device=0)
    try:
        c0 = eng.debug_counters(24).astype(np.int64)
        t0 = time.perf_counter()
        eng.debug_llr_upto(c["sig"], c["lens"], c["n"], c["mb"], 1, tails_nan=tails)
        d = eng.debug_counters(24).astype(np.int64) - c0
        t_dev = time.perf_counter() - t0
        st = eng.debug_n1_fused(n_mb)
        params = eng.debug_norm_params(n_mb)
    finally:
        eng.close()
    cc = dict(c, tails=tails)
    preds = [check_minibatch(x, Te, cc, st[i], params[i], oracle_mod, c["expect"][i]) for i, (x, Te) in enumerate(N.minibatches(cc))]
    for k in N.COUNTERS:
        exp = [p["counters"][k] for p in preds]
        if None not in exp:
            assert d[k] == sum(exp), (c["name"], "g_dbg[%d]" % k, int(d[k]), exp, [p["why"] for p in preds])
    assert d[22] == sum(s["nh"] for s in st) and d[23] == sum(int(s["counts"].sum()) for s in st)
    print("%-20s %s  device call %.3f s  g_dbg %s" % (c["name"], [p["outcome"] for p in preds], t_dev, {k: int(d[k]) for k in N.COUNTERS}))
    return preds, st, params, d


@pytest.mark.parametrize("name", N.NAMES)
def test_case(hip, oracle_mod, monkeypatch, name):
    monkeypatch.setenv("ADP_N1_FUSED_MIN", "1")
    c = N.case(name)
    preds, st, params, d = run_case(hip, oracle_mod, c)
    # what the case was built for, by the tally that says so
    if name in N.CONTROLS:
        assert d[5] == len(preds) and d[6] == 0 and d[7] == 0 and all(s["fused"] for s in st)
    if c["expect"][0] == "not_set_up":
        assert not d[5] and not d[6] and not d[7] and not st[0]["ok"] and not st[0]["fused"]
    if name == "median_outside":
        assert d[6] == 1 and not d[17] and not d[18] and not d[19]
    if name == "mad_outside":
        assert d[7] == 1 and d[6] == 0
    if name == "median_list_cap":
        assert d[18] == 1 and d[6] == 1 and d[19] == 0
    if name == "staging_overflow":
        assert d[19] == 1 and d[6] == 1
    if name in N.HEAVY:
        (p,) = preds
        assert d[22] > 0 and d[23] > 0 and p["wide"], (d[22], d[23], p["wide"])
        keys = st[0]["keys"][:st[0]["nh"]].astype(np.int64)
        if name == "even_lower_heavy":  # the lower middle value is a counted one, the upper one a copied one
            assert p["med_lower_key"] in keys and p["med_key"] not in keys
        else:
            assert p["med_heavy"]
    if name == "tails":  # the flag off: NaN behind the reads' ends are read and counted for nothing -- the same bits
        preds2, st2, params2, _ = run_case(hip, oracle_mod, c, tails=False)
        assert params2.tobytes() == params.tobytes()
        for k in FIELDS + ("D0", "D1"):
            assert _bits(st2[0][k]) == _bits(st[0][k]), k
        assert st2[0]["fused"] == st[0]["fused"] == 1
    if name == "two_minibatches":
        assert len(preds) == 2 and c["n"] % c["mb"] != 0


def test_not_the_fused_route_is_an_error(hip, monkeypatch):
    """below ADP_N1_FUSED_MIN the call takes n1_select.h's passes alone: there is no fused state to fetch"""
    monkeypatch.setenv("ADP_N1_FUSED_MIN", str(1 << 40))
    c = N.case("odd_count")
    eng = hip.Engine(N.make_spc(c["T"]), c["n"], c["m"], device=0)
    try:
        eng.debug_llr_upto(c["sig"], c["lens"], c["n"], c["mb"], 1)
        with pytest.raises(hip.HipLibraryError):
            eng.debug_n1_fused(1)
    finally:
        eng.close()


def test_int16_rows_give_the_float32_run_of_their_calibrated_values(hip, oracle_mod, monkeypatch):
    """k_n1_fused<SigI16> and the sampling kernels on raw int16 + per-read calibration (detect_llr_rows_i16: the whole pipeline
    runs, so only tallies 5..7, 22, 23 are N1's): brackets, heavy keys, counts and N1 parameters are those of the float32 run
    over the calibrated values (calibrate_i16), which check_minibatch holds to the restatement and the oracle."""
    monkeypatch.setenv("ADP_N1_FUSED_MIN", "1")
    c = dict(N.case("adc_grid"))
    n, m = c["n"], c["m"]
    raw = np.round(c["sig"] / np.float32(0.18)).astype(np.int16)
    scale, offset = np.full(n, 0.18, dtype=np.float32), np.zeros(n, dtype=np.float32)
    eng = hip.Engine(N.make_spc(c["T"]), n, m, device=0)
    d_raw, d_len, d_cal, d_f32 = eng.dev_alloc(raw.nbytes + 64), eng.dev_alloc(n * 4), eng.dev_alloc(2 * n * 4), eng.dev_alloc(n * m * 4)
    try:
        eng.h2d(d_raw, raw)
        eng.h2d(d_len, c["lens"])
        eng.h2d(d_cal, np.concatenate([scale, offset]))
        cal = np.zeros((n, m), dtype=np.float32)
        eng.calibrate_i16(d_raw, d_len, d_cal, d_cal + n * 4, n, d_f32)
        eng.d2h(cal, d_f32)
        c0 = eng.debug_counters(24).astype(np.int64)
        eng.detect_llr_rows_i16(d_raw, d_len, d_cal, d_cal + n * 4, n, n)
        d = eng.debug_counters(24).astype(np.int64) - c0
        st16, p16 = eng.debug_n1_fused(1)[0], eng.debug_norm_params(1)[0]
        eng.debug_llr_upto(cal, c["lens"], n, n, 1)
        st32, p32 = eng.debug_n1_fused(1)[0], eng.debug_norm_params(1)[0]
    finally:
        for p in (d_raw, d_len, d_cal, d_f32):
            eng.dev_free(p)
        eng.close()
    for k in FIELDS + ("D0", "D1"):
        assert _bits(st16[k]) == _bits(st32[k]), k
    for k in ("ok", "wide_ok", "fused", "status", "nh", "sample_in"):
        assert st16[k] == st32[k], k
    assert st16["keys"].tolist() == st32["keys"].tolist() and st16["counts"].tolist() == st32["counts"].tolist()
    assert p16.tobytes() == p32.tobytes()
    c.update(sig=cal)
    (x, Te), = N.minibatches(c)
    p = check_minibatch(x, Te, c, st32, p32, oracle_mod, "settled")
    assert [int(d[k]) for k in (5, 6, 7)] == [1, 0, 0] and st16["fused"] == 1
    assert d[22] == st16["nh"] > 0 and d[23] == int(st16["counts"].sum()) > 0 and p["wide"]
