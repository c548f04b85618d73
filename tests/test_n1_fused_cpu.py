"""tests/n1_fused_cases.py held to numpy (no GPU): every case's predicted outcome is the one it was built for, every outcome is
reached, and whatever the restated single-pass N1 settles -- from the restated sampler's brackets or from brackets perturbed by
hand, with or without heavy keys -- is np.nanmedian and the float32 MAD of the oracle, bit for bit."""
import numpy as np
import pytest

import n1_fused_cases as N

F32 = np.float32


def _bits(p):
    return [float(p["med"]), float(p["mad"]), float(p["lo"]), float(p["hi"])]


@pytest.fixture(scope="module")
def predictions():
    return {name: N.predict_case(N.case(name)) for name in N.NAMES}


@pytest.mark.parametrize("name", N.NAMES)
def test_case_gives_the_outcome_it_was_built_for(predictions, oracle_mod, name):
    c = N.case(name)
    for (x, Te), p, want in zip(N.minibatches(c), predictions[name], c["expect"]):
        assert p["outcome"] in N.OUTCOMES
        if want is not None:
            assert p["outcome"] == want, (name, p["outcome"], p["why"])
        if p["outcome"] == "settled":
            ref = N.oracle_params(oracle_mod, x, c["T"])
            assert _bits(p) == list(ref), (name, _bits(p), list(ref))
            assert p["counters"][5] == 1 and not p["counters"][6] and not p["counters"][7]


def test_every_outcome_is_reached_and_the_controls_settle(predictions):
    seen = {p["outcome"] for ps in predictions.values() for p in ps}
    assert seen == set(N.OUTCOMES), seen
    for name in N.CONTROLS:
        assert [p["outcome"] for p in predictions[name]] == ["settled"] * len(predictions[name]), name
    # each decline by the counter it was built for
    assert predictions["median_list_cap"][0]["counters"][18] == 1 and predictions["staging_overflow"][0]["counters"][19] == 1
    assert predictions["median_outside"][0]["counters"][6] == 1 and predictions["mad_outside"][0]["counters"][7] == 1
    assert len({N.CASE_GEOM[n] for n in N.NAMES}) == len(N.GEOM)


@pytest.mark.parametrize("name", N.HEAVY)
def test_grid_cases_count_their_median(predictions, name):
    """(with the stand-in's keys; the GPU test asserts the same of the device's)"""
    (p,) = predictions[name]
    assert p["counters"][22] > 0 and p["counters"][23] > 0
    assert p["used"]["D0"] == p["brackets"]["D0w"] and p["used"]["D1"] == p["brackets"]["D1w"]
    if name == "even_lower_heavy":
        keys = N.standin_heavy(*_mb0(name), p["brackets"])[0].astype(np.int64)
        lo, up = N.case(name)["middle"]
        assert p["med_lower_key"] in keys and p["med_key"] not in keys
        assert (N._k2f(p["med_lower_key"]), N._k2f(p["med_key"])) == (F32(lo), F32(up))
    else:
        assert p["med_heavy"]


def _mb0(name):
    c = N.case(name)
    x, Te = N.minibatches(c)[0]
    return x, Te, c["T"]


def test_even_counts_take_the_lower_value_from_below(predictions):
    for name, apart in (("even_lower_copied", None), ("even_lower_one_key", 1)):
        (p,) = predictions[name]
        lo, up = N.case(name)["middle"]
        assert p["n_valid"] % 2 == 0 and p["med_lower_key"] < p["med_key"]
        assert (N._k2f(p["med_lower_key"]), N._k2f(p["med_key"])) == (F32(lo), F32(up))
        assert p["med"] == F32(F32(F32(lo) + F32(up)) / F32(2.0))
        if apart:
            assert p["med_key"] - p["med_lower_key"] == apart


def test_tails_flag_changes_nothing(predictions):
    c = dict(N.case("tails"))
    assert {0, 1, 3, 2001, c["T"]} <= set(c["lens"].tolist())
    c["tails"] = False
    (a,), (b,) = predictions["tails"], N.predict_case(c)
    assert a["outcome"] == b["outcome"] == "settled" and _bits(a) == _bits(b)
    for k in ("med_s", "A0", "A1", "D0", "D1", "eps", "ok", "wide_ok", "D0w", "D1w"):
        assert a["brackets"][k] == b["brackets"][k], k


def _dataset(kind, rng, g, rows):
    T = g["T"]
    x = N._base(rng, (rows, T), g, centre=0.0 if kind == "zero" else 100.0)
    if kind == "grid":
        x = N._grid(x, 0.18)
    elif kind == "coarse":
        x = N._grid(x, 3.0)
    elif kind == "half_grid":
        x[0::2] = N._grid(x[0::2], 0.18)
    elif kind == "odd":
        x[1, 5] = np.nan
    elif kind == "nan_rows":
        x[0::3] = np.nan
    elif kind == "few":
        x[:, :] = np.nan
        x[0, :3] = [1.0, 2.0, 4.0]
    Te = np.full(rows, T)
    if kind == "tails":
        Te = np.minimum(T, (400 * (1.0 + rng.pareto(1.2, rows))).astype(np.int64))
        Te[:4] = [0, 1, 3, T]
        x[np.arange(T)[None, :] >= Te[:, None]] = np.nan
    return x, Te


def _hand_brackets(x, rng):
    """brackets round the true statistics, as the sampler would place them"""
    v = x[x == x]
    med = F32(np.median(v)) if v.size else F32(0)
    mad = F32(np.median(np.abs(v - med))) if v.size else F32(1)
    w = F32(max(float(mad) * 0.05, 1e-3))
    f = N.zero_brackets()
    f.update(med_s=F32(med + F32(rng.uniform(-0.5, 0.5)) * w), A0=-w, A1=w, eps=w, ok=1, wide_ok=1)
    e, e2 = F32(1.01) * w, F32(2.02) * w
    f["D0"], f["D1"] = F32(mad - w - e), F32(mad + w + e)
    f["D0w"], f["D1w"] = F32(mad - w - e2), F32(mad + w + e2)
    if not (f["D0"] > f["eps"] and f["D0w"] > f["eps"]):
        f["ok"] = 0
    return f


def _perturb(f, rng, how):
    """a bracket the sampler might as well have produced: A0 <= 0 < A1, eps = max(-A0, A1) < D0 < D1 stay (k_n1_fuse_setup)"""
    g = dict(f)
    eps = float(f["eps"])
    if how == "med_s":
        g["med_s"] = F32(f["med_s"] + F32(rng.uniform(-eps, eps)))
    elif how == "shift":
        d = F32(rng.uniform(-0.9, 0.9) * eps)
        g["A0"], g["A1"] = F32(min(f["A0"] + d, 0.0)), F32(max(f["A1"] + d, 1e-6))
    elif how == "narrow":
        s = F32(rng.choice([0.5, 0.1, 0.01, 0.001]))
        g["A0"], g["A1"] = F32(f["A0"] * s), F32(f["A1"] * s)
    elif how == "band":
        w = float(f["D1"]) - float(f["D0"])
        g["D0"], g["D1"] = F32(f["D0"] + F32(rng.uniform(-0.3, 0.6) * w)), F32(f["D1"] + F32(rng.uniform(-0.6, 0.3) * w))
    g["eps"] = F32(max(-g["A0"], g["A1"]))
    if not (g["D0"] > g["eps"] and g["D1"] > g["D0"]):
        return None
    return g


@pytest.mark.parametrize("geom", ["g4000", "g8192", "g16000", "cap"])
def test_whatever_settles_is_numpys(oracle_mod, geom):
    """>= 200 seeded trials per geometry.  No trial may settle to anything but the oracle's bits."""
    g = N.GEOM[geom]
    T = g["T"]
    rng = np.random.default_rng(77 + T)
    kinds = ["plain", "odd", "grid", "coarse", "half_grid", "nan_rows", "zero", "tails", "plain", "few"]
    tally = {o: 0 for o in N.OUTCOMES}
    trials = zero_settled = heavy_settled = 0
    for di, kind in enumerate(kinds):
        rows = g["n"] if di == 0 else max(16, g["n"] // 4)
        x, Te = _dataset(kind, rng, g, rows)
        ref = list(N.oracle_params(oracle_mod, x, T))
        fs = N.brackets(x, Te, T, rows)
        base = fs if fs["ok"] else _hand_brackets(x, rng)
        for trial in range(21):
            how = ["sampler", "med_s", "shift", "narrow", "band", "hand"][trial % 6]
            f = base if how == "sampler" else _hand_brackets(x, rng) if how == "hand" else _perturb(base, rng, how)
            if f is None or not f["ok"]:
                f = base
            wide = bool(trial % 2) and bool(f["wide_ok"]) and how in ("sampler", "hand")
            fu = N.use_band(f, wide)
            keys = np.zeros(0, dtype=np.uint32)
            if fu["ok"] and trial % 3:  # a random subset of the true in-zone values as heavy keys
                zc = np.array(sorted(N.zone_counts(x, Te, T, fu)), dtype=np.uint32)
                if zc.size:
                    keys = np.sort(rng.choice(zc, size=min(zc.size, int(rng.integers(1, N.N1H_MAX + 1))), replace=False))
            p = N.predict(x, Te, T, rows, keys, False, f=fu)
            trials += 1
            tally[p["outcome"]] += 1
            if p["outcome"] == "settled":
                assert _bits(p) == ref, (geom, kind, how, trial, _bits(p), ref)
                zero_settled += kind == "zero"
                heavy_settled += bool(keys.size and p["counters"][23])
    print(geom, "trials", trials, tally, "settled across zero", zero_settled, "with counted keys", heavy_settled)
    assert trials >= 200
    # (not vacuous: most trials settle, hand-made brackets whose keys span the sign and counted keys among them)
    assert tally["settled"] >= trials // 3 and zero_settled > 0 and heavy_settled > 0, (tally, zero_settled, heavy_settled)
