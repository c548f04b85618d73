"""The MVS poly(A) module drop-in (adapted_amd/detect/mvs.py -> adp_mvs_check / adp_mvs_detect_at_loc / adp_mvs_detect,
adapted_amd/csrc/mvs_api.h) against the vectors of the REAL reference (tests/golden/mvs_module.npz: values, dtypes, Python types
and exceptions, exactly) and, on many synthetic reads in every dtype, against the CPU restatement (tests/mvs_module_restated.py):
indices, flags, statuses and float values identical, no tolerance."""
import os
import types
import warnings

import numpy as np
import pytest

import mvs_module_cases as M
import mvs_module_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "mvs_module.npz")
RESTATED = types.SimpleNamespace(mean_var_shift_polyA_check=R.check, mean_var_shift_polyA_detect_at_loc=R.detect_at_loc,
                                 mean_var_shift_polyA_detect=R.detect)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def mvs():
    from adapted_amd.detect import mvs

    return mvs


def _cfg():
    from adapted_amd.config.schema import MVSPolyAConfig, StreamingConfig

    return MVSPolyAConfig, StreamingConfig


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES])
def test_dropins_match_reference(gold, mvs, name):
    mc, sc = _cfg()
    case = M.by_name(name)
    x64, ae, pe, loc = M.inputs(case)
    mp, sp = M.mvs_params(mc, case), M.stream_params(sc, case)
    for dt in M.DTYPES + ("i16",):
        x = M.as_dtype(x64, dt)
        for key, fn, kw in M.CALLS:
            want = str(gold["%s.%s.%s" % (name, "i32" if dt == "i16" else dt, key)])
            assert M.call(mvs, fn, x, ae, pe, loc, mp, sp, kw) == want, (dt, key)


def test_defaults_and_import(mvs):
    from adapted_amd.detect.mvs import (mean_var_shift_polyA_check, mean_var_shift_polyA_detect,  # noqa: F401
                                        mean_var_shift_polyA_detect_at_loc)

    x, a, p = M.pa_read(1, 9000)
    x = x.astype(np.float32)
    assert mean_var_shift_polyA_detect(x) == R.detect(x, _cfg()[1]())
    assert mean_var_shift_polyA_detect_at_loc(x, a) == R.detect_at_loc(x, a, _cfg()[0]())
    r = mean_var_shift_polyA_detect(x[:100])
    assert r == 0 and type(r) is int


def _mixed(seed, n, dtype):
    """n reads of every shape the cases have, with positions near the true ones, past the end, and NaN holes"""
    rng = np.random.default_rng(seed)
    rows, meta = [], []
    for r in range(n):
        ln = int(rng.integers(2500, 9000))
        kw = dict(adapter=(int(rng.integers(800, 2000)), int(rng.integers(2100, 3600))), polya=(100, int(rng.integers(200, 1500))),
                  decoys=int(rng.integers(0, 3)), polya_sd=float(rng.choice([1.5, 2.0, 3.5])), rna_level=float(rng.choice([95.0, 100.0, 112.0])))
        if rng.random() < 0.15:
            kw["nan_at"] = tuple(int(v) for v in rng.integers(0, ln, int(rng.integers(1, 4))))
        if rng.random() < 0.1:
            kw["polya_level"] = 75.0
        x, a, p = M.pa_read(int(rng.integers(1 << 30)), ln, **kw)
        u = rng.random()
        ae = a + int(rng.integers(-40, 40)) if u < 0.7 else int(rng.integers(0, ln + 400))
        pe = p + int(rng.integers(-40, 40)) if rng.random() < 0.7 else ae + int(rng.integers(-10, 400))
        loc = a + int(rng.integers(-60, 60)) if rng.random() < 0.7 else int(rng.integers(0, ln + 300))
        rows.append(M.as_dtype(x, dtype))
        meta.append((max(ae, 0), max(pe, 0), max(loc, 0)))
    L = max(r.size for r in rows)
    X = np.zeros((n, L), dtype=rows[0].dtype)
    for i, r in enumerate(rows):
        X[i, :r.size] = r
    lens = np.array([r.size for r in rows])
    return rows, X, lens, np.array(meta, dtype=np.int64)


def _st(res):
    return 0 if not (isinstance(res, tuple) and res and res[0] == "raise") else (1 if res[1] == "IndexError" else 2)


def _bits(v):
    """the float64 bit patterns, every NaN as one (its sign and payload mean nothing to the reference either)"""
    a = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.int64)


@pytest.mark.parametrize("dtype", ["f32", "f64", "i16"])
def test_batches_match_restatement(mvs, dtype):
    mc, sc = _cfg()
    rows, X, lens, meta = _mixed({"f32": 11, "f64": 12, "i16": 13}[dtype], 2000, dtype)
    mp, sp = mc(), sc()
    sp_small = sc()
    sp_small.min_obs_adapter, sp_small.median_shift_window = 700, 800
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for lso in (False, True):
            for ws in (False, True):
                ok, vec, vals, st = mvs.mean_var_shift_polyA_check_batch(X, lens, meta[:, 0], meta[:, 1], mp, lso, ws, return_status=True)
                for r, x in enumerate(rows):
                    want = R.run(R.check, x, int(meta[r, 0]), int(meta[r, 1]), mp, True, lso, ws)
                    assert st[r] == _st(want), (r, lso, ws, want)
                    if st[r]:
                        continue
                    assert ok[r] == bool(want[0]) and vec[r].tolist() == want[1].tolist(), (r, lso, ws)
                    assert _bits(vals[r]).tolist() == _bits(want[2:]).tolist(), (r, lso, ws, vals[r], want)
        for lso in (False, True):
            ok, idx, vals, st = mvs.mean_var_shift_polyA_detect_at_loc_batch(X, lens, meta[:, 2], mp, lso)
            for r, x in enumerate(rows):
                want = R.run(R.detect_at_loc, x, int(meta[r, 2]), mp, True, lso)
                assert st[r] == _st(want), (r, lso, want)
                if st[r]:
                    assert idx[r] == 0
                    continue
                assert ok[r] == want[0] and idx[r] == want[1], (r, lso)
                assert _bits(vals[r]).tolist() == _bits(want[2:]).tolist(), (r, lso, vals[r], want)
        for p in (sp, sp_small):
            got = mvs.mean_var_shift_polyA_detect_batch(X, lens, p)
            want = [int(R.detect(x, p)) for x in rows]
            assert got.dtype == np.int64 and got.tolist() == want
            assert (got > 0).sum() > 100 and (got == 0).sum() > 100  # (both outcomes are well represented)


def test_dropin_equals_batch_row(mvs):
    mc, sc = _cfg()
    rows, X, lens, meta = _mixed(21, 64, "f32")
    ok, idx, vals, st = mvs.mean_var_shift_polyA_detect_at_loc_batch(X, lens, meta[:, 2], mc())
    det = mvs.mean_var_shift_polyA_detect_batch(X, lens, sc())
    cok, cvec, cvals, cst = mvs.mean_var_shift_polyA_check_batch(X, lens, meta[:, 0], meta[:, 1], mc(), return_status=True)
    for r, x in enumerate(rows):
        d = mvs.mean_var_shift_polyA_detect(x)
        assert int(d) == det[r]
        if st[r] == 0:
            one = mvs.mean_var_shift_polyA_detect_at_loc(x, int(meta[r, 2]), mc(), return_values=True)
            assert one[0] == ok[r] and one[1] == idx[r] and _bits(one[2:]).tolist() == _bits(vals[r]).tolist()
        if cst[r] == 0:
            one = mvs.mean_var_shift_polyA_check(x, int(meta[r, 0]), int(meta[r, 1]), mc(), return_values=True)
            assert one[0] == cok[r] and one[1].tolist() == cvec[r].tolist()
            if one[2:] != (0.0,) * 5:
                assert _bits(one[2:]).tolist() == _bits(cvals[r]).tolist()


def _long_batch(n, L, seed=5):
    """n reads of up to L float32 samples: 40 base reads, each row with a poly(A) stretch at its own depth (or none)"""
    rng = np.random.default_rng(seed)
    base = np.stack([M.pa_read(s, L, adapter=(3000, 3001), polya=(0, 1), adapter_level=75.0)[0].astype(np.float32) for s in range(40)])
    X = np.empty((n, L), dtype=np.float32)
    lens = rng.integers(L // 2, L + 1, n)
    for r in range(n):
        X[r] = base[r % 40]
        if r % 5:
            d = int(rng.integers(5000, lens[r] - 1000))
            X[r, d - 2000:d] = rng.normal(75.0, 6.0, 2000).astype(np.float32)  # (an adapter in front: the median shift holds)
            X[r, d:d + 700] = rng.normal(110.0, 2.0, 700).astype(np.float32)
            X[r, d + 700:min(L, d + 2700)] = rng.normal(101.0, 8.0, min(L, d + 2700) - d - 700).astype(np.float32)
    return X, lens


def test_detect_batch_200k_host_and_device(mvs):
    from adapted_amd.detect import _c_llr

    sc = _cfg()[1]
    n, L = 2000, 200000
    X, lens = _long_batch(n, L)
    host = mvs.mean_var_shift_polyA_detect_batch(X, lens, sc())
    eng = _c_llr._engine()
    d = eng.dev_alloc(X.nbytes)
    try:
        eng.h2d(d, X)
        dev = mvs.mean_var_shift_polyA_detect_batch(d, lens, sc(), n=n, L=L, dtype=np.float32)
    finally:
        eng.dev_free(d)
    assert dev.tolist() == host.tolist()
    assert (host > 0).sum() > n // 2 and (host == 0).sum() > n // 10
    pick = np.random.default_rng(1).choice(n, 48, replace=False)
    for r in pick.tolist():
        assert host[r] == int(R.detect(X[r, :lens[r]], sc())), r
