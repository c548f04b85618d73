"""The signal statistics drop-ins (adapted_amd/partition/signal_partitions.py, adapted_amd/detect/normalize.py, downscale.py,
real_range.py, anomalies.py -> adp_seg_stats, adp_med_mad, adp_normalize, adp_pool_mean, adp_real_range, adp_open_pores;
adapted_amd/csrc/sigstats_api.h) against the vectors of the REAL reference (tests/golden/sigstats_module.npz: values, Python types and None
results, exactly) and, on many synthetic reads in both dtypes, against the CPU restatement (tests/sigstats_module_restated.py):
lengths and float bit patterns identical, no tolerance (all NaNs count as one)."""
import importlib
import os
import types
import warnings

import numpy as np
import pytest

import sigstats_module_cases as M
import sigstats_module_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sigstats_module.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def sp():
    from adapted_amd.partition import signal_partitions

    return signal_partitions


@pytest.fixture(scope="module")
def mods():
    return {key: importlib.import_module("adapted_amd.detect." + key) for key in M.DETECT_NAMES}


def _bits(a):
    """float bit patterns with every NaN made the same one"""
    a = np.array(a, dtype=np.float64)
    a[a != a] = np.nan
    return a.view(np.uint64).tolist()


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in M.CASES])
def test_dropins_match_reference(gold, sp, name):
    from adapted_amd.container_types import Boundaries

    case = M.by_name(name)
    x64, names = M.inputs(case)
    for dt in M.DTYPES + ("i16",):
        x = M.as_dtype(x64, dt)
        for i, c in enumerate(case["calls"]):
            want = str(gold["%s.%s.%s" % (name, "i32" if dt == "i16" else dt, M.call_key(i, c))])
            assert M.call(sp, Boundaries, x, names, c) == want, (dt, i, c)


@pytest.mark.parametrize("key", ["%s.%s" % (c["module"], c["name"]) for c in M.DETECT_CASES])
def test_detect_dropins_match_reference(gold, mods, key):
    from adapted_amd.config.schema import RealRangeConfig

    d = types.SimpleNamespace(**{nm: getattr(mods[k], nm) for k, names in M.DETECT_NAMES.items() for nm in names})
    case = M.detect_case(*key.split("."))
    x64 = M.detect_input(case)
    for dt in case["dtypes"] + (("i16",) if "i32" in case["dtypes"] else ()):
        x = M.as_dtype(x64, dt)
        for i, c in enumerate(case["calls"]):
            want = str(gold[M.detect_key(case, "i32" if dt == "i16" else dt, i, c)])
            assert M.detect_call(d, RealRangeConfig, x, c) == want, (dt, i, c)


# ---- 2. mixed batches ----------------------------------------------------------------------------------------------------------
N_MIX = 2000


@pytest.fixture(scope="module")
def mix():
    """the 2000 mixed reads (float64 rows padded with 7.0) with their boundaries"""
    reads = [M.mixed_read(r) for r in range(N_MIX)]
    lens = np.array([x.size for x, _, _ in reads])
    X = np.full((N_MIX, int(lens.max())), 7.0)
    for r, (x, _, _) in enumerate(reads):
        X[r, :x.size] = x
    ae = np.array([a for _, a, _ in reads])
    pe = np.array([p for _, _, p in reads])
    return X, lens, ae, pe


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batches_match_restatement(sp, mix, dtype):
    X64, lens, ae, pe = mix
    X = X64.astype(dtype)
    n = N_MIX
    start, length, stats = sp.calc_partitions_from_vals_batch(X, lens, np.zeros(n, dtype=np.int64), ae, pe)
    rows = np.repeat(np.arange(n), 3)
    st = np.stack([np.zeros(n, dtype=np.int64), ae, pe], axis=1)
    en = np.stack([ae, pe, lens], axis=1)
    want_len, want = R.seg_stats(X, lens, rows, st.reshape(-1), en.reshape(-1))
    assert start.tolist() == st.tolist()
    assert length.reshape(-1).tolist() == want_len.tolist()
    assert _bits(stats.reshape(-1, 4)) == _bits(want)
    # the mix: the comparison does not pass on one outcome only
    live = length >= 0
    nan_reads = int((np.isnan(stats[:, :, 0]) & live).any(axis=1).sum())
    none_reads = int((~live).any(axis=1).sum())
    mad0 = int(((stats[:, 0, 3] == 0) & live[:, 0]).sum())
    print("reads with a NaN partition %d, with a None-length partition %d, with an adapter MAD of 0: %d" % (nan_reads, none_reads, mad0))
    assert nan_reads >= 100 and none_reads >= 150
    assert mad0 >= 40
    # the single-partition form, with None starts and ends among them
    s1 = np.where(np.arange(n) % 7 == 0, -1, ae)
    e1 = np.where(np.arange(n) % 11 == 0, -1, pe)
    length1, stats1 = sp.calc_partition_stats_batch(X, lens, s1, e1)
    want_len1, want1 = R.seg_stats(X, lens, np.arange(n), s1, e1)
    assert length1.tolist() == want_len1.tolist() and _bits(stats1) == _bits(want1)
    # truncated reads: a mask
    trunc = np.arange(n) % 3 == 0
    start_t, length_t, stats_t = sp.calc_partitions_from_vals_batch(X[:300], lens[:300], np.zeros(300, dtype=np.int64), ae[:300], pe[:300],
                                                                    trunc[:300])
    assert (start_t[trunc[:300], 2] == -1).all() and (length_t[trunc[:300], 2] == -1).all() and np.isnan(stats_t[trunc[:300], 2]).all()
    keep = ~trunc[:300]
    assert _bits(stats_t[keep]) == _bits(stats[:300][keep]) and _bits(stats_t[:, :2]) == _bits(stats[:300, :2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_detect_batches_match_restatement(mods, mix, dtype):
    """real_range_check, find_open_pores, med_mad and normalize_signal of signal[0:adapter_end], pooling of the rows"""
    from adapted_amd.config.schema import RealRangeConfig

    X64, lens, ae, pe = mix
    X = X64.astype(dtype)
    n = N_MIX
    zero = np.zeros(n, dtype=np.int64)
    seg_len = np.minimum(ae, lens)
    params = RealRangeConfig()
    # real range
    ok, vals, stage = mods["real_range"].real_range_check_batch(X, lens, zero, ae, params)
    want = [R.real_range_check(X[r, :seg_len[r]], params, True) for r in range(n)]
    assert ok.tolist() == [bool(w[0]) for w in want]
    assert stage.tolist() == [0 if w[1] is None else 1 if w[3] is None else 2 for w in want]
    assert _bits(vals) == _bits([[np.nan if v is None else float(v) for v in w[1:]] for w in want])
    print("real_range_check True %d False %d" % (ok.sum(), (~ok).sum()))
    assert ok.sum() >= 400 and (~ok).sum() >= 400
    # open pores
    pos, cnt, inr = mods["anomalies"].find_open_pores_batch(X, lens, zero, ae)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [R.find_open_pores(X[r, :seg_len[r]]).reshape(-1) for r in range(n)]
    assert cnt.tolist() == [w.size for w in want]
    assert pos.shape[1] == max(16, cnt.max())
    for r in range(n):
        assert pos[r, :cnt[r]].tolist() == want[r].tolist() and (pos[r, cnt[r]:] == -1).all(), r
    k = [int((cnt == 0).sum()), int((cnt == 1).sum()), int(((cnt > 1) & (cnt <= 16)).sum()), int((cnt > 16).sum())]
    print("open-pore lists of length 0 / 1 / 2-16 / > 16:", k)
    assert min(k) >= 200
    # a custom range with an upper bound, a cap that has to grow from 1
    pos2, cnt2, _ = mods["anomalies"].find_open_pores_batch(X[:200], lens[:200], zero[:200], ae[:200], (225.0, 235.0), 3, cap=1)
    for r in range(200):
        assert pos2[r, :cnt2[r]].tolist() == R.find_open_pores(X[r, :seg_len[r]], (225.0, 235.0), 3).reshape(-1).tolist(), r
    # median / MAD and the normalised rows, each read by itself
    mad0 = {}
    for with_nan in (False, True):
        mm = mods["normalize"].med_mad_batch(X, seg_len, with_nan)
        assert _bits(mm) == _bits([R.med_mad(X[r, :seg_len[r]], with_nan) for r in range(n)])
        out, mm2, status = mods["normalize"].normalize_signal_batch(X, seg_len, 5.0, with_nan)
        assert _bits(mm2) == _bits(mm) and out.dtype == dtype and out.shape == X.shape
        assert status.tolist() == [int(m == 0) for m in mm[:, 1]]
        for r in range(n):
            if status[r]:
                assert not out[r].any()
            else:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    w = R.normalize_signal(X[r, :seg_len[r]], 5.0, with_nan) if seg_len[r] else np.zeros(0, dtype)
                assert w.dtype == dtype and _bits(out[r, :seg_len[r]]) == _bits(w) and not out[r, seg_len[r]:].any(), r
        mad0[with_nan] = int(status.sum())
    print("rows with MAD == 0:", mad0)
    assert mad0[False] >= 40
    # pooling of the padded rows
    for p in (10, 3, 32, 7):
        got = mods["downscale"].efficient_average_pooling(X[:300], p)
        assert got.dtype == dtype and _bits(got) == _bits(R.efficient_average_pooling(X[:300], p)), p


# ---- 3. a batch row is the per-read call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16], ids=["f32", "f64", "i16"])
def test_dropin_equals_batch_row(sp, mix, dtype):
    X64, lens, ae, pe = mix
    n = 64
    X = np.round(np.nan_to_num(X64[:n])).astype(dtype) if dtype == np.int16 else X64[:n].astype(dtype)
    start, length, stats = sp.calc_partitions_from_vals_batch(X, lens[:n], np.zeros(n, dtype=np.int64), ae[:n], pe[:n])
    for r in range(n):
        P = sp.calc_partitions_from_vals(X[r, :lens[r]], 0, int(ae[r]), int(pe[r]))
        for k, part in enumerate((P.adapter, P.polya, P.rna)):
            assert part.start == start[r, k]
            if length[r, k] < 0:
                assert part == sp.Partition(int(start[r, k]), None, None, None, None, None)
            else:
                assert part.len == length[r, k] and type(part.len) is int and type(part.mean) is float
                assert _bits([part.mean, part.std, part.med, part.mad]) == _bits(stats[r, k])


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16], ids=["f32", "f64", "i16"])
def test_detect_dropins_equal_batch_rows(mods, mix, dtype):
    from adapted_amd.config.schema import RealRangeConfig

    X64, lens, ae, pe = mix
    n = 64
    X = np.round(np.nan_to_num(X64[:n])).astype(dtype) if dtype == np.int16 else X64[:n].astype(dtype)
    zero, seg_len, params = np.zeros(n, dtype=np.int64), np.minimum(ae, lens)[:n], RealRangeConfig()
    ok, vals, stage = mods["real_range"].real_range_check_batch(X, lens[:n], zero, ae[:n], params)
    pos, cnt, inr = mods["anomalies"].find_open_pores_batch(X, lens[:n], zero, ae[:n])
    mm = mods["normalize"].med_mad_batch(X, seg_len)
    out, _, status = mods["normalize"].normalize_signal_batch(X, seg_len)
    pooled = mods["downscale"].efficient_average_pooling(X, 10)
    for r in range(n):
        x = X[r, :seg_len[r]]
        one = mods["real_range"].real_range_check(x, params, True)
        assert one[0] == ok[r] and mods["real_range"].real_range_check(x, params) == ok[r]
        assert [v is None for v in one[1:]] == [stage[r] < 1, stage[r] < 1, stage[r] < 2]
        assert _bits([np.nan if v is None else float(v) for v in one[1:]]) == _bits(vals[r])
        got = mods["anomalies"].find_open_pores(x)
        assert got.reshape(-1).tolist() == pos[r, :cnt[r]].tolist()
        assert got.shape == R.find_open_pores(x).shape and got.dtype == np.int64
        assert _bits(mods["normalize"].med_mad(x)) == _bits(mm[r])
        if status[r] or not seg_len[r]:
            if seg_len[r]:
                with pytest.raises(ValueError, match="MAD normalization failed: scale is 0"):
                    mods["normalize"].normalize_signal(x)
        else:
            assert _bits(mods["normalize"].normalize_signal(x)) == _bits(out[r, :seg_len[r]])
        assert _bits(mods["downscale"].efficient_average_pooling(X[r:r + 1], 10)) == _bits(pooled[r:r + 1])


# ---- 4. size ------------------------------------------------------------------------------------------------------------------
def _long_batch(n, L, seed=5):
    """n float32 reads of up to L samples: adapter ~3000, poly(A) ~600, then RNA events; some quantised to 0.18 pA, some with
    NaN samples"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(L - 20000, L + 1, n)
    lens[::9] = L
    X = np.empty((n, L), dtype=np.float32)
    ae = rng.integers(2500, 3500, n)
    pe = ae + rng.integers(200, 1200, n)
    block = 50
    for r0 in range(0, n, block):
        m = min(block, n - r0)
        lv = np.repeat(rng.normal(100.0, 12.0, (m, L // 8 + 1)).astype(np.float32), 8, axis=1)[:, :L]
        X[r0:r0 + m] = lv + rng.normal(0.0, 3.0, (m, L)).astype(np.float32)
    for r in range(n):
        X[r, :ae[r]] = rng.normal(75.0, 6.0, ae[r]).astype(np.float32)
        X[r, ae[r]:pe[r]] = rng.normal(110.0, 2.0, pe[r] - ae[r]).astype(np.float32)
        if r % 10 == 3:
            X[r] = np.round(X[r] / np.float32(0.18)) * np.float32(0.18)
        if r % 25 == 7:
            X[r, rng.integers(0, lens[r], 2)] = np.nan
    return X, lens, ae, pe


def test_partitions_200k_host_and_device(sp):
    from adapted_amd.detect import _c_llr

    n, L = 2000, 200000
    X, lens, ae, pe = _long_batch(n, L)
    zero = np.zeros(n, dtype=np.int64)
    _, length, host = sp.calc_partitions_from_vals_batch(X, lens, zero, ae, pe)
    eng = _c_llr._engine()
    d = eng.dev_alloc(X.nbytes)
    try:
        eng.h2d(d, X)
        _, length_d, dev = sp.calc_partitions_from_vals_batch(d, lens, zero, ae, pe, n=n, L=L, dtype=np.float32)
    finally:
        eng.dev_free(d)
    assert length_d.tolist() == length.tolist() and _bits(dev) == _bits(host)
    assert (length[:, 2] > L - 25000).all() and np.isnan(host[:, 2, 0]).sum() >= n // 30
    pick = np.random.default_rng(1).choice(n, 48, replace=False)
    rows = np.repeat(pick, 3)
    st = np.stack([zero, ae, pe], axis=1)[pick].reshape(-1)
    en = np.stack([ae, pe, lens], axis=1)[pick].reshape(-1)
    want_len, want = R.seg_stats(X, lens, rows, st, en)
    assert length[pick].reshape(-1).tolist() == want_len.tolist()
    assert _bits(host[pick].reshape(-1, 4)) == _bits(want)


def _ragged_minibatch(rows, m, seed):
    """float32 [rows, m]: reads of events with NaN behind each read's end, every fifth row quantised to 0.18 pA"""
    rng = np.random.default_rng(seed)
    X = np.empty((rows, m), dtype=np.float32)
    for r0 in range(0, rows, 100):
        k = min(100, rows - r0)
        lv = np.repeat(rng.normal(95.0, 14.0, (k, m // 8 + 1)).astype(np.float32), 8, axis=1)[:, :m]
        X[r0:r0 + k] = lv + rng.normal(0.0, 3.0, (k, m)).astype(np.float32)
    X[::5] = np.round(X[::5] / np.float32(0.18)) * np.float32(0.18)
    ends = rng.integers(m // 4, m + 1, rows)
    ends[::7] = m
    X[np.arange(m)[None, :] >= ends[:, None]] = np.nan
    return X


@pytest.mark.parametrize("shape", [(1000, 17500), (96, 201500)], ids=["1000x17500", "96x201500"])
def test_whole_minibatch_normalisation(mods, shape):
    """normalize_signal(minibatch, with_nan=True) as the reference's callers use it: one population of up to 1.9e7 samples with
    NaN tails (the many-workgroup selection), against numpy"""
    X = _ragged_minibatch(shape[0], shape[1], 11)
    assert X.size > 4 * 262144 and np.isnan(X).sum() > X.size // 10
    got = mods["normalize"].normalize_signal(X, 5.0, True)
    med, mad = mods["normalize"].med_mad(X, True)
    assert (med, mad) == R.med_mad(X, True)
    want = R.normalize_signal(X, 5.0, True)
    assert got.dtype == np.float32 and got.shape == X.shape
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    # without with_nan a NaN anywhere makes both NaN, and every sample with them
    nm = mods["normalize"].med_mad(X)
    assert nm[0] != nm[0] and nm[1] != nm[1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_population_regimes_agree_across_the_threshold(dtype):
    """populations of ADP_SS_GRID_MIN - 1, + 0, + 1 samples (one wave below and at the threshold, many workgroups above it): the
    regime taken by itself, and each regime forced, give the same median and MAD, numpy's"""
    from adapted_amd import lib
    from adapted_amd.detect import _c_llr

    eng = _c_llr._engine()
    rng = np.random.default_rng(3)
    base = rng.normal(90.0, 12.0, max(lib.ADP_SS_GRID_MIN + 1, 4000 * 60))
    base[::3] = np.round(base[::3] / 0.18) * 0.18
    base[rng.integers(0, base.size, 50)] = np.nan
    base[rng.integers(0, lib.ADP_SS_GRID_MIN - 1, 5)] = np.nan
    for n in (lib.ADP_SS_GRID_MIN - 1, lib.ADP_SS_GRID_MIN, lib.ADP_SS_GRID_MIN + 1):
        x = base[:n].astype(dtype).reshape(1, -1)
        for with_nan in (True, False):
            want = R.med_mad(x, with_nan)
            got = [eng.med_mad(x, with_nan=with_nan, whole=True, regime=rg)[0] for rg in (None, "grid", "wave")]
            assert _bits(got[0]) == _bits(got[1]) == _bits(got[2]) == _bits(want), (n, with_nan)
        clean = np.nan_to_num(x, nan=77.0)
        got = [eng.med_mad(clean, whole=True, regime=rg)[0] for rg in (None, "grid", "wave")]
        assert _bits(got[0]) == _bits(got[1]) == _bits(got[2]) == _bits(R.med_mad(clean)), n
    # a [n, L] array is one population as it lies in memory, in either regime
    x2 = base[:4000 * 60].astype(dtype).reshape(60, 4000)
    assert _bits(eng.med_mad(x2, with_nan=True, whole=True, regime="grid")) == _bits(eng.med_mad(x2, with_nan=True, whole=True, regime="wave"))
    assert _bits(eng.med_mad(x2, with_nan=True, whole=True)[0]) == _bits(R.med_mad(x2, True))


def test_device_resident_rows(mods, mix):
    """every batch form on a device-resident batch equals the host form; pooling and normalisation also into device memory"""
    from adapted_amd.config.schema import RealRangeConfig
    from adapted_amd.detect import _c_llr

    X64, lens, ae, pe = mix
    n = 256
    X = np.ascontiguousarray(X64[:n].astype(np.float32))
    L = X.shape[1]
    zero, seg_len = np.zeros(n, dtype=np.int64), np.minimum(ae, lens)[:n]
    eng = _c_llr._engine()
    n_out = -(-L // 10)
    d, d_out, d_pool = eng.dev_alloc(X.nbytes), eng.dev_alloc(X.nbytes), eng.dev_alloc(n * n_out * 4)
    try:
        eng.h2d(d, X)
        kw = dict(n=n, L=L, dtype=np.float32)
        for a, b in zip(mods["real_range"].real_range_check_batch(X, lens[:n], zero, ae[:n], RealRangeConfig()),
                        mods["real_range"].real_range_check_batch(d, lens[:n], zero, ae[:n], RealRangeConfig(), **kw)):
            assert _bits(a) == _bits(b)
        for a, b in zip(mods["anomalies"].find_open_pores_batch(X, lens[:n], zero, ae[:n]),
                        mods["anomalies"].find_open_pores_batch(d, lens[:n], zero, ae[:n], **kw)):
            assert a.tolist() == b.tolist()
        assert _bits(mods["normalize"].med_mad_batch(X, seg_len, True)) == _bits(mods["normalize"].med_mad_batch(d, seg_len, True, **kw))
        host = mods["normalize"].normalize_signal_batch(X, seg_len)
        dev = mods["normalize"].normalize_signal_batch(d, seg_len, **kw)
        for a, b in zip(host, dev):
            assert _bits(a) == _bits(b)
        eng.h2d(d_out, np.zeros_like(X))
        none, mm, status = mods["normalize"].normalize_signal_batch(d, seg_len, out=d_out, **kw)
        back = np.empty_like(X)
        eng.d2h(back, d_out)
        assert none is None and _bits(back) == _bits(host[0]) and _bits(mm) == _bits(host[1]) and status.tolist() == host[2].tolist()
        pooled = mods["downscale"].efficient_average_pooling(X, 10)
        assert _bits(mods["downscale"].efficient_average_pooling_device(d, n, L, 10)) == _bits(pooled)
        assert mods["downscale"].efficient_average_pooling_device(d, n, L, 10, out=d_pool) is None
        back = np.empty((n, n_out), dtype=np.float32)
        eng.d2h(back, d_pool)
        assert _bits(back) == _bits(pooled)
    finally:
        for p in (d, d_out, d_pool):
            eng.dev_free(p)


# ---- 5. one engine, the families in turn -------------------------------------------------------------------------------------------
def test_alternating_with_other_modules_equals_fresh_engines(mix):
    """partition statistics alternating with adp_mvs_* / adp_c_llr_* calls on one engine, small and large batches in turn (the
    workspace is shared and grows): every result is the one a fresh engine gives for the same call"""
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.config.schema import StreamingConfig
    from adapted_amd.detect import mvs

    X64, lens, ae, pe = mix
    big, sm = X64[:400].astype(np.float32), X64[400:406].astype(np.float64)
    nb, ns = np.arange(400), np.arange(6)
    margs = mvs._args(None, StreamingConfig())
    from adapted_amd.config.schema import RealRangeConfig
    from adapted_amd.detect import real_range

    rargs = real_range._args(RealRangeConfig())
    raw = np.nan_to_num(X64[:32, :2400])
    steps = [
        lambda e: e.seg_stats(sm, lens[400:406], ns, ae[400:406], pe[400:406]),
        lambda e: e.mvs_detect(big, lens[:400], margs),
        lambda e: e.seg_stats(big, lens[:400], np.repeat(nb, 2), np.stack([0 * ae[:400], pe[:400]], 1).reshape(-1),
                              np.stack([ae[:400], lens[:400]], 1).reshape(-1)),
        lambda e: e.c_llr_detect(raw, np.full(32, 2400), 200, 20, 50, polya=True),
        lambda e: e.seg_stats(sm, lens[400:406], ns, 0 * ns, lens[400:406]),
        lambda e: e.mvs_detect(sm.astype(np.float32), lens[400:406], margs),
        lambda e: e.seg_stats(big, lens[:400], nb, ae[:400], pe[:400]),
        lambda e: e.normalize(sm, lens[400:406], 5.0, True),
        lambda e: e.open_pores(big, lens[:400], nb, 0 * ae[:400], ae[:400], 200.0, np.inf, 10.0, cap=2),
        lambda e: e.med_mad(big, with_nan=True, whole=True),
        lambda e: e.real_range(sm, lens[400:406], ns, 0 * ns, ae[400:406], rargs),
        lambda e: e.pool_mean(big, 10),
        lambda e: e.normalize(big[:50], with_nan=True, whole=True),
        lambda e: e.mvs_detect(big, lens[:400], margs),
        lambda e: e.med_mad(sm, lens[400:406]),
    ]
    spc = get_chemistry_specific_config("RNA004")

    def fresh():
        return lib.Engine(spc, 1, spc.sig_preload_size)

    eng = fresh()
    try:
        got = [step(eng) for step in steps]
    finally:
        eng.close()
    for i, step in enumerate(steps):
        one = fresh()
        try:
            want = step(one)
        finally:
            one.close()
        g = got[i] if isinstance(got[i], (tuple, list)) else (got[i],)
        w = want if isinstance(want, (tuple, list)) else (want,)
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert _bits(a) == _bits(b), i
