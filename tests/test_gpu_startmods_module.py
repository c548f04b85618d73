"""The start-peak and adapter-start drop-ins (adapted_amd/detect/start_peak.py, adapter_start.py -> adp_start_peak /
adp_adapter_start, adapted_amd/csrc/startmods_api.h) against the vectors of the REAL reference (tests/golden/
startmods_module.npz: values, Python types, exception texts, None cells, exactly) and, on batches in every dtype, against the CPU
restatement (tests/startmods_module_restated.py): adapter_start, status, cand and the 64 bits of difference[cand], no tolerance."""
import os
import types
import warnings

import numpy as np
import pytest

import startmods_module_cases as M
import startmods_module_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "startmods_module.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def A():
    from adapted_amd.detect import adapter_start

    return adapter_start


@pytest.fixture(scope="module")
def S():
    from adapted_amd.detect import start_peak

    return start_peak


def _cfg(**kw):
    from adapted_amd.config.sig_proc import MMAdapterStartConfig

    return MMAdapterStartConfig(**kw)


def _bits(v):
    """the float64 bit patterns, every NaN as one (its sign and payload mean nothing to the reference either)"""
    a = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.int64)


# ---- 1. both drop-ins against the golden, case by case
@pytest.mark.parametrize("dt", M.AS_DTYPES + ("i16",))
def test_adapter_start_dropin_matches_reference(gold, A, dt):
    for case in M.AS_CASES:
        x = M.as_dtype(M.as_input(case), dt)
        want = str(gold["as.%s.%s" % (case["name"], "i32" if dt == "i16" else dt)])
        assert M.as_call(A.moving_mean_adapter_start_detect, x, M.as_params(_cfg, case)) == want, case["name"]


@pytest.mark.parametrize("name", [c["name"] for c in M.SP_CASES])
def test_start_peak_dropin_matches_reference(gold, S, name):
    from adapted_amd.config.schema import RNAStartPeakConfig

    case = M.sp_by_name(name)
    sec = M.sp_section(RNAStartPeakConfig, case)
    X64, lens = M.sp_input(case, sec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dt in M.SP_DTYPES:
            got = M.sp_call(S.detect_rna_start_peak, M.sp_as_dtype(X64, dt), lens, types.SimpleNamespace(rna_start_peak=sec))
            assert M.frame_diff(got, M.sp_want(gold, name, dt), dtypes=M.same_pandas(gold)) == [], dt


# ---- 2. the batch forms against the restatement, bit for bit
def _want(rows, p):
    """the restatement per read: (adapter_start, status, cand, difference[cand])"""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for x in rows:
            try:
                r, _, cand, val = R.adapter_start_details(x, p)
                out.append((int(r), 0, cand, val))
            except ValueError:
                out.append((0, 2, -1, 0.0))
    return out


def _compare(A, rows, p, **kw):
    L = max(max(r.size for r in rows), 1)
    X = np.zeros((len(rows), L), dtype=rows[0].dtype)
    for i, r in enumerate(rows):
        X[i, :r.size] = r
    got = A.moving_mean_adapter_start_detect_batch(X, [r.size for r in rows], p, details=True, **kw)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int64 and got[3].dtype == np.float64
    want = _want(rows, p)
    for r, w in enumerate(want):
        g = (int(got[0][r]), int(got[1][r]), int(got[2][r]), int(_bits(got[3][r])))
        assert g == (w[0], w[1], w[2], int(_bits(w[3]))), (r, rows[r].size, g, w, float(got[3][r]))
    return want


def _mixed(seed, n, dt, top=8192):
    """n reads of up to `top` samples: both kinds of read, every length class, NaN and inf holes, reads too short"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        ln = int(rng.integers(2400, top + 1)) if r % 8 else int(rng.integers(0, 2700))
        sp = int(rng.integers(ln // 8, ln // 2 + 1)) if ln >= 8 else 0
        x = M.noisy_read(int(rng.integers(1 << 30)), ln, sp) if r % 2 else M.step_read(int(rng.integers(1 << 30)), ln, split=sp)
        if r % 7 == 3 and ln:
            x[int(rng.integers(0, ln))] = (np.nan, np.inf, -np.inf)[r % 3]
        if r % 11 == 5:
            x[:sp] -= 35.0  # (the shift passes, the current does not)
        rows.append(M.as_dtype(x, dt))
    return rows


@pytest.mark.parametrize("dt", ["f32", "f64", "i32"])
def test_mixed_batch_matches_restatement(A, dt):
    rows = _mixed({"f32": 31, "f64": 32, "i32": 33}[dt], 64, dt)
    want = _compare(A, rows, _cfg())
    assert sum(w[0] > 0 for w in want) > 10 and sum(w[1] == 2 for w in want) > 2 and sum(w[0] == 0 and w[1] == 0 for w in want) > 5
    _compare(A, rows, _cfg(window=300, min_obs_adapter=1000, min_shift=10.0))  # (a window longer than the staged history)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_boundary_sweep_matches_restatement(A, dt):
    """window 7, min_obs 5: one read for every size of `difference` from 0 to two staging chunks and two"""
    from adapted_amd import lib

    w, mo = 7, 5
    top = 2 * lib.ADAPTER_START_CHUNK + 2
    base = M.step_read(77, top + w + mo, split=400)
    noisy = M.noisy_read(78, top + w + mo, 400)
    rows = [M.as_dtype((base if ls % 2 else noisy)[:ls + w + mo], dt) for ls in range(top + 1)]
    want = _compare(A, rows, _cfg(window=w, min_obs_adapter=mo, min_shift=5.0))
    assert want[0][2] == -1 and sum(x[0] > 0 for x in want) > top // 4


# ---- 3. float32 is computed in float32
def test_float32_runs_in_float32(A):
    rng = np.random.default_rng(41)
    rows64 = [M.noisy_read(int(s), 6000, int(rng.integers(900, 2500))) for s in rng.integers(1 << 30, size=16)]
    rows32 = [x.astype(np.float32) for x in rows64]
    p = _cfg()
    w32, w64 = _want(rows32, p), _want([x.astype(np.float64) for x in rows32], p)
    differ = [r for r in range(16) if _bits(w32[r][3]) != _bits(w64[r][3])]
    assert len(differ) >= 8  # (the same samples, summed in the other type, give other bits)
    _compare(A, rows32, p)


# ---- 4. host input, device-pointer input and the single-read drop-in give the same row
def test_host_device_and_single_read_agree(A, S):
    from adapted_amd.config.schema import RNAStartPeakConfig
    from adapted_amd.detect._rows import _engine

    eng = _engine()
    for dt, npdt in (("f32", np.float32), ("f64", np.float64)):
        rows = _mixed(51, 24, dt, top=5000)
        L = max(r.size for r in rows)
        X = np.zeros((len(rows), L), dtype=npdt)
        lens = np.array([r.size for r in rows])
        for i, r in enumerate(rows):
            X[i, :r.size] = r
        host = A.moving_mean_adapter_start_detect_batch(X, lens, _cfg(), details=True)
        case = M.sp_by_name("ragged_ds3")
        sec = M.sp_section(RNAStartPeakConfig, case)
        P64, plens = M.sp_input(case, sec)
        P = np.ascontiguousarray(P64, dtype=npdt)
        sp_host = S.detect_rna_start_peak_batch(P, plens, sec)
        d, dp = eng.dev_alloc(X.nbytes), eng.dev_alloc(P.nbytes)
        try:
            eng.h2d(d, X)
            eng.h2d(dp, P)
            dev = A.moving_mean_adapter_start_detect_batch(d, lens, _cfg(), n=len(rows), L=L, dtype=npdt, details=True)
            sp_dev = S.detect_rna_start_peak_batch(dp, plens, sec, n=P.shape[0], m=P.shape[1], dtype=npdt)
        finally:
            eng.dev_free(d)
            eng.dev_free(dp)
        for h, g in zip(host, dev):
            assert _bits(h).tolist() == _bits(g).tolist() if h.dtype.kind == "f" else h.tolist() == g.tolist()
        assert sp_host.tobytes() == sp_dev.tobytes() and sp_host["valid"].any()
        for r, x in enumerate(rows):
            try:
                one = A.moving_mean_adapter_start_detect(x, _cfg())
                assert host[1][r] == 0 and int(one) == host[0][r] and (type(one) is int) == (host[0][r] == 0)
            except ValueError as e:
                assert host[1][r] == 2 and str(e) == "Moving window (=100) must between 1 and %d, inclusive" % max(x.size - 2500, 0)


# ---- 5. long reads
def test_eight_reads_of_200k_match_restatement(A):
    rng = np.random.default_rng(61)
    rows = [M.noisy_read(int(rng.integers(1 << 30)), 200000, int(rng.integers(20000, 90000))).astype(np.float32) for _ in range(8)]
    rows[3][150000] = np.nan
    want = _compare(A, rows, _cfg())
    assert sum(w[0] > 0 for w in want) >= 6


# ---- 6. the existing operator and the new module agree
@pytest.mark.parametrize("name", ["rna004_start_peak_blips", "rna004_start_peak_params", "rna004_start_peak_nan"])
def test_start_peak_batch_equals_the_detect_operator(S, name):
    from util import load_case

    from adapted_amd.detect.combined import combined_detect_start_peak

    _, spc, sig, lens, _ = load_case(name)
    res = combined_detect_start_peak(sig, lens, spc)
    got = S.detect_rna_start_peak_batch(sig, lens, spc.rna_start_peak)
    assert got["valid"].sum() > len(res) // 2
    for g, w in zip(got, res):
        assert bool(g["valid"]) == (w.start_peak_idx is not None)
        if not g["valid"]:
            continue
        assert (int(g["start_peak_idx"]), int(g["next_greater_idx"])) == (w.start_peak_idx, w.start_peak_next_max_idx)
        assert np.float32(g["start_peak_pa"]).tobytes() == np.float32(w.start_peak_pa).tobytes()
        assert np.float32(g["next_greater_pa"]).tobytes() == np.float32(w.start_peak_next_max_pa).tobytes()
        op = w.start_peak_open_pore_idx
        assert int(g["open_pore_idx"]) == (-1 if op is None or op != op else int(op))
        assert S.FLAGGED_TYPES[int(g["flagged_type"])] == w.start_peak_open_pore_type


# ---- 7. the shared workspace
def test_one_engine_alternating_calls_equals_fresh_engines(A, S):
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.config.schema import MVSPolyAConfig
    from adapted_amd.detect import mvs
    from adapted_amd.detect.adapter_start import _args as as_args
    from adapted_amd.detect.start_peak import _args as sp_args

    spc = get_chemistry_specific_config("RNA004")
    rows = _mixed(71, 16, "f32", top=6000)
    L = max(r.size for r in rows)
    X = np.zeros((len(rows), L), dtype=np.float32)
    lens = np.array([r.size for r in rows], dtype=np.int32)
    for i, r in enumerate(rows):
        X[i, :r.size] = r
    ae, pe = np.minimum(lens // 3, 2000).astype(np.int64), np.minimum(lens // 3 + 400, lens).astype(np.int64)
    seg_rows = np.arange(len(rows))
    margs = mvs._args(MVSPolyAConfig(), None, True, True)

    def calls(eng):
        return [lambda: eng.adapter_start(X, lens, as_args(_cfg())),
                lambda: eng.mvs_check(X, lens, ae, pe, margs),
                lambda: eng.start_peak(X, lens, sp_args(spc.rna_start_peak)),
                lambda: eng.seg_stats(X, lens, seg_rows, ae, pe),
                lambda: eng.adapter_start(X[:, :3000].copy(), np.minimum(lens, 3000), as_args(_cfg(window=7, min_obs_adapter=5)))]

    def flat(res):
        return [np.asarray(a).tobytes() for a in res]

    fresh = []
    for k in range(5):
        eng = lib.Engine(spc, 1, spc.sig_preload_size)
        fresh.append(flat(calls(eng)[k]()))
        eng.close()
    eng = lib.Engine(spc, 1, spc.sig_preload_size)
    try:
        for rep in range(2):
            for k in (0, 1, 2, 3, 4, 2, 0):
                assert flat(calls(eng)[k]()) == fresh[k], (rep, k)
    finally:
        eng.close()
