"""The best-split segmenters of the `_c_llr` drop-in (adapted_amd/detect/_c_llr.py -> adp_c_llr_detect / adp_c_llr_best_split,
adapted_amd/csrc/llr_detect_api.h) against the vectors of the REAL reference (tests/golden/c_llr_detect.npz) and, on many
synthetic reads, against the CPU restatement (tests/c_llr_detect_restated.py): split indices equal, medians equal, rows equal.

The device logarithm is correctly rounded and glibc's is not, so a gain may differ in the last bit: a split index may differ
only where the restatement's gains at the two indices are within 1e-12 relative (an exact tie in all but the last bits).  Such
reads are counted and reported; the expectation is none."""
import os

import numpy as np
import pytest

import c_llr_detect_restated as R
from c_llr_detect_cases import CASES, SPLITS, by_name, signal_of

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c_llr_detect.npz")
MO, BT, MPO = 300, 20, 50


def _same_trace(got, want):
    # (the tolerance of test_gpu_trace_api.py)
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    if fin.any():
        scale = max(1.0, float(np.max(np.abs(want[fin]))))
        assert float(np.max(np.abs(got[fin] - want[fin]))) <= 1e-9 * scale
    inf = np.isinf(want)
    assert np.array_equal(np.sign(got[inf]), np.sign(want[inf]))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_scalar_dropins_equal_the_reference(gold, case):
    from adapted_amd.detect import _c_llr

    x = signal_of(case)
    nm, mo, bt, mpo = case["name"], case["mo"], case["bt"], case["mpo"]
    a = _c_llr.c_llr_detect_adapter(x, mo, bt)
    p = _c_llr.c_llr_detect_adapter_polya(x, mo, bt, mpo)
    assert type(a) is tuple and all(type(v) is int for v in a)
    assert type(p) is tuple and all(type(v) is int for v in p)
    assert a == tuple(gold[nm + ".adapter"].tolist())
    assert p == tuple(gold[nm + ".polya"].tolist())
    # float32 input: the same as x.astype(float64) (exact when x holds float32 values, as every case does but the raw ones)
    if np.array_equal(x.astype(np.float32).astype(np.float64), x, equal_nan=True):
        assert _c_llr.c_llr_detect_adapter(x.astype(np.float32), mo, bt) == a
    if case["trace"]:
        for key, got in (("trace", _c_llr.c_llr_detect_adapter_trace(x, mo, bt)),
                         ("ptrace", _c_llr.c_llr_detect_adapter_polya_trace(x, mo, bt, mpo)),
                         ("btrace", _c_llr.c_llr_boundary_traces(x, mo, bt))):
            assert len(got) == (4 if key == "ptrace" else 3)
            for k, g in enumerate(got):
                _same_trace(g, gold["%s.trace%d" % (nm, k)])


@pytest.mark.parametrize("k", range(len(SPLITS)))
def test_best_split_equals_the_reference(gold, k):
    from adapted_amd.detect import _c_llr

    nm, s, e, oh, ot = SPLITS[k]
    x = signal_of(by_name(nm))
    c, c2 = np.cumsum(x), np.cumsum(np.multiply(x, x))
    xs, g = _c_llr._best_split(s, e, c, c2, oh, ot)
    want = gold["split%d" % k]
    assert type(xs) is int and type(g) is float
    assert xs == int(want[0])
    assert g == pytest.approx(float(want[1]), rel=1e-12) or g == want[1]


def _mixed_reads(n, seed=11):
    """n synthetic reads (adapted_amd/synth.py), lengths from below min_obs to 200 000, with NaN holes, constant runs, constant
    reads and 0.5 pA-quantised rows, as two padded float64 batches (NaN padding): the short reads [n - n // 50, 30 000] and
    the long ones [n // 50, 200 000] -> [(raw, lens), (raw, lens)]"""
    from adapted_amd.synth import synth_read

    rng = np.random.default_rng(seed)
    n_long = n // 50
    groups = []
    for g, (lo, hi, k) in enumerate(((2, 30_000, n - n_long), (150_000, 200_001, n_long))):
        lens = rng.integers(lo, hi, k)
        if g == 0:
            lens[:4] = (1, 2, 3, 250)
        else:
            lens[0] = 200_000
        raw = np.full((k, int(lens.max())), np.nan)
        for r in range(k):
            m = int(lens[r])
            x = synth_read(seed + g, r, m, m).astype(np.float64)
            kind = r % 5
            if kind == 1 and m > 20:    # a NaN hole: the last sample (which no split sees) or inside
                x[m - 1 if r % 2 else int(rng.integers(0, m))] = np.nan
            elif kind == 2 and m > 20:  # a constant run
                a = int(rng.integers(0, m // 2))
                x[a: a + m // 3] = x[a]
            elif kind == 3:             # 0.5 pA-quantised
                x = np.round(x * 2.0) / 2.0
            elif kind == 4 and r % 20 == 4:  # a constant read
                x[:] = 90.0
            raw[r, :m] = x
        groups.append((raw, lens))
    return groups


def _near(g, i, j):
    a, b = g[i], g[j]
    return np.isfinite(a) and np.isfinite(b) and abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def _compare(oracle_mod, raw, lens, rows, splits, stats, polya):
    """rows / splits / stats of the device against the restatement -> (number of reads, margin-explained index differences)"""
    margin = 0
    for r in range(raw.shape[0]):
        x = raw[r, : lens[r]]
        d = R.detect(oracle_mod, x, MO, BT, MPO if polya else None)
        ok = True
        for k in range(4):
            if splits[r, k] != d["splits"][k]:
                g = d["gain_arrays"][k]
                assert g is not None and splits[r, k] >= 0 and d["splits"][k] >= 0 and _near(g, splits[r, k], d["splits"][k]), \
                    (r, k, splits[r], d["splits"])
                margin += 1
                ok = False
                break
        if not ok:
            continue
        if d["branch"] != "no_first_split":
            assert np.array_equal(stats[r, 4:], np.array(d["medians"]), equal_nan=True), (r, stats[r, 4:], d["medians"])
            gh, gt = d["gains"][1], d["gains"][2]
            if (stats[r, 2] > stats[r, 1]) != (gt > gh):  # the decision's gain comparison on a near tie
                assert abs(gt - gh) <= 1e-12 * max(abs(gt), abs(gh)), r
                margin += 1
                continue
        res = d["result"]
        assert int(rows[r, 3]) == len(res), (r, rows[r], res)
        assert tuple(int(v) for v in rows[r, : len(res)]) == res, (r, rows[r], res)
    return raw.shape[0], margin


@pytest.fixture(scope="module")
def mixed():
    return _mixed_reads(1000)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_batch_vs_restatement_mixed(oracle_mod, mixed, dtype):
    from adapted_amd.detect import _c_llr

    total = 0
    for raw, lens in mixed:
        x = raw.astype(np.float32) if dtype == "float32" else raw
        ref = x.astype(np.float64)  # (what the float32 rows mean: exact widening)
        for polya in (False, True):
            f = _c_llr.c_llr_detect_adapter_polya_batch if polya else _c_llr.c_llr_detect_adapter_batch
            args = (MO, BT, MPO) if polya else (MO, BT)
            rows, splits, stats = f(x, lens, *args, details=True)
            n, margin = _compare(oracle_mod, ref, lens, rows, splits, stats, polya)
            print("%s polya=%s L=%d: %d reads, %d index differences explained by a 1e-12 margin" % (dtype, polya, x.shape[1], n, margin))
            total += margin
    assert total <= 4  # (expected 0; reported above)


def test_batch_equals_per_read_calls_and_ignores_padding(mixed):
    from adapted_amd.detect import _c_llr

    raw, lens = mixed[0]
    idx = np.r_[0:40, 500:520]
    sub, sl = raw[idx], lens[idx]
    L = int(sl.max())
    sub = sub[:, :L]
    a = _c_llr.c_llr_detect_adapter_polya_batch(sub, sl, MO, BT, MPO)
    garbage = sub.copy()
    rng = np.random.default_rng(3)
    for r in range(garbage.shape[0]):
        garbage[r, sl[r]:] = rng.normal(0, 1e6, L - sl[r])
    b = _c_llr.c_llr_detect_adapter_polya_batch(garbage, sl, MO, BT, MPO)
    wide = np.concatenate([garbage, np.full((garbage.shape[0], 777), np.inf)], axis=1)
    c = _c_llr.c_llr_detect_adapter_polya_batch(wide, sl, MO, BT, MPO)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    for r in range(0, len(idx), 3):
        one = _c_llr.c_llr_detect_adapter_polya(sub[r, : sl[r]], MO, BT, MPO)
        assert one == tuple(int(v) for v in a[r, : a[r, 3]])
        assert _c_llr.c_llr_detect_adapter(sub[r, : sl[r]], MO, BT) == tuple(
            int(v) for v in _c_llr.c_llr_detect_adapter_batch(sub[r: r + 1, : sl[r]], sl[r: r + 1], MO, BT)[0, :2])
    # best_split_batch against per-row _best_split
    z = np.nan_to_num(sub[:8], nan=0.0)
    cs, cs2 = np.cumsum(z, axis=1), np.cumsum(z * z, axis=1)
    st, en = np.zeros(8, np.int64), sl[:8] - 1
    xs, gs = _c_llr.best_split_batch(cs, cs2, sl[:8], st, en, np.full(8, 25), np.full(8, 25))
    for r in range(8):
        assert (int(xs[r]), float(gs[r])) == _c_llr._best_split(0, int(en[r]), cs[r, : sl[r]], cs2[r, : sl[r]], 25, 25)


def test_large_batch_spot_check(oracle_mod):
    """2000 x 200 000 float32 reads in one call; 64 rows checked against the restatement"""
    from adapted_amd.detect import _c_llr
    from adapted_amd.synth import synth_read

    n, L = 2000, 200_000
    base = np.stack([synth_read(21, k, L, L) for k in range(64)])
    x = np.empty((n, L), dtype=np.float32)
    for r in range(n):
        x[r] = np.roll(base[r % 64], (r // 64) * 4099)
    lens = np.full(n, L, dtype=np.int64)
    lens[1::7] = L - 12_345
    rows, splits, stats = _c_llr.c_llr_detect_adapter_polya_batch(x, lens, MO, BT, MPO, details=True)
    pick = np.random.default_rng(1).choice(n, 64, replace=False)
    _, margin = _compare(oracle_mod, x[pick].astype(np.float64), lens[pick], rows[pick], splits[pick], stats[pick], True)
    print("2000 x 200k: 64 rows checked, %d margin-explained differences" % margin)
    assert margin <= 1
