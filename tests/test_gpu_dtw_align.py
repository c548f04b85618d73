"""adp_dtw_align and adp_dba_step (include/adapted_hip_templates.h; kernels: adapted_amd/csrc/dtw_align_api.h) against their numpy
oracle (tests/dtw_align_oracle.py): every output bit for bit (all NaNs count as one), no tolerance -- every rounding and every
tie of both calls is specified."""
import numpy as np
import pytest

import dtw_align_oracle as do

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def _sequence(rng, kind, n):
    return rng.standard_normal(n) if kind == "gauss" else rng.integers(-1, 2, n).astype(np.float64)


def _pad(xs, E, fill=np.nan):
    out = np.full((len(xs), E), fill)
    for r, x in enumerate(xs):
        out[r, :len(x)] = x
    return out, np.asarray([len(x) for x in xs], dtype=np.int32)


def _compare(got, want):
    assert got["dist"].dtype == got["sum"].dtype == np.float64 and got["status"].dtype == got["lo"].dtype == got["hi"].dtype == np.int32
    assert got["status"].tolist() == want["status"].tolist()
    bad = [p for p in range(len(want["dist"])) if not (do.same(got["dist"][p], want["dist"][p]) and do.same(got["lo"][p], want["lo"][p])
                                                      and do.same(got["hi"][p], want["hi"][p]) and do.same(got["sum"][p], want["sum"][p]))]
    assert not bad, (bad[:8], got["lo"][bad[0]], want["lo"][bad[0]], got["hi"][bad[0]], want["hi"][bad[0]])


def _check(eng, q, qc, which, t, tc, band):
    want = do.align(q, qc, which, t, tc, band)
    got = eng.dtw_align(q, qc, which, np.where(np.isnan(t), 0.0, t), tc, band)
    _compare(got, want)
    return got, want


def _small_shapes(seed=21):
    """every (n, m) in 1 .. 9, Gaussian and {-1, 0, 1} sequences: 18 templates, 9 queries each"""
    rng = np.random.default_rng(seed)
    ts, qs, which = [], [], []
    for kind in ("gauss", "ternary"):
        for m in range(1, 10):
            ts.append(_sequence(rng, kind, m))
            for n in range(1, 10):
                qs.append(_sequence(rng, kind, n))
                which.append(len(ts) - 1)
    q, qc = _pad(qs, 9)
    t, tc = _pad(ts, 9)
    return q, qc, np.asarray(which, dtype=np.int32), t, tc


@pytest.mark.parametrize("band", [0, 1, 3])
def test_every_small_shape_and_the_ties(eng, band):
    q, qc, which, t, tc = _small_shapes()
    got, want = _check(eng, q, qc, which, t, tc, band)
    assert (want["status"] == 0).all()
    # the distance is adp_dtw_assign's for the same pair
    dist = eng.dtw_assign(q, qc, np.where(np.isnan(t), 0.0, t), tc, band)[0]
    assert do.same(got["dist"], dist[np.arange(len(which)), which].copy())


@pytest.mark.parametrize("Et", [64, 65, 128, 129, 256, 257, 512])
def test_register_tile_seams(eng, Et):
    """the widths around C = 1, 2, 4, 8 columns per lane; Eq = 512 puts the direction codes of the wide ones into global scratch"""
    rng = np.random.default_rng(Et)
    m = Et
    ts = [_sequence(rng, "gauss", m), _sequence(rng, "ternary", m), _sequence(rng, "gauss", m - 1), _sequence(rng, "ternary", max(m - 63, 1))]
    qs, which = [], []
    for n in (1, m - 1, m, 512):
        for k, kind in ((0, "gauss"), (1, "ternary")):
            qs.append(_sequence(rng, kind, n))
            which.append(k)
    qs += [_sequence(rng, "gauss", 511), _sequence(rng, "ternary", 300)]
    which += [2, 3]
    q, qc = _pad(qs, 512)
    t, tc = _pad(ts, Et)
    for band in (0, 5):
        _check(eng, q, qc, np.asarray(which, dtype=np.int32), t, tc, band)
    dist = eng.dtw_assign(q, qc, np.where(np.isnan(t), 0.0, t), tc, 5)[0]
    assert do.same(eng.dtw_align(q, qc, which, np.where(np.isnan(t), 0.0, t), tc, 5, want_path=False)["dist"], dist[np.arange(len(which)), which].copy())


def _mixed(seed=3, Eq=12, Et=10):
    """usable queries among refused, overflowing and skipped ones"""
    rng = np.random.default_rng(seed)
    ts = [_sequence(rng, "gauss", 10), _sequence(rng, "ternary", 4), np.asarray([0.5, 1.0])]
    t, tc = _pad(ts, Et)
    qs = [_sequence(rng, "gauss", n) for n in (12, 5, 1, 7, 7, 7, 7, 3, 2, 9)]
    q, qc = _pad(qs, Eq)
    which = np.asarray([0, 1, 0, 1, 0, 1, 0, 2, -1, 2], dtype=np.int32)
    qc[3] = 0  # refused: count 0
    qc[4] = Eq + 1  # refused: count above Eq
    q[5, 2] = np.nan  # refused: NaN inside the count
    q[6, 6] = np.inf  # refused: inf inside the count
    q[1, 8] = np.nan  # beyond the count: fine
    q[7, :3] = [1e200, 2.0, 3.0]  # overflow: status 2
    return q, qc, which, t, tc


def test_refused_overflowing_and_skipped_queries(eng):
    q, qc, which, t, tc = _mixed()
    got, want = _check(eng, q, qc, which, t, tc, 0)
    assert want["status"].tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 3, 0] and got["dist"][7] == np.inf
    _check(eng, q, qc, which, t, tc, 2)
    # the path outputs may be left out
    r = eng.dtw_align(q, qc, which, np.where(np.isnan(t), 0.0, t), tc, 0, want_path=False)
    assert r["lo"] is None and do.same(r["dist"], want["dist"]) and r["status"].tolist() == want["status"].tolist()


def test_device_inputs_give_the_same_bytes(eng):
    q, qc, which, t, tc = _mixed()
    t0 = np.where(np.isnan(t), 0.0, t)
    host = eng.dtw_align(q, qc, which, t0, tc, 2)
    dq, dqc = eng.dev_alloc(q.nbytes), eng.dev_alloc(qc.nbytes)
    try:
        eng.h2d(dq, q)
        eng.h2d(dqc, qc)
        dev = eng.dtw_align(dq, dqc, which, t0, tc, 2, nq=q.shape[0], Eq=q.shape[1])
        step_dev = eng.dba_step(dq, dqc, which, t0, tc, 2, nq=q.shape[0], Eq=q.shape[1], want_dist=True)
    finally:
        eng.dev_free(dq)
        eng.dev_free(dqc)
    for key in host:
        assert do.same(host[key], dev[key]), key
    for a, b in zip(eng.dba_step(q, qc, which, t0, tc, 2, want_dist=True), step_dev):
        assert do.same(a, b)
    assert do.same(step_dev[3], host["dist"])


def _batch_case(kind, seed=9):
    """queries over several batches of a 1 MiB budget: many short ones (1 KiB each, the codes in LDS), or few wide ones (72 KiB each
    with the codes in global scratch)"""
    rng = np.random.default_rng(seed)
    nq, Eq, Et = (2100, 8, 64) if kind == "lds" else (40, 512, 512)
    ts = [_sequence(rng, "ternary" if k % 2 else "gauss", int(rng.integers(1, 9))) for k in range(5)]
    if kind == "global":
        ts[0] = _sequence(rng, "gauss", 500)  # (the call's longest template sizes the rows of codes)
    qs = [_sequence(rng, "ternary" if p % 3 else "gauss", int(rng.integers(1, 9))) for p in range(nq)]
    which = rng.integers(-1, 5, nq).astype(np.int32)
    if kind == "global":
        which[which == 0] = 1
        which[[0, 17, 39]] = 0
        qs[17] = _sequence(rng, "gauss", 200)
    q, qc = _pad(qs, Eq)
    t, tc = _pad(ts, Et)
    qc[5] = 0
    return q, qc, which, t, tc


@pytest.mark.parametrize("kind", ["lds", "global"])
def test_the_scratch_budget_changes_no_bit(eng, kind, monkeypatch):
    q, qc, which, t, tc = _batch_case(kind)
    t0 = np.where(np.isnan(t), 0.0, t)
    whole = eng.dtw_align(q, qc, which, t0, tc, 0)
    step = eng.dba_step(q, qc, which, t0, tc, 0, want_dist=True)
    _compare(whole, do.align(q, qc, which, t, tc, 0))
    monkeypatch.setenv("ADP_DTW_SCRATCH_MIB", "1")
    split = eng.dtw_align(q, qc, which, t0, tc, 0)
    step_split = eng.dba_step(q, qc, which, t0, tc, 0, want_dist=True)
    monkeypatch.delenv("ADP_DTW_SCRATCH_MIB")
    for key in whole:
        assert do.same(whole[key], split[key]), key
    want = do.dba_step(q, qc, which, t, tc, 0)
    for a, b, w in zip(step, step_split, want):
        assert do.same(a, b) and do.same(a, w)
    monkeypatch.setenv("ADP_DTW_SCRATCH_MIB", "0")
    from adapted_amd import lib

    with pytest.raises(lib.HipLibraryError, match="ADP_DTW_SCRATCH_MIB"):
        eng.dtw_align(q, qc, which, t0, tc, 0)


def test_dba_step_three_templates_of_forty_members_and_an_empty_one(eng):
    rng = np.random.default_rng(77)
    bases = [_sequence(rng, "gauss", n) for n in (14, 20, 9)]
    qs, which = [], []
    for k, base in zip((0, 1, 3), bases):  # (template 2 has no member)
        for _ in range(40):
            x = np.repeat(base, rng.integers(1, 3, base.size))
            qs.append(x + 0.1 * rng.standard_normal(x.size))
            which.append(k)
    order = rng.permutation(len(qs))
    qs, which = [qs[i] for i in order], np.asarray(which, dtype=np.int32)[order]
    q, qc = _pad(qs, 40)
    t, tc = _pad([bases[0], bases[1], _sequence(rng, "gauss", 6), bases[2]], 24)
    q[7, 1] = np.inf  # a member that is refused
    which[11] = -1  # and one that is skipped
    for band in (0, 4):
        want = do.dba_step(q, qc, which, t, tc, band)
        got = eng.dba_step(q, qc, which, np.where(np.isnan(t), 0.0, t), tc, band, want_dist=True)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and do.same(g, w)
        assert want[1][2] == 0 and want[1].sum() == 118 and do.same(got[0][2], t[2]) and got[2][2] == 0.0
    assert eng.dba_step(q, qc, which, np.where(np.isnan(t), 0.0, t), tc, 0)[3] is None
    # the module function does the same
    from adapted_amd import barcode_templates as bt

    for g, w in zip(bt.dba_step(q, qc, which, np.where(np.isnan(t), 0.0, t), tc, 4), want[:3]):
        assert do.same(g, w)


def test_invalid_arguments_leave_the_handle_usable(eng):
    from adapted_amd import lib

    q, qc, which, t, tc = _mixed()
    t0 = np.where(np.isnan(t), 0.0, t)
    before = eng.dtw_align(q, qc, which, t0, tc, 0)
    wrong = which.copy()
    wrong[2] = 3
    low = which.copy()
    low[2] = -2
    tbad = t0.copy()
    tbad[1, 1] = np.nan
    for call in (lambda: eng.dtw_align(q, qc, wrong, t0, tc, 0), lambda: eng.dba_step(q, qc, low, t0, tc, 0),
                 lambda: eng.dtw_align(q, qc, which, t0, tc, -1), lambda: eng.dba_step(q, qc, which, tbad, tc, 0),
                 lambda: eng.dtw_align(q, qc, which, t0, tc * 0, 0), lambda: eng.dtw_align(q, qc, which, t0, tc + 20, 0)):
        with pytest.raises(lib.HipLibraryError):
            call()
        after = eng.dtw_align(q, qc, which, t0, tc, 0)
        for key in before:
            assert do.same(before[key], after[key]), key
