"""adp_event_levels and adp_dtw_assign (include/adapted_hip_fingerprint.h; kernels: adapted_amd/csrc/fingerprint_api.h) against
their numpy oracle (tests/fingerprint_oracle.py, on top of tests/events_oracle.py): every output bit for bit (all NaNs count as
one), no tolerance -- every rounding of both algorithms is specified.  Every generated signal is first checked, on the oracle's
side, to hold no two candidates closer than the minimum distance with equal scores (tests/test_gpu_events.py)."""
import ctypes

import numpy as np
import pytest

import events_oracle as eo
import fingerprint_oracle as fo

pytestmark = pytest.mark.gpu

W, D, THR, VF = 8, 8, 16.0, 1e-3


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def _args(w=W, D=D, thr=THR, vf=VF):
    from adapted_amd import lib

    a = lib.AdpEventArgs()
    a.window, a.min_distance, a.threshold, a.var_floor = w, D, thr, vf
    return a


def _pad(xs, dtype=None, L=None):
    """signals of several lengths -> (NaN-padded [n, L], lens)"""
    dtype = dtype or xs[0].dtype
    L = L or max(max(x.size for x in xs), 1)
    sig = np.full((len(xs), L), np.nan, dtype=dtype)
    for r, x in enumerate(xs):
        sig[r, :x.size] = x
    return sig, np.asarray([x.size for x in xs], dtype=np.int32)


def _want(sig, lens, rows, starts, ends, E, w=W, D=D, thr=THR, vf=VF, cache=None):
    cache = {} if cache is None else cache
    out = []
    for r, s, e in zip(rows, starts, ends):
        key = (int(r), int(s), int(e), E)
        if key not in cache:
            x = eo.clip(sig[r], int(lens[r]), int(s), int(e))
            assert not eo.has_close_ties(x, w, D, thr, vf), ("the input has tied candidates within the distance", key)
            cache[key] = fo.levels(x, E, w, D, thr, vf)
        out.append(cache[key])
    return out


def _compare(got, want, E):
    ns = len(want)
    assert got["info"].shape == (ns, 2) and got["lengths"].shape == got["levels"].shape == got["fingerprints"].shape == (ns, E)
    assert got["count"].dtype == got["status"].dtype == got["lengths"].dtype == np.int32
    for g, o in enumerate(want):
        assert got["info"][g].tolist() == [o["nk"], o["seg_status"]], (g, got["info"][g], o["nk"], o["seg_status"])
        assert fo.same(got["stats"][g], np.asarray([o["med_gap"], o["mad_gap"]])), g
        assert (int(got["count"][g]), int(got["status"][g])) == (o["count"], o["status"]), (g, got["count"][g], got["status"][g], o["count"], o["status"])
        assert got["lengths"][g].tolist() == o["lengths"].tolist(), g
        assert fo.same(got["levels"][g], o["levels"]), (g, got["levels"][g][:4], o["levels"][:4])
        assert fo.same(got["norm"][g], np.asarray(o["norm"])), (g, got["norm"][g], o["norm"])
        assert fo.same(got["fingerprints"][g], o["fp"]), (g, got["fingerprints"][g][:4], o["fp"][:4])


def _check(eng, sig, lens, rows, starts, ends, E, w=W, D=D, thr=THR, vf=VF, cache=None):
    want = _want(sig, lens, rows, starts, ends, E, w, D, thr, vf, cache)
    got = eng.event_levels(sig, lens, rows, starts, ends, _args(w, D, thr, vf), E)
    _compare(got, want, E)
    # the segmentation's outputs are adp_segment_events' bytes
    _, info, stats = eng.segment_events(sig, lens, rows, starts, ends, _args(w, D, thr, vf), cap=0)
    assert info.tobytes() == got["info"].tobytes() and fo.same(stats, got["stats"])
    return got, want


LENGTHS = [0, 1, 2 * W - 1, 2 * W, 2 * W + 1, 64, 65, 1023, 1024, 1025, 3500]


@pytest.fixture(scope="module")
def staircases():
    xs = [eo.staircase(np.random.default_rng(1), n) for n in LENGTHS]
    return _pad(xs)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("E", [2, 16, 110, 512])
def test_staircases_of_the_lengths_that_matter(eng, staircases, dtype, E):
    sig, lens = staircases
    if dtype == np.float64:  # values float32 cannot hold: the order of a level's sum shows
        sig = sig.astype(np.float64) + 1e-7 * np.random.default_rng(2).normal(size=sig.shape)
    rows = np.arange(len(LENGTHS), dtype=np.int32)
    got, want = _check(eng, sig, lens, rows, np.zeros(rows.size, dtype=np.int64), lens.astype(np.int64), E)
    nk = want[-1]["nk"]
    assert nk > 110 and nk < 511  # 3500 samples: E = 16 and E = 110 select, E = 512 does not
    assert want[-1]["count"] == min(E, nk + 1) and [o["status"] for o in want[:3]] == [2, 2, 2] and want[3]["status"] in (0, 4)


@pytest.mark.parametrize("E", [2, 16, 110])
def test_exactly_as_many_boundaries_as_fit_one_fewer_and_one_more(eng, E):
    """slices [0, end) of one staircase with exactly E - 2, E - 1 and E boundaries: the selection's threshold"""
    x = eo.staircase(np.random.default_rng(1), 3500)
    ends, n = {}, 2 * W
    while len(ends) < 3 and n <= x.size:
        k = eo.segment(x[:n], W, D, THR, VF)[0].size
        if k in (E - 2, E - 1, E) and k not in ends:
            ends[k] = n
        n += 1
    assert sorted(ends) == [E - 2, E - 1, E]
    e = np.asarray([ends[k] for k in sorted(ends)], dtype=np.int64)
    got, want = _check(eng, x[None, :].copy(), [x.size], np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int64), e, E)
    assert [o["nk"] for o in want] == [E - 2, E - 1, E] and [o["count"] for o in want] == [E - 1, E, E]


def test_the_selection_cuts_through_a_class_of_equal_scores(eng):
    x = np.tile(eo.staircase(np.random.default_rng(2), 200), 6)
    b = eo.segment(x, W, D, THR, VF)[0]
    sc = eo.scores(x, W, VF)[b]
    E = 10
    order = np.lexsort((b, sc))
    cut, first_kept = order[b.size - E], order[b.size - (E - 1)]
    assert b.size > E and sc[cut] == sc[first_kept] and b[cut] < b[first_kept]  # the earlier of two equal scores goes
    tied = b[sc == sc[cut]]
    assert tied.size >= 2 and np.diff(tied).min() >= D
    got, want = _check(eng, x[None, :].copy(), [x.size], [0], [0], [x.size], E)
    kept = np.cumsum(want[0]["lengths"][:E - 1])
    assert b[first_kept] in kept and b[cut] not in kept
    for E2 in (5, 20, 41, 42):
        _check(eng, x[None, :].copy(), [x.size], [0], [0], [x.size], E2)


def test_event_sizes(eng):
    rng = np.random.default_rng(3)
    f64 = lambda x: x.astype(np.float64) + 1e-7 * rng.normal(size=x.size)  # noqa: E731
    tiny = f64(eo.staircase(rng, 600, dwell=(1, 7), noise_sd=0.2))
    mid = f64(eo.staircase(rng, 3000, dwell=(60, 128), noise_sd=1.0))
    big = f64(eo.staircase(rng, 6000, dwell=(129, 700), noise_sd=1.0))
    flat = f64(np.concatenate([eo.staircase(rng, 1500), np.full(9000, 70.0, dtype=np.float32) + rng.normal(0, 0.5, 9000).astype(np.float32),
                               eo.staircase(rng, 1500)]))
    sig, lens = _pad([tiny, mid, big, flat])
    z, e = np.zeros(1, dtype=np.int64), lambda r: lens[r:r + 1].astype(np.int64)  # noqa: E731
    got, want = _check(eng, sig, lens, [0], z, e(0), 512, w=2, D=1, thr=30.0)
    ln = want[0]["lengths"][:want[0]["count"]]
    assert set(range(1, 8)) <= set(ln.tolist()) or (ln.min() <= 2 and (ln <= 7).sum() > 20)
    for r, E in ((1, 110), (2, 110), (3, 512), (3, 16)):
        got, want = _check(eng, sig, lens, [r], z, e(r), E, thr=200.0 if r == 3 else THR)  # (no boundary in the flat stretch's noise)
        ln = want[0]["lengths"][:want[0]["count"]]
        if r == 1:
            assert ((ln >= 8) & (ln <= 128)).sum() > 10
        if r == 2:
            assert (ln >= 129).sum() > 5
        if r == 3:
            assert ln.max() > 8192  # more than numpy's buffer of a reduction


def test_status_and_nan_cases(eng):
    rng = np.random.default_rng(4)
    a = eo.staircase(rng, 1200)
    plateaus = np.repeat(np.asarray([80.0, 120.0, 80.0], dtype=np.float32), 40)
    inf1 = a.copy()
    inf1[300] = np.inf
    nan1 = a.copy()
    nan1[700] = np.nan
    two = np.repeat(np.asarray([80.0, 120.0], dtype=np.float32), 40)
    two[70] = np.inf  # two events, one of them infinite: the median of the levels is
    sig, lens = _pad([a, plateaus, inf1, nan1, two])
    segs = [(0, 0, 1200), (1, 0, 120), (2, 0, 1200), (2, 0, 290), (3, 0, 1200), (3, 0, 700), (3, 701, 1200), (0, 5, 20), (0, 7, 7), (1, 0, 40),
            (4, 0, 80)]
    rows, starts, ends = (np.asarray(v) for v in zip(*segs))
    got, want = _check(eng, sig, lens, rows.astype(np.int32), starts.astype(np.int64), ends.astype(np.int64), 32)
    st = [o["status"] for o in want]
    assert st[0] == 0 and st[1] == 4 and st[4] == 1 and st[5] == st[6] == 0 and st[7] == st[8] == 2 and st[9] == 4
    assert want[1]["levels"][:3].tolist() == [80.0, 120.0, 80.0] and want[1]["lengths"][:4].tolist() == [40, 40, 40, 0]
    assert want[9]["count"] == 1 and st[2] in (0, 4) and np.isinf(want[2]["levels"]).sum() == 1  # one infinite level among many
    assert st[10] == 4 and want[10]["count"] == 2 and want[10]["levels"][:2].tolist() == [80.0, np.inf]  # the table stays, no fingerprint
    assert np.isnan(got["fingerprints"][10]).all() and got["lengths"][10, :3].tolist() == [40, 40, 0]
    # permuted segments: the caller's order is the outputs' order
    perm = np.random.default_rng(5).permutation(len(segs))
    got2 = eng.event_levels(sig, lens, rows[perm].astype(np.int32), starts[perm], ends[perm], _args(), 32)
    for k in got:
        assert fo.same(got[k][perm], got2[k]), k


def test_batches_of_slots_a_second_call_and_device_input(eng, monkeypatch):
    from adapted_amd import lib

    rng = np.random.default_rng(6)
    L = 40000
    monkeypatch.setenv("ADP_EVENTS_SCRATCH_MIB", "8")
    slots = (8 << 20) // lib.events_slot_bytes(L)
    sig = eo.staircase(rng, L)[None, :].copy()
    tail = [(0, 100 * k, 100 * k + 900 + 37 * k) for k in range(1, 8)]
    n_full = slots + 3
    rows = np.zeros(n_full + len(tail), dtype=np.int32)
    starts = np.asarray([0] * n_full + [t[1] for t in tail], dtype=np.int64)
    ends = np.asarray([L] * n_full + [t[2] for t in tail], dtype=np.int64)
    cache = {}
    got, want = _check(eng, sig, [L], rows, starts, ends, 110, cache=cache)
    assert want[0]["nk"] > 500 and want[0]["count"] == 110
    monkeypatch.delenv("ADP_EVENTS_SCRATCH_MIB")
    one = eng.event_levels(sig, [L], rows, starts, ends, _args(), 110)  # a second call, one batch
    for k in got:
        assert fo.same(got[k], one[k]), k
    d = eng.dev_alloc(sig.nbytes)
    try:
        eng.h2d(d, sig)
        dev = eng.event_levels(d, [L], rows[-9:], starts[-9:], ends[-9:], _args(), 110, n=1, L=L)
        for k in got:
            assert fo.same(got[k][-9:], dev[k]), k
    finally:
        eng.dev_free(d)


@pytest.mark.parametrize("E", [1, 0, -1, 513])
def test_a_width_out_of_range_is_refused_and_the_handle_stays_usable(eng, E):
    from adapted_amd import lib

    sig = eo.staircase(np.random.default_rng(7), 800)[None, :].copy()
    with pytest.raises(lib.HipLibraryError, match="max_events"):
        eng.event_levels(sig, [800], [0], [0], [800], _args(), E)
    with pytest.raises(lib.HipLibraryError, match="window"):
        eng.event_levels(sig, [800], [0], [0], [800], _args(w=1), 16)
    _check(eng, sig, [800], [0], [0], [800], 16)


# ---- DTW

COUNTS = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512]


def _sequences(rng, counts, E):
    v = np.full((len(counts), E), np.nan)
    for p, c in enumerate(counts):
        c = min(max(int(c), 0), E)
        v[p, :c] = np.cumsum(rng.normal(0.0, 1.0, c)) * 0.3 + rng.normal(0.0, 1.0, c)
    return v


def _dtw_check(eng, q, qc, t, tc, band, want_dist=True, oracle=None):
    qc, tc = np.asarray(qc, dtype=np.int32), np.asarray(tc, dtype=np.int32)
    want = fo.dtw(q, qc, t, tc, band) if oracle is None else oracle
    wbest, wbd = fo.assign(want)
    dist, best, bd = eng.dtw_assign(q, qc, t, tc, band, want_dist=want_dist)  # (NaN beyond a count: not read)
    if want_dist:
        assert fo.same(dist, want), np.argwhere(~((dist == want) | (np.isnan(dist) & np.isnan(want))))[:5]
    else:
        assert dist is None
    assert best.dtype == np.int32 and fo.same(best, wbest) and fo.same(bd, wbd)
    return want, best, bd


@pytest.mark.parametrize("band", [0, 1, 5])
def test_dtw_counts_at_the_lanes_strip_edges(eng, band):
    """every pair of query and template counts at the edges of a lane's strip of columns, Eq = Et = 512 (C = 8)"""
    rng = np.random.default_rng(8 + band)
    q, t = _sequences(rng, COUNTS, 512), _sequences(rng, COUNTS, 512)
    want, _, _ = _dtw_check(eng, q, COUNTS, t, COUNTS, band)
    assert np.isfinite(want).all() and (np.diag(want) > 0).all()


@pytest.mark.parametrize("Eq,Et", [(110, 110), (40, 129), (300, 64), (7, 256), (1, 1)])
def test_dtw_widths_bands_and_batch_sizes(eng, Eq, Et):
    """Eq != Et and every C in {1, 2, 4, 8}; nq in {1, 65, 300} against nt in {1, 3, 13}; |n - m| above and below the band"""
    rng = np.random.default_rng(Eq * 1000 + Et)
    for nq, nt, band in ((1, 1, 0), (65, 3, 5), (300, 13, 1), (65, 13, 0)):
        if Eq * Et > 10000 and nq == 300:
            nq = 30  # (the oracle's time: a few hundred pairs at these widths)
        qc = rng.integers(1, Eq + 1, nq)
        tc = rng.integers(1, Et + 1, nt)
        qc[0], tc[0] = Eq, Et
        if nq > 2:
            qc[1] = min(Eq, tc[0] + 2) if Eq > 1 else 1  # within a band of 5 of template 0's count
        q, t = _sequences(rng, qc, Eq), _sequences(rng, tc, Et)
        want, _, _ = _dtw_check(eng, q, qc, t, tc, band)
        if band and nq > 2 and Eq > 20 and Et > 20:
            dm = np.abs(qc[:, None] - tc[None, :])
            assert (dm > band).any() and (dm < band).any()


def test_dtw_duplicate_template_refused_queries_and_no_matrix(eng):
    rng = np.random.default_rng(9)
    Eq, Et = 30, 24
    tc = np.asarray([24, 10, 24, 17], dtype=np.int32)
    t = _sequences(rng, tc, Et)
    t[2] = t[0]  # a duplicate: the lower index wins, the second best equals the best
    qc = np.asarray([24, 0, Eq + 1, 12, 30, -3, 9], dtype=np.int32)
    q = _sequences(rng, qc, Eq)
    q[0, :24] = t[0, :24] + 0.01
    q[3, 5] = np.nan  # inside its count
    q[4, 7] = np.inf
    q[6, 20] = np.nan  # beyond its count: not read
    q[2, :] = 1.0
    want, best, bd = _dtw_check(eng, q, qc, t, tc, 0)
    assert best[0].tolist() == [0, 2] and bd[0, 0] == bd[0, 1]
    assert np.isnan(want[[1, 2, 3, 4, 5]]).all() and (best[[1, 2, 3, 4, 5]] == -1).all() and np.isfinite(want[6]).all()
    _dtw_check(eng, q, qc, t, tc, 3, want_dist=False)
    one, best1, bd1 = _dtw_check(eng, q, qc, t[:1], tc[:1], 0)  # one template: no second
    assert best1[0].tolist() == [0, -1] and np.isnan(bd1[0, 1]) and bd1[0, 0] == one[0, 0]


def test_dtw_crosses_the_query_batch_boundary(eng, monkeypatch):
    """with a budget of 1 MiB a distance matrix of 600 templates holds 218 queries: 300 take two batches"""
    from adapted_amd import lib

    rng = np.random.default_rng(10)
    nq, nt, E = 300, 600, 6
    assert (1 << 20) // (nt * 8) == 218 and lib.DTW_SCRATCH_MIB == 512
    qc, tc = rng.integers(1, E + 1, nq), rng.integers(1, E + 1, nt)
    q, t = _sequences(rng, qc, E), _sequences(rng, tc, E)
    want = fo.dtw(q, qc, t, tc, 2)
    monkeypatch.setenv("ADP_DTW_SCRATCH_MIB", "1")
    _dtw_check(eng, q, qc, t, tc, 2, oracle=want)
    _dtw_check(eng, q, qc, t, tc, 2, want_dist=False, oracle=want)
    monkeypatch.delenv("ADP_DTW_SCRATCH_MIB")
    _dtw_check(eng, q, qc, t, tc, 2, oracle=want)
    monkeypatch.setenv("ADP_DTW_SCRATCH_MIB", "0")
    with pytest.raises(lib.HipLibraryError, match="ADP_DTW_SCRATCH_MIB"):
        eng.dtw_assign(q[:2], qc[:2].astype(np.int32), t, tc.astype(np.int32), 0)


@pytest.mark.parametrize("bad", ["nt", "Et", "Eq", "count0", "count_big", "nan", "inf", "band"])
def test_dtw_refuses_bad_templates_and_the_handle_stays_usable(eng, bad):
    rng = np.random.default_rng(11)
    q, qc = _sequences(rng, [5, 6], 8), np.asarray([5, 6], dtype=np.int32)
    t, tc = np.where(np.isnan(_sequences(rng, [4, 8, 3], 8)), 0.0, _sequences(rng, [4, 8, 3], 8)), np.asarray([4, 8, 3], dtype=np.int32)
    nt, Et, Eq, band = 3, 8, 8, 0
    if bad == "nt":
        nt = 4097
    elif bad == "Et":
        Et = 513
    elif bad == "Eq":
        Eq = 0
    elif bad == "count0":
        tc[1] = 0
    elif bad == "count_big":
        tc[2] = 9
    elif bad == "nan":
        t[0, 3] = np.nan
    elif bad == "inf":
        t[1, 7] = -np.inf
    else:
        band = -1
    big_t = np.zeros((max(nt, 3), max(Et, 8)))
    big_t[:3, :8] = t
    big_tc = np.ones(max(nt, 3), dtype=np.int32)
    big_tc[:3] = tc
    best, bd = np.zeros((2, 2), dtype=np.int32), np.zeros((2, 2))
    rc = eng.lib.adp_dtw_assign(eng._h, np.ascontiguousarray(q), qc, 2, Eq, big_t if bad in ("nt", "Et") else np.ascontiguousarray(t),
                                big_tc if bad in ("nt", "Et") else tc, nt, Et, band, 0, None, best, bd)
    assert rc == -1 and eng.lib.adp_last_error()
    t2 = np.where(np.isfinite(t), t, 0.0)
    _dtw_check(eng, q, qc, t2, np.asarray([4, 8, 3], dtype=np.int32), 0)


def test_fingerprints_stay_on_the_device_between_the_two_calls(eng):
    """event_levels with ADP_OUT_DEVICE, then dtw_assign with ADP_IN_DEVICE: what the form through host arrays gives, and the oracle"""
    rng = np.random.default_rng(12)
    E, n = 24, 40
    xs = [eo.staircase(rng, int(k)) for k in rng.integers(200, 900, n)]
    xs[3] = xs[3][:10]  # status 2: count 0, a refused query
    sig, lens = _pad(xs)
    rows, starts, ends = np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int64), lens.astype(np.int64)
    host, want = _check(eng, sig, lens, rows, starts, ends, E)
    tidx = [0, 5, 9]
    t = np.where(np.isnan(host["fingerprints"][tidx]), 0.0, host["fingerprints"][tidx])
    tc = host["count"][tidx]
    assert (host["status"][tidx] == 0).all() and host["count"][3] == 0
    fp_d, cnt_d = eng.dev_alloc(n * E * 8), eng.dev_alloc(n * 4)
    try:
        dev = eng.event_levels(sig, lens, rows, starts, ends, _args(), E, fp_ptr=fp_d, count_ptr=cnt_d)
        assert dev["fingerprints"] is None and dev["count"] is None
        for k in ("info", "stats", "status", "lengths", "levels", "norm"):
            assert fo.same(dev[k], host[k]), k
        chained = eng.dtw_assign(fp_d, cnt_d, t, tc, 3, nq=n, Eq=E)
        back_fp, back_c = np.zeros((n, E)), np.zeros(n, dtype=np.int32)
        eng.d2h(back_fp, fp_d)
        eng.d2h(back_c, cnt_d)
        assert fo.same(back_fp, host["fingerprints"]) and fo.same(back_c, host["count"])
    finally:
        eng.dev_free(fp_d)
        eng.dev_free(cnt_d)
    through_host = eng.dtw_assign(host["fingerprints"], host["count"], t, tc, 3)
    wantd = fo.dtw(np.stack([o["fp"] for o in want]), [o["count"] for o in want], t, tc, 3)
    wbest, wbd = fo.assign(wantd)
    for a, b, c in zip(chained, through_host, (wantd, wbest, wbd)):
        assert fo.same(a, b) and fo.same(a, c)
    assert np.isnan(wantd[3]).all() and chained[1][0].tolist()[0] == 0 and chained[2][0, 0] == 0.0


def test_one_engine_alternating_modules_against_fresh_engines(eng):
    """the modules share one workspace: event_levels, dtw_assign, segment_events and seg_stats in turn on one engine give what
    each gives on an engine of its own"""
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config

    rng = np.random.default_rng(13)
    sig, lens = _pad([eo.staircase(rng, 1500), eo.staircase(rng, 1400), eo.staircase(rng, 900)])
    rows, starts, ends = np.arange(3, dtype=np.int32), np.zeros(3, dtype=np.int64), lens.astype(np.int64)
    qc = rng.integers(1, 41, 20).astype(np.int32)
    q = np.where(np.isnan(_sequences(rng, qc, 40)), 0.0, _sequences(rng, qc, 40))
    calls = [lambda e: e.event_levels(sig, lens, rows, starts, ends, _args(), 32),
             lambda e: e.dtw_assign(q, qc, q[:4], qc[:4], 2),
             lambda e: e.segment_events(sig, lens, rows, starts, ends, _args(), cap=16),
             lambda e: e.seg_stats(sig, lens, rows, starts, ends),
             lambda e: e.event_levels(sig[:, :1000].copy(), [1000, 1000, 900], rows, starts + 3, ends, _args(10, 37, 50.0), 8),
             lambda e: e.dtw_assign(q, qc, q[:4], qc[:4], 0, want_dist=False)]
    spc = get_chemistry_specific_config("RNA004")

    def flat(r):
        vals = list(r.values()) if isinstance(r, dict) else list(r)
        return [v for v in vals if v is not None]

    mixed = [flat(c(eng)) for c in calls + calls[::-1]]
    for c, got in zip(calls + calls[::-1], mixed):
        fresh = lib.Engine(spc, 1, spc.sig_preload_size)
        try:
            for a, b in zip(flat(c(fresh)), got):
                assert fo.same(a, b)
        finally:
            fresh.close()


def test_medoid_templates_and_assign_barcodes(eng):
    from adapted_amd import fingerprint as fpm

    rng = np.random.default_rng(14)
    E = 20
    base = _sequences(rng, [18, 20, 15], E)
    counts, labels, rowsv = [], [], []
    for lab, name in enumerate(["bc03", "bc01", "bc02"]):
        for k in range(8):
            c = int(np.isfinite(base[lab]).sum()) - (k % 3)
            v = np.full(E, np.nan)
            v[:c] = base[lab, :c] + rng.normal(0.0, 0.15, c)
            rowsv.append(v)
            counts.append(c)
            labels.append(name)
    fp, counts = np.stack(rowsv), np.asarray(counts, dtype=np.int32)
    order = rng.permutation(len(labels))
    fp, counts, labels = fp[order], counts[order], [labels[i] for i in order]
    tm = fpm.medoid_templates(fp, counts, labels, band=2, engine=eng)
    zero = np.where(np.isnan(fp), 0.0, fp)
    dist = fo.dtw(zero, counts, zero, counts, 2)
    want_rows = fo.medoids(dist, labels)
    assert tm.names == ["bc01", "bc02", "bc03"] and tm.counts.tolist() == counts[want_rows].tolist()
    assert fo.same(tm.levels, np.stack([np.where(np.arange(E) < counts[r], fp[r], np.nan) for r in want_rows]))
    got = fpm.assign_barcodes(fp, counts, tm, band=2, engine=eng)
    wbest, wbd = fo.assign(dist[:, want_rows])
    assert fo.same(got.best, wbest[:, 0].copy()) and fo.same(got.second, wbest[:, 1].copy())
    assert fo.same(got.dist, wbd[:, 0].copy()) and fo.same(got.margin, wbd[:, 1] - wbd[:, 0])
    assert [tm.names[b] for b in got.best] == labels  # (well separated synthetic classes: not a claim about real barcodes)
    d2 = fpm.dtw_distances(fp, counts, zero[want_rows], counts[want_rows], band=2, engine=eng)
    assert fo.same(d2, dist[:, want_rows].copy())
