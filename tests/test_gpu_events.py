"""adp_segment_events (include/adapted_hip_events.h; kernels: adapted_amd/csrc/events_api.h) against its numpy + scipy oracle
(tests/events_oracle.py): positions, counts, status and the two statistics bit for bit (all NaNs count as one), no tolerance --
every rounding of the algorithm is specified.  Every generated input is first checked, on the oracle's side, to hold no two
candidates closer than the minimum distance with equal scores, so that the tie rule is not what is compared."""
import ctypes

import numpy as np
import pytest

import events_oracle as eo
from adapted_amd.lib import EVENTS_TILE as TILE  # positions per workgroup of the score kernel (tests/test_events_cpu.py holds it against the header)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def _args(w=8, D=8, thr=16.0, vf=1e-3):
    from adapted_amd import lib

    a = lib.AdpEventArgs()
    a.window, a.min_distance, a.threshold, a.var_floor = w, D, thr, vf
    return a


def _bits(a):
    a = np.array(a, dtype=np.float64)
    a[a != a] = np.nan
    return a.view(np.uint64).tolist()


def _want(sig, lens, rows, starts, ends, w, D, thr, vf, cache=None):
    """the oracle's answer per segment (identical segments computed once), with the tie precondition asserted"""
    cache = {} if cache is None else cache
    out = []
    for r, s, e in zip(rows, starts, ends):
        key = (int(r), int(s), int(e))
        if key not in cache:
            x = eo.clip(sig[r], int(lens[r]), int(s), int(e))
            assert not eo.has_close_ties(x, w, D, thr, vf), ("the input has tied candidates within the distance", key)
            cache[key] = eo.segment(x, w, D, thr, vf)
        out.append(cache[key])
    return out


def _compare(got, want, cap):
    pos, info, stats = got
    assert info.shape == (len(want), 2) and stats.shape == (len(want), 2) and pos.shape == (len(want), cap)
    for g, (b, status, med, mad) in enumerate(want):
        assert (int(info[g, 0]), int(info[g, 1])) == (b.size, status), (g, info[g], b.size, status)
        k = min(cap, b.size)
        assert pos[g, :k].tolist() == b[:k].tolist(), g
        assert (pos[g, k:] == -1).all(), g
        assert _bits(stats[g]) == _bits([med, mad]), (g, stats[g], med, mad)


def _check(eng, sig, lens, rows, starts, ends, w=8, D=8, thr=16.0, vf=1e-3, cap=None, cache=None):
    want = _want(sig, lens, rows, starts, ends, w, D, thr, vf, cache)
    if cap is None:
        cap = max([b.size for b, _, _, _ in want] + [1])
    got = eng.segment_events(sig, lens, rows, starts, ends, _args(w, D, thr, vf), cap=cap)
    _compare(got, want, cap)
    return got, want


def _length_cases(w):
    ns = {0, 1, 2 * w - 1, 2 * w, 2 * w + 1, 63, 64, 65, 127, 128, 129, 3500, 40000}
    # around the score kernel's tile: one tile / two, a last tile shorter than a window, the halo at a tile's edge
    ns |= {TILE - 1, TILE, TILE + 1, TILE + w - 1, TILE + w, TILE + w + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, TILE - w, TILE - w + 1}
    return sorted(ns)


@pytest.fixture(scope="module")
def staircases():
    """one float32 staircase per length of any window's list: levels N(85, 12^2), a dwell per event, noise sd 2"""
    rng = np.random.default_rng(20240)
    ns = sorted(set(n for w in (2, 8, 10, 64) for n in _length_cases(w)))
    sig = np.full((len(ns), 40000), np.nan, dtype=np.float32)
    for r, n in enumerate(ns):
        sig[r, :n] = eo.staircase(rng, n)
    return ns, sig, np.asarray(ns, dtype=np.int32)


@pytest.mark.parametrize("w", [2, 8, 10, 64])
@pytest.mark.parametrize("dk", ["one", "w", "37"])
def test_lengths_windows_distances_thresholds(eng, staircases, w, dk):
    ns, sig, lens = staircases
    D = {"one": 1, "w": w, "37": 37}[dk]
    rows = np.asarray([ns.index(n) for n in _length_cases(w)], dtype=np.int32)
    for thr in (16.0, 100.0):
        got, want = _check(eng, sig, lens, rows, np.zeros(rows.size, dtype=np.int64), lens[rows].astype(np.int64), w, D, thr)
        assert sum(b.size for b, _, _, _ in want) > 100 and any(b.size >= 2 for b, _, _, _ in want)
        for n, (b, status, _, _) in zip(_length_cases(w), want):
            assert status == (2 if n < 2 * w else 0)


def test_one_step_at_every_offset_of_a_tile_edge(eng):
    """161 segments of 400 samples, one step 80 -> 96 at p = 100 .. 260, each placed so that the step crosses the first tile edge
    of its row's score tiles at a different offset"""
    rng = np.random.default_rng(7)
    ps = np.arange(100, 261)
    L = TILE + 400
    sig = rng.normal(0.0, 1.0, size=(ps.size, L)).astype(np.float32)
    starts = np.zeros(ps.size, dtype=np.int64)
    for k, p in enumerate(ps):
        starts[k] = TILE - 400 + (k * 5) % 400  # the slice may start anywhere in the row
        sig[k, starts[k]:starts[k] + 400] += np.where(np.arange(400) < p, 80.0, 96.0).astype(np.float32)
    lens = np.full(ps.size, L, dtype=np.int32)
    got, want = _check(eng, sig, lens, np.arange(ps.size, dtype=np.int32), starts, starts + 400, 8, 8, 200.0)
    for p, (b, _, _, _) in zip(ps, want):
        assert b.size == 1 and abs(int(b[0]) - p) <= 1
    # the same steps inside LONG slices, so that they meet the score kernel's tile edges: a step at 1024 - 80 + p of 3 tiles
    sig2 = rng.normal(0.0, 1.0, size=(ps.size, 3 * TILE)).astype(np.float32)
    for k, p in enumerate(ps):
        sig2[k] += np.where(np.arange(3 * TILE) < TILE - 180 + p, 80.0, 96.0).astype(np.float32)
    lens2 = np.full(ps.size, 3 * TILE, dtype=np.int32)
    got, want = _check(eng, sig2, lens2, np.arange(ps.size, dtype=np.int32), np.zeros(ps.size, dtype=np.int64),
                       np.full(ps.size, 3 * TILE, dtype=np.int64), 8, 8, 200.0)
    for p, (b, _, _, _) in zip(ps, want):
        assert b.size == 1 and abs(int(b[0]) - (TILE - 180 + p)) <= 1


def test_distance_rule_is_a_cascade(eng):
    x = np.repeat([0, 1, 3, 7, 15, 31], [10, 5, 5, 5, 5, 10]).astype(np.float64)
    x = x + np.resize([0, .25, -.25, .125], x.size)
    c, h = eo.candidates(x, 3, 1.0, 1e-3)
    assert c.tolist() == [6, 10, 15, 20, 25, 30, 34] and (np.diff(h[:-1]) > 0).all()
    sig = x[None, :].copy()
    got, want = _check(eng, sig, [x.size], [0], [0], [x.size], 3, 6, 1.0)
    assert want[0][0].tolist() == [10, 20, 30]  # ("drop whatever has a higher neighbour within D" would keep [30])
    assert got[0][0, :3].tolist() == [10, 20, 30]


@pytest.mark.parametrize("flank", [20, 300, 1500])
def test_plateau_midpoint_rounds_down(eng, flank):
    x = np.asarray([0] * flank + [5] + [10] * flank, dtype=np.float32)
    sc = eo.scores(x, 8, 1e-3)
    assert sc[flank] == sc[flank + 1] and sc[flank - 1] < sc[flank] > sc[flank + 2]
    # (the two equal scores are ONE plateau, not two candidates: has_close_ties sees one maximum)
    got, want = _check(eng, x[None, :].copy(), [x.size], [0], [0], [x.size])
    assert want[0][0].tolist() == [flank]


def test_slices_nan_clipping_and_segment_order(eng):
    rng = np.random.default_rng(11)
    L = 3000
    sig = np.stack([eo.staircase(rng, L) for _ in range(4)])
    lens = np.asarray([3000, 2500, 1800, 0], dtype=np.int32)
    sig[0, 1000] = np.nan  # inside some slices of row 0, outside others
    sig[1, 2500:] = np.nan  # the padding behind row 1's end
    sig[2, 1800:] = np.nan
    segs = [(0, 0, 1000), (0, 1001, 3000), (0, 990, 1010), (0, 0, 3000), (0, 1000, 1001),  # NaN: outside, outside, inside, inside, alone
            (1, 100, 2500), (1, 100, 2600), (1, 2400, 9000), (1, 2500, 2600), (1, 2600, 2700),  # clipped by len; empty beyond it
            (2, 500, 400), (2, 500, 500), (2, -5, 900), (2, 0, 1800), (2, 0, 1 << 40),  # end <= start, start < 0 (empty), whole, far end
            (3, 0, 100),  # a read of no samples
            (1, 0, 700), (0, 1500, 2600), (2, 300, 1700), (1, 600, 1300), (0, 20, 36), (0, 20, 35)]  # rows out of order; n = 2 w, 2 w - 1
    rows, starts, ends = (np.asarray(v) for v in zip(*segs))
    got, want = _check(eng, sig, lens, rows.astype(np.int32), starts.astype(np.int64), ends.astype(np.int64))
    status = [st for _, st, _, _ in want]
    assert status[:5] == [0, 0, 1, 1, 1] and status[5:10] == [0, 0, 0, 2, 2] and status[10:16] == [2, 2, 2, 0, 0, 2]
    assert want[5][0].tolist() == want[6][0].tolist() and want[5][0].size > 10
    assert status[-2:] == [0, 2]
    # the caller's order of the segments is the outputs' order
    perm = np.random.default_rng(3).permutation(len(segs))
    got2 = eng.segment_events(sig, lens, rows[perm].astype(np.int32), starts[perm], ends[perm], _args(), cap=got[0].shape[1])
    for a, b in zip(got, got2):
        assert _bits(a[perm]) == _bits(b)


def test_cap_device_input_and_float64(eng):
    rng = np.random.default_rng(5)
    n, L = 6, 2600
    sig = np.stack([eo.staircase(rng, L) for _ in range(n)])
    lens = np.asarray([2600, 2599, 1025, 1024, 700, 40], dtype=np.int32)
    rows = np.arange(n, dtype=np.int32)
    starts, ends = np.zeros(n, dtype=np.int64), lens.astype(np.int64)
    cache = {}
    full, want = _check(eng, sig, lens, rows, starts, ends, cache=cache)
    biggest = max(b.size for b, _, _, _ in want)
    assert biggest > 40
    for cap in (0, 7, biggest + 9):
        got, _ = _check(eng, sig, lens, rows, starts, ends, cap=cap, cache=cache)
        assert _bits(got[1]) == _bits(full[1]) and _bits(got[2]) == _bits(full[2])  # count and statistics do not depend on cap
    # the same rows resident on the device
    d = eng.dev_alloc(sig.nbytes)
    try:
        eng.h2d(d, sig)
        dev = eng.segment_events(d, lens, rows, starts, ends, _args(), cap=full[0].shape[1], n=n, L=L)
        for a, b in zip(full, dev):
            assert _bits(a) == _bits(b)
    finally:
        eng.dev_free(d)
    # the same values as float64: the same answer
    f64 = eng.segment_events(sig.astype(np.float64), lens, rows, starts, ends, _args(), cap=full[0].shape[1])
    for a, b in zip(full, f64):
        assert _bits(a) == _bits(b)
    # float64 values float32 cannot hold
    x64 = sig.astype(np.float64) + 1e-9 * rng.normal(size=sig.shape)
    _check(eng, x64, lens, rows, starts, ends)


def test_more_segments_than_one_batch_of_slots(eng, monkeypatch):
    """the scratch of a call is bounded in bytes (512 MiB; ADP_EVENTS_SCRATCH_MIB, read per call, sets another bound): with 8 MiB,
    whole-row segments of 40 000 samples take three batches of slots, and the segments of the last batch are others than the first's"""
    from adapted_amd import lib

    rng = np.random.default_rng(13)
    L = 40000
    monkeypatch.setenv("ADP_EVENTS_SCRATCH_MIB", "8")
    slots = (8 << 20) // lib.events_slot_bytes(L)
    n_full = 2 * slots + 6
    assert slots == 17 and lib.EVENTS_SCRATCH_MIB == 512
    sig = eo.staircase(rng, L)[None, :].copy()
    tail = [(0, 100 * k, 100 * k + 900 + 37 * k) for k in range(1, 16)]
    rows = np.zeros(n_full + len(tail), dtype=np.int32)
    starts = np.asarray([0] * n_full + [t[1] for t in tail], dtype=np.int64)
    ends = np.asarray([L] * n_full + [t[2] for t in tail], dtype=np.int64)
    got, want = _check(eng, sig, [L], rows, starts, ends, cap=64)
    assert want[0][0].size > 500 and len(set(tuple(b.tolist()) for b, _, _, _ in want[n_full:])) == len(tail)
    # the default budget gives the same answers in one batch; a budget that is no number of MiB is refused
    monkeypatch.delenv("ADP_EVENTS_SCRATCH_MIB")
    one = eng.segment_events(sig, [L], rows, starts, ends, _args(), cap=64)
    for a, b in zip(got, one):
        assert _bits(a) == _bits(b)
    monkeypatch.setenv("ADP_EVENTS_SCRATCH_MIB", "0")
    with pytest.raises(lib.HipLibraryError, match="ADP_EVENTS_SCRATCH_MIB"):
        eng.segment_events(sig, [L], rows[:2], starts[:2], ends[:2], _args(), cap=4)
    monkeypatch.delenv("ADP_EVENTS_SCRATCH_MIB")
    _check(eng, sig, [L], rows[-3:], starts[-3:], ends[-3:])


def test_one_engine_many_calls(eng):
    rng = np.random.default_rng(17)
    sig = np.stack([eo.staircase(rng, 1500) for _ in range(3)])
    lens = np.asarray([1500, 1400, 900], dtype=np.int32)
    rows, starts, ends = np.arange(3, dtype=np.int32), np.zeros(3, dtype=np.int64), lens.astype(np.int64)
    first, _ = _check(eng, sig, lens, rows, starts, ends, 8, 8, 16.0, cap=100)
    _check(eng, sig[:, :1000].copy(), [1000, 1000, 900], rows, starts + 3, ends, 10, 37, 50.0, cap=5)
    stats, cnt = eng.seg_stats(sig, lens, rows, starts, ends)
    assert cnt.tolist() == lens.tolist() and np.isfinite(stats).all()
    again = eng.segment_events(sig, lens, rows, starts, ends, _args(), cap=100)
    for a, b in zip(first, again):
        assert _bits(a) == _bits(b)


@pytest.mark.parametrize("bad", [dict(w=1), dict(w=65), dict(w=0), dict(D=0), dict(D=-3), dict(thr=0.0), dict(thr=-1.0),
                                 dict(thr=float("nan")), dict(thr=float("inf")), dict(vf=0.0), dict(vf=-1e-3), dict(vf=float("nan")),
                                 dict(vf=float("inf")), dict(cap=-1)])
def test_invalid_arguments_are_refused_and_the_handle_stays_usable(eng, bad):
    from adapted_amd import lib

    rng = np.random.default_rng(19)
    sig = eo.staircase(rng, 800)[None, :].copy()
    lens = np.asarray([800], dtype=np.int32)
    segs = np.zeros(1, dtype=lib.SEG_DTYPE)
    segs["end"] = 800
    kw = dict(bad)
    cap = kw.pop("cap", 4)
    pos, info, stats = np.zeros((1, 4), dtype=np.int64), np.zeros((1, 2), dtype=np.int64), np.zeros((1, 2))
    rc = eng.lib.adp_segment_events(eng._h, sig, lens, 1, 800, segs, 1, ctypes.byref(_args(**kw)), 0, cap, pos, info, stats)
    assert rc == -1 and eng.lib.adp_last_error()  # ADP_ERR_INVALID
    _check(eng, sig, lens, [0], [0], [800])
