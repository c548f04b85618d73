"""adp_dtw_knn (include/adapted_hip_knn.h; kernels: adapted_amd/csrc/dtw_knn_api.h) and `adapted knn` on the GPU.  Every comparison
is bit for bit, no tolerance: the wanted neighbours are adp_dtw_assign's distances -- dtw_distances, in chunks of at most 4096
references -- ordered by np.lexsort((index, distance)), and for the small cases the numpy oracle's too (tests/dtw_knn_oracle.py).
Pruning must not change a bit: every case runs with and without it."""
import os
import sys

import numpy as np
import pytest

import clusters_cases as cc
import dtw_knn_oracle as ko

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def _matrix(eng, q, qc, r, rc, band):
    """dtw_distances of every query to every reference: what the parent commit offers, 4096 references at a time"""
    from adapted_amd.fingerprint import dtw_distances

    return np.concatenate([dtw_distances(q, qc, r[a:a + 4096], rc[a:a + 4096], band, engine=eng) for a in range(0, r.shape[0], 4096)], axis=1)


def _same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape == got[1].shape
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert ko.same(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[0] < 0, np.isnan(got[1]))


def _both(eng, q, qc, r, rc, k, band, ex, want):
    """the pruned and the unpruned call against ``want``, and what the header holds the work counters to"""
    cand = ko.candidates(q, qc, r.shape[0], ex)
    for prune in (True, False):
        idx, dist, work = eng.dtw_knn(q, qc, r, rc, k, band, exclude=ex, prune=prune, want_work=True)
        _same((idx, dist), want)
        assert work.dtype == np.int64 and (work >= 0).all() and np.array_equal(work[:, 0] + work[:, 1], cand)
        assert (work[cand == 0] == 0).all()
        if not prune:
            assert (work[:, 1] == 0).all() and np.array_equal(work[:, 2], ko.full_steps(q, qc, rc, r.shape[1], ex))
        else:
            assert (work[:, 2] <= ko.full_steps(q, qc, rc, r.shape[1], ex)).all()
    assert eng.dtw_knn(q, qc, r, rc, k, band, exclude=ex)[0].shape == want[0].shape  # (without the counters: a pair)


@pytest.mark.parametrize("Er", [1, 2, 64, 65, 130, 257])
@pytest.mark.parametrize("nr", [1, 2, 63, 65, 130])
def test_knn_is_dtw_assign_ordered_by_lexsort(eng, nr, Er):
    nq, Eq = 9, (Er + 2 if Er % 2 == 0 else max(1, Er - 1))  # (a width of the queries' own)
    q, qc, ok = cc.ragged(nq, Eq, 100 * nr + Er)
    assert (~ok).sum() == 4 and qc.min() == 0 and qc.max() == Eq + 1  # count 0, count Eq + 1, a NaN, an infinity
    r, rc, _ = cc.ragged(nr, Er, 7 * nr + Er, unusable=False)
    assert nr == 1 or rc[1] == 1  # ragged down to 1
    ex = np.asarray([p % nr if p % 2 else -1 for p in range(nq)], dtype=np.int32)
    for band in (0, 1, 5):
        D = _matrix(eng, q, qc, r, rc, band)
        assert np.isnan(D[~ok]).all() and not np.isnan(D[ok]).any()
        if nr * Er <= 65 * 65:
            from fingerprint_oracle import dtw

            assert ko.same(D, dtw(q, qc, r, rc, band))
        for k in (1, 3, 32):
            for e in (None, ex):
                want = ko.topk(D, k, e)
                assert (want[0][~ok] == -1).all() and (want[0][ok, :min(k, nr - 1)] >= 0).all()
                _both(eng, q, qc, r, rc, k, band, e, want)


def test_ties_go_to_the_lower_index(eng):
    k, E = 4, 20
    rng = np.random.default_rng(5)
    r, rc, _ = cc.ragged(60, E, 11, low=3, unusable=False)
    copies = np.sort(rng.permutation(60)[:2 * k + 3])
    r[copies], rc[copies] = r[copies[0]], rc[copies[0]]
    q, qc, ok = cc.ragged(9, E, 12, low=3)
    q[0], qc[0] = r[copies[0]], rc[copies[0]]  # a query that IS the copied reference: +0.0, 2k + 3 times
    q[1], qc[1] = r[5], rc[5]
    for band in (0, 2):
        D = _matrix(eng, q, qc, r, rc, band)
        want = ko.topk(D, k)
        assert want[0][0].tolist() == copies[:k].tolist() and (want[1][0] == 0.0).all() and not np.signbit(want[1][0]).any()
        _both(eng, q, qc, r, rc, k, band, None, want)
        ex = np.full(9, -1, dtype=np.int32)
        ex[0] = copies[1]
        want = ko.topk(D, 2 * k + 3, ex)
        assert want[0][0].tolist()[:2 * k + 2] == [c for c in copies.tolist() if c != copies[1]]
        _both(eng, q, qc, r, rc, 2 * k + 3, band, ex, want)
    # all-constant sequences: every distance is equal, so the index orders
    rc2 = np.asarray(rng.integers(1, E + 1, 70), dtype=np.int32)
    r2 = np.full((70, E), 1.5)
    q2, qc2 = np.full((3, E), 1.5), np.asarray([1, E, 7], dtype=np.int32)
    for k in (1, 32):
        got = eng.dtw_knn(q2, qc2, r2, rc2, k, 0, exclude=np.asarray([0, -1, 31], dtype=np.int32))
        assert got[0].tolist() == [list(range(1, k + 1)), list(range(k)), [j for j in range(k + 1) if j != 31][:k]]
        assert (got[1] == 0.0).all() and not np.signbit(got[1]).any()


def test_padding_and_self_exclusion(eng):
    q, qc, ok = cc.ragged(12, 33, 21)
    good = np.flatnonzero(ok)
    D = _matrix(eng, q, qc, q[good], qc[good], 0)
    r, rc = np.ascontiguousarray(q[good]), qc[good]
    me = np.full(12, -1, dtype=np.int32)
    me[good] = np.arange(good.size)
    # without the exclusion every usable query is its own nearest, at +0.0
    idx, dist = eng.dtw_knn(q, qc, r, rc, 3)
    assert np.array_equal(idx[good, 0], me[good]) and (dist[good, 0] == 0.0).all() and not np.signbit(dist[good, 0]).any()
    _both(eng, q, qc, r, rc, 3, 0, None, ko.topk(D, 3))
    # with it none gets itself
    idx, dist = eng.dtw_knn(q, qc, r, rc, 3, exclude=me)
    assert not (idx[good] == me[good, None]).any() and (idx[good] >= 0).all()
    _both(eng, q, qc, r, rc, 3, 0, me, ko.topk(D, 3, me))
    # k above the candidates: -1 and NaN behind them
    for nr, k in ((1, 1), (1, 4), (3, 5), (2, 32)):
        e = np.where(me >= nr, -1, me).astype(np.int32)
        want = ko.topk(D[:, :nr], k, e)
        for p in good:
            have = nr - (e[p] >= 0)
            assert (want[0][p, :have] >= 0).all() and (want[0][p, have:] == -1).all() and np.isnan(want[1][p, have:]).all()
        _both(eng, q, qc, r[:nr], rc[:nr], k, 0, e, want)


def test_more_references_than_dtw_assign_takes(eng):
    from adapted_amd import lib
    from adapted_amd.fingerprint import dtw_distances

    r, rc, _ = cc.ragged(4100, 6, 31, unusable=False)
    q, qc, ok = cc.ragged(5, 6, 32)
    with pytest.raises(ValueError):
        dtw_distances(q, qc, r, rc, 0, engine=eng)
    with pytest.raises(lib.HipLibraryError):
        eng.dtw_assign(q, qc, r, rc)
    for band, k in ((0, 5), (2, 32)):
        _both(eng, q, qc, r, rc, k, band, None, ko.topk(_matrix(eng, q, qc, r, rc, band), k))


def test_forced_segments_batches_and_periods_give_the_same_bits(eng, monkeypatch):
    from adapted_amd import lib

    for name in ("ADP_KNN_SEGMENT_REFS", "ADP_KNN_CHECK_PERIOD", "ADP_DTW_SCRATCH_MIB"):
        monkeypatch.delenv(name, raising=False)
    r, rc, _ = cc.ragged(40, 8, 41, unusable=False)
    q, qc, ok = cc.ragged(70, 8, 42)
    ex = np.asarray([p % 40 if p % 3 == 0 else -1 for p in range(70)], dtype=np.int32)
    for band, k in ((0, 3), (1, 32)):
        want = ko.topk(_matrix(eng, q, qc, r, rc, band), k, ex)
        _both(eng, q, qc, r, rc, k, band, ex, want)  # one segment, one batch
        # 6 segments of 7; 40 segments of 1 -- whose lists of 70 queries are more than a budget of 1 MiB holds at k = 32: two batches
        for seg, mib, period in (("7", None, None), ("1", "1", None), ("7", None, "1"), ("39", None, "64"), ("262144", None, "8")):
            for name, value in (("ADP_KNN_SEGMENT_REFS", seg), ("ADP_DTW_SCRATCH_MIB", mib), ("ADP_KNN_CHECK_PERIOD", period)):
                if value is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, value)
            _both(eng, q, qc, r, rc, k, band, ex, want)
    assert 40 * (32 * 12 + 24) * 70 > 1 << 20  # (the batches of the second setting)
    for name, value in (("ADP_KNN_SEGMENT_REFS", "0"), ("ADP_KNN_SEGMENT_REFS", "262145"), ("ADP_KNN_CHECK_PERIOD", "3"),
                        ("ADP_KNN_CHECK_PERIOD", "128"), ("ADP_DTW_SCRATCH_MIB", "0")):
        for other in ("ADP_KNN_SEGMENT_REFS", "ADP_KNN_CHECK_PERIOD", "ADP_DTW_SCRATCH_MIB"):
            monkeypatch.delenv(other, raising=False)
        monkeypatch.setenv(name, value)
        with pytest.raises(lib.HipLibraryError, match=name):
            eng.dtw_knn(q, qc, r, rc, 3)
    for name in ("ADP_KNN_SEGMENT_REFS", "ADP_KNN_CHECK_PERIOD", "ADP_DTW_SCRATCH_MIB"):
        monkeypatch.delenv(name, raising=False)
    _same(eng.dtw_knn(q, qc, r, rc, 32, 1, exclude=ex), want)  # the handle stays usable


@pytest.fixture(scope="module")
def model():
    """the speed tool's model at E = 40: 12 groups x 20 references, 24 queries (member p belongs to group p % 12)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from dtw_cluster_speed import fingerprints
    finally:
        sys.path.pop(0)
    x, c = fingerprints(12 * 20 + 24, 40, 22)
    return x[:240], c[:240], x[240:], c[240:]


def test_pruning_abandons_pairs_and_changes_no_bit(eng, model, monkeypatch):
    r, rc, q, qc = model
    for name in ("ADP_KNN_SEGMENT_REFS", "ADP_KNN_CHECK_PERIOD"):
        monkeypatch.delenv(name, raising=False)
    for k, band in ((1, 0), (5, 0), (5, 6)):
        want = ko.topk(_matrix(eng, q, qc, r, rc, band), k)
        assert (np.arange(240)[want[0][:, 0]] % 12 == np.arange(24) % 12).all()  # (the model is plain: the nearest is of the own group)
        _both(eng, q, qc, r, rc, k, band, None, want)
        pruned = eng.dtw_knn(q, qc, r, rc, k, band, want_work=True)[2]
        full = eng.dtw_knn(q, qc, r, rc, k, band, prune=False, want_work=True)[2]
        assert pruned[:, 1].sum() > 0 and full[:, 1].sum() == 0
        assert np.array_equal(pruned[:, 0] + pruned[:, 1], np.full(24, 240)) and np.array_equal(full[:, 0], np.full(24, 240))
        assert pruned[:, 2].sum() < full[:, 2].sum()
    # adversarial orders: the references of group 0 -- the own group of queries 0 and 12 -- last (their threshold stays loose until
    # the end), and first; several segments too
    k = 5
    base = ko.topk(_matrix(eng, q, qc, r, rc, 0), k)
    own = np.arange(240) % 12 == 0
    for perm in (np.concatenate([np.flatnonzero(~own), np.flatnonzero(own)]), np.concatenate([np.flatnonzero(own), np.flatnonzero(~own)])):
        rp, rcp = np.ascontiguousarray(r[perm]), np.ascontiguousarray(rc[perm])
        want = ko.topk(_matrix(eng, q, qc, rp, rcp, 0), k)
        assert ko.same(want[1], base[1]) and np.array_equal(perm[want[0]], base[0])  # (no ties in this model: the same neighbours)
        for seg in (None, "50"):
            if seg is None:
                monkeypatch.delenv("ADP_KNN_SEGMENT_REFS", raising=False)
            else:
                monkeypatch.setenv("ADP_KNN_SEGMENT_REFS", seg)
            _both(eng, q, qc, rp, rcp, k, 0, None, want)
    monkeypatch.delenv("ADP_KNN_SEGMENT_REFS", raising=False)


def test_device_resident_queries_and_one_engine_for_many_calls(eng, model):
    from adapted_amd.fingerprint import dtw_distances

    r, rc, q, qc = model
    q = q.copy()
    qc = qc.copy()
    qc[3] = 0  # an unusable one among them
    want = ko.topk(_matrix(eng, q, qc, r, rc, 3), 7)
    first_pair = eng.dtw_pairwise(q, qc, 3)
    first_dist = dtw_distances(q, qc, r[:50], rc[:50], 3, engine=eng)
    dq, dqc = eng.dev_alloc(q.nbytes), eng.dev_alloc(qc.nbytes)
    try:
        eng.h2d(dq, q)
        eng.h2d(dqc, qc)
        for _ in range(2):
            _same(eng.dtw_knn(dq, dqc, r, rc, 7, 3, n=q.shape[0], E=q.shape[1]), want)
            assert ko.same(eng.dtw_pairwise(q, qc, 3), first_pair)
            _same(eng.dtw_knn(q, qc, r, rc, 7, 3, prune=False), want)
            assert ko.same(dtw_distances(q, qc, r[:50], rc[:50], 3, engine=eng), first_dist)
            idx, dist, work = eng.dtw_knn(dq, dqc, r, rc, 7, 3, n=q.shape[0], E=q.shape[1], want_work=True)
            _same((idx, dist), want)
            assert (work[3] == 0).all() and (work[:, 0] + work[:, 1] == np.where(np.arange(24) == 3, 0, 240)).all()
    finally:
        eng.dev_free(dq)
        eng.dev_free(dqc)
    with pytest.raises(ValueError):
        eng.dtw_knn(1234, qc, r, rc, 1)  # (device queries without their sizes)


def test_invalid_arguments_are_refused_and_the_handle_stays_usable(eng):
    from adapted_amd import lib

    q, qc, ok = cc.ragged(6, 10, 51)
    r, rc, _ = cc.ragged(8, 10, 52, unusable=False)
    want = ko.topk(_matrix(eng, q, qc, r, rc, 0), 3)
    nan_r = r.copy()
    nan_r[4, rc[4] - 1] = np.nan
    zero_c = rc.copy()
    zero_c[2] = 0
    over_c = rc.copy()
    over_c[2] = 11
    bad_ex = np.full(6, -1, dtype=np.int32)
    bad_ex[5] = 8
    low_ex = np.full(6, -1, dtype=np.int32)
    low_ex[0] = -2
    cases = [(dict(k=0), "k must lie"), (dict(k=33), "k must lie"), (dict(r=np.zeros((0, 10)), rc=np.zeros(0, dtype=np.int32)), "nr must lie"),
             (dict(r=np.zeros((8, 513))), "Er must lie"), (dict(q=np.zeros((6, 513))), "Eq and Er"), (dict(band=-1), "band must be"),
             (dict(rc=zero_c), "r_count"), (dict(rc=over_c), "r_count"), (dict(r=nan_r), "finite"), (dict(ex=bad_ex), "exclude"),
             (dict(ex=low_ex), "exclude")]
    for change, why in cases:
        a = dict(q=q, qc=qc, r=r, rc=rc, k=3, band=0, ex=None)
        a.update(change)
        with pytest.raises(lib.HipLibraryError, match=why):
            eng.dtw_knn(a["q"], a["qc"], a["r"], a["rc"], a["k"], a["band"], exclude=a["ex"])
        _same(eng.dtw_knn(q, qc, r, rc, 3), want)
    nan_r[4, rc[4] - 1] = 0.0
    if rc[4] < 10:
        nan_r[4, rc[4]] = np.nan  # (beyond the count: not read)
        _same(eng.dtw_knn(q, qc, nan_r, rc, 3), ko.topk(_matrix(eng, q, qc, np.where(np.isnan(nan_r), 0.0, nan_r), rc, 0), 3))


def _write(path, ids, fp, counts):
    np.savez(path, read_id=np.asarray(ids), count=counts, status=np.zeros(len(counts), dtype=np.int32),
             lengths=np.zeros(fp.shape, dtype=np.int32), levels=fp, fingerprints=fp)


def test_adapted_knn_on_the_gpu(tmp_path, capsys):
    from adapted_amd import main as cli

    fp, counts, truth = cc.planted(per=35)
    ref = np.sort(np.concatenate([np.flatnonzero(truth == g)[:30] for g in range(4)]))
    qry = np.sort(np.concatenate([np.flatnonzero(truth == g)[30:] for g in range(4)]))
    assert ref.size == 120 and qry.size == 20
    rids, qids = ["ref_%03d" % i for i in range(120)], ["query_%02d" % i for i in range(20)]
    qids[4] = rids[17]  # a read that is also a reference (with another fingerprint here): reference 17 does not vote for it
    rdir, qdir = tmp_path / "refrun" / "fingerprints", tmp_path / "qrun"
    rdir.mkdir(parents=True)
    qdir.mkdir()
    _write(rdir / "fingerprints_0.npz", rids[:50], fp[ref[:50]], counts[ref[:50]])
    _write(rdir / "fingerprints_1.npz", rids[50:], fp[ref[50:]], counts[ref[50:]])
    qfp, qcn = fp[qry].copy(), counts[qry].copy()
    qcn[9] = 0  # not usable
    _write(qdir / "fingerprints_0.npz", qids, qfp, qcn)
    lab = tmp_path / "labels.csv"
    lab.write_text("read_id,barcode\n" + "".join("%s,bc%d\n" % (rids[i], truth[ref[i]]) for i in range(120)))
    out, rep = str(tmp_path / "o.csv"), str(tmp_path / "r.json")
    cli.main(["knn", "-r", str(tmp_path / "refrun"), "-l", str(lab), "-f", str(qdir), "-o", out, "--evaluate", "--report", rep, "-k", "5"])
    text = capsys.readouterr().out
    rfp = np.where(np.isfinite(fp[ref]), fp[ref], 0.0)
    rlab = np.asarray(["bc%d" % truth[p] for p in ref])
    ex = np.full(20, -1)
    ex[4] = 17
    idx, dist = ko.knn(qfp, qcn, rfp, counts[ref], 5, 0, ex)
    want = ko.vote(idx, dist, rlab)
    with open(out) as fh:
        lines = [ln.rstrip("\n").split(",") for ln in fh]
    assert lines[0] == ["read_id", "n_events", "barcode", "votes", "dtw_dist", "barcode_second", "votes_second", "dtw_dist_second", "nearest_read_id"]
    assert len(lines) == 21 and [ln[0] for ln in lines[1:]] == qids
    for p in range(20):
        ln, w = lines[1 + p], want[p]
        if p == 9:
            assert ln[1:] == ["0"] + [""] * 7
            continue
        assert ln[1] == str(qcn[p]) and ln[2] == w[0] == "bc%d" % truth[qry[p]] and int(ln[3]) == w[1] and float(ln[4]) == w[2]
        assert ln[8] == rids[w[6]] and (p != 4 or ln[8] != rids[17])
        assert ln[5:8] == (["", "", ""] if w[3] is None else [w[3], str(w[4]), repr(w[5])])
    names, conf, acc = ko.leave_one_out(fp[ref], counts[ref], rlab, 5, 0)
    import json

    with open(rep) as fh:
        js = json.load(fh)
    assert js["names"] == names == ["bc0", "bc1", "bc2", "bc3"] and js["confusion"] == conf.tolist() and js["accuracy"] == acc == 1.0
    assert js["n"] == 120 and js["k"] == 5 and 0.0 <= js["abandoned_share"] < 1.0
    assert "19 of 20 fingerprints classified" in text and "accuracy = 1.000000" in text
