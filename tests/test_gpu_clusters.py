"""adp_dtw_pairwise, adp_kmedoids_build, adp_kmedoids and adp_silhouette (include/adapted_hip_clusters.h; kernels:
adapted_amd/csrc/dtw_cluster_api.h) on the GPU: the pairwise matrix against adp_dtw_assign's -- dtw_distances(q, q) -- and the three
calls on a matrix against their numpy oracle (tests/dtw_cluster_oracle.py), every output bit for bit, no tolerance: every rounding
and every tie is specified.  The planted set through discover_clusters equals the oracle's result in every field."""
import os

import numpy as np
import pytest

import clusters_cases as cc
import dtw_cluster_oracle as co

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def _reference(eng, q, qc, ok, band):
    """dtw_distances(q, q) of the usable rows (adp_dtw_assign refuses unusable TEMPLATES), NaN rows and columns for the others"""
    from adapted_amd.fingerprint import dtw_distances

    n = q.shape[0]
    want = np.full((n, n), np.nan)
    good = np.flatnonzero(ok)
    if good.size:
        want[np.ix_(good, good)] = dtw_distances(q[good], qc[good], q[good], qc[good], band, engine=eng)
    return want


def _exact(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    assert co.same(got, want), int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())
    assert co.same(got, np.ascontiguousarray(got.T))  # symmetric to the bit
    d = np.diag(got)
    assert not np.signbit(d[~np.isnan(d)]).any() and (d[~np.isnan(d)] == 0.0).all()  # a +0.0 diagonal


@pytest.mark.parametrize("E", [1, 2, 64, 65, 110, 512])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130])
def test_pairwise_is_dtw_assign_bit_for_bit(eng, n, E):
    q, qc, ok = cc.ragged(n, E, 1000 * n + E)
    if n >= 5:
        assert (~ok).sum() == 4 and qc.min() == 0 and qc.max() == E + 1
    assert n == 1 or qc[1] == 1  # ragged down to 1
    for band in (0, 1, 5):
        want = _reference(eng, q, qc, ok, band)
        if ok.all():  # (then adp_dtw_assign takes q as its templates: the whole matrix from one call)
            from adapted_amd.fingerprint import dtw_distances

            assert co.same(want, dtw_distances(q, qc, q, qc, band, engine=eng))
        _exact(eng.dtw_pairwise(q, qc, band), want)


def _through_device(eng, q, qc, band, dev_in, dev_out):
    n, E = q.shape
    ptrs = []
    try:
        a, b = q, qc
        if dev_in:
            a, b = eng.dev_alloc(q.nbytes), eng.dev_alloc(qc.nbytes)
            ptrs += [a, b]
            eng.h2d(a, q)
            eng.h2d(b, qc)
        if not dev_out:
            return eng.dtw_pairwise(a, b, band, n=n, E=E)
        out = eng.dev_alloc(n * n * 8)
        ptrs.append(out)
        assert eng.dtw_pairwise(a, b, band, n=n, E=E, out_ptr=out) is None
        got = np.full((n, n), -1.0)
        eng.d2h(got, out)
        return got
    finally:
        for p in ptrs:
            eng.dev_free(p)


def test_pairwise_host_and_device_inputs_and_outputs_and_two_budgets(eng, monkeypatch):
    # n = 400: 400 * 400 * 8 bytes are more than the least budget, 1 MiB: a host matrix then comes in two bands of rows
    for n, E, band in ((65, 110, 0), (130, 65, 5), (400, 8, 2)):
        q, qc, ok = cc.ragged(n, E, 7 * n + E)
        want = _reference(eng, q, qc, ok, band)
        for budget in (None, "1"):
            if budget is None:
                monkeypatch.delenv("ADP_DTW_SCRATCH_MIB", raising=False)
            else:
                monkeypatch.setenv("ADP_DTW_SCRATCH_MIB", budget)
            for dev_in in (False, True):
                for dev_out in (False, True):
                    _exact(_through_device(eng, q, qc, band, dev_in, dev_out), want)
    monkeypatch.delenv("ADP_DTW_SCRATCH_MIB", raising=False)


def test_pairwise_module_function_and_refusals(eng):
    from adapted_amd import clusters, lib

    q, qc, ok = cc.ragged(20, 12, 3)
    want = _reference(eng, q, qc, ok, 0)
    _exact(clusters.dtw_pairwise(q, qc, engine=eng), want)
    m = clusters.dtw_pairwise(q, qc, engine=eng, out_device=True)
    try:
        got = np.zeros((20, 20))
        eng.d2h(got, m.ptr)
        _exact(got, want)
    finally:
        m.free()
    out = np.zeros((20, 20))
    for args in ((q, qc, 0, 12, 0, 0, out), (q, qc, 20, 0, 0, 0, out), (q, qc, 20, 513, 0, 0, out), (q, qc, 16385, 12, 0, 0, out),
                 (q, qc, 20, 12, -1, 0, out), (None, qc, 20, 12, 0, 0, out), (q, qc, 20, 12, 0, 0, None)):
        assert eng.lib.adp_dtw_pairwise(eng._h, *args) == -1
    with pytest.raises(lib.HipLibraryError):
        eng.dtw_pairwise(q, qc, -1)
    _exact(eng.dtw_pairwise(q, qc, 0), want)  # the handle is still usable


def _matrices(n):
    out = [("points", cc.points_matrix(n, 40 + n))]
    if n in (2, 65):
        out.append(("equal", np.full((n, n), 2.5) - np.diag(np.full(n, 2.5))))
        out.append(("zero", np.zeros((n, n))))
    return out


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 130, 200])
def test_build_kmedoids_and_silhouette_are_the_oracle_bit_for_bit(eng, n, on_device):
    for name, D in _matrices(n):
        ptr = None
        try:
            dist = D
            if on_device:
                dist = ptr = eng.dev_alloc(D.nbytes)
                eng.h2d(ptr, D)
            full, gain = co.build(D, n)
            for K in sorted({k for k in (1, 2, 3, 64, 65, n) if k <= n}):
                med, g = eng.kmedoids_build(dist, K, n=n)
                assert med.dtype == np.int32 and med.tolist() == full[:K].tolist() and co.same(g, gain[:K]), (name, K)
                for max_iter in (0, 1, 50):
                    if on_device and max_iter == 1:
                        continue
                    # (BUILD's medoids, and a bad start that makes the updates work: the first K rows)
                    for start in (med, np.arange(K, dtype=np.int32)):
                        want = co.kmedoids(D, start, max_iter)
                        got = eng.kmedoids(dist, start, max_iter, n=n, want_sums=True)
                        assert got["iters"] == want["iters"] <= max_iter and got["medoids"].tolist() == want["medoids"].tolist(), (name, K, max_iter)
                        assert got["assign"].tolist() == want["assign"].tolist() and co.same(got["cost"], want["cost"]), (name, K, max_iter)
                        assert co.same(got["sums"], want["sums"]), (name, K, max_iter)
                        assert np.bincount(got["assign"], minlength=K).min() >= 1
                        nosums = eng.kmedoids(dist, start, max_iter, n=n)
                        assert nosums["sums"] is None and nosums["assign"].tolist() == want["assign"].tolist() and co.same(nosums["cost"], want["cost"])
                    assert co.same(eng.silhouette(dist, want["assign"], K, n=n), co.silhouette(D, want["assign"], K)), (name, K)
        finally:
            if ptr is not None:
                eng.dev_free(ptr)


def test_the_cost_series_does_not_increase(eng):
    # (integer coordinates: every sum is exact, so PAM's argument holds to the bit; tests/test_clusters_cpu.py has the oracle's side)
    for seed in range(3):
        D = cc.points_matrix(200, seed, integer=True)
        r = eng.kmedoids(D, np.arange(7, dtype=np.int32), 50)
        assert r["iters"] >= 1 and r["cost"].size == r["iters"] + 1 and (np.diff(r["cost"]) <= 0).all()
        assert co.same(r["cost"], co.kmedoids(D, np.arange(7), 50)["cost"])


def test_refusals_leave_the_handle_usable(eng):
    from adapted_amd import lib

    D = cc.points_matrix(30, 2)
    med, gain = co.build(D, 4)
    assign = co.kmedoids(D, med, 5)["assign"]
    for bad in (np.nan, -1.0, np.inf):
        B = D.copy()
        B[17, 29] = bad  # (the last column of a row: every thread of the check sees its own part)
        ptr = eng.dev_alloc(B.nbytes)
        try:
            eng.h2d(ptr, B)
            for dist in (B, ptr):
                for call in (lambda: eng.kmedoids_build(dist, 4, n=30), lambda: eng.kmedoids(dist, med, 5, n=30),
                             lambda: eng.silhouette(dist, assign, 4, n=30)):
                    with pytest.raises(lib.HipLibraryError, match="NaN, a negative value or an infinity"):
                        call()
        finally:
            eng.dev_free(ptr)
    wrong = assign.copy()
    wrong[3] = 4
    low = assign.copy()
    low[3] = -1
    empty = np.where(assign == 3, 0, assign).astype(np.int32)
    for a, why in ((wrong, "assign < k"), (low, "assign < k"), (empty, "without a member")):
        with pytest.raises(lib.HipLibraryError, match=why):
            eng.silhouette(D, a, 4)
    with pytest.raises(lib.HipLibraryError):
        eng.silhouette(D, assign, 0)
    with pytest.raises(lib.HipLibraryError):
        eng.silhouette(D, np.zeros(30, dtype=np.int32), 31)
    for k in (0, 31):
        with pytest.raises(lib.HipLibraryError):
            eng.kmedoids_build(D, k)
    for start in ([0, 0], [0, 30], [-1, 2], list(range(30)) + [0]):
        with pytest.raises(lib.HipLibraryError):
            eng.kmedoids(D, start, 5)
    with pytest.raises(lib.HipLibraryError):
        eng.kmedoids(D, med, -1)
    got, g = eng.kmedoids_build(D, 4)
    assert got.tolist() == med.tolist() and co.same(g, gain)
    assert co.same(eng.silhouette(D, assign, 4), co.silhouette(D, assign, 4))


def test_the_planted_set_through_discover_clusters_is_the_oracles(eng):
    from adapted_amd import clusters

    fp, counts, truth = cc.planted()
    want_t, want = clusters.discover_clusters(fp, counts, (2, 8), engine=co.OracleEngine())
    got_t, got = clusters.discover_clusters(fp, counts, (2, 8), engine=eng)
    assert got["k"] == want["k"] == 4 and cc.same_partition(got["assign"], truth)
    assert sorted(got) == sorted(want)
    for key in want:
        if key != "k":
            assert co.same(np.asarray(got[key]), np.asarray(want[key])), key
    assert got_t.names == want_t.names and co.same(got_t.levels, want_t.levels) and got_t.counts.tolist() == want_t.counts.tolist()
    # a sample, a band and a single K, the default engine of the device
    want_t, want = clusters.discover_clusters(fp, counts, 3, sample=50, band=6, engine=co.OracleEngine())
    got_t, got = clusters.discover_clusters(fp, counts, 3, sample=50, band=6, device=0)
    for key in want:
        assert co.same(np.asarray(got[key]), np.asarray(want[key])), key
    assert co.same(got_t.levels, want_t.levels)
    assert os.environ.get("ADP_DTW_SCRATCH_MIB") is None
