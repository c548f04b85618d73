"""One pair gets one distance from every DTW kernel: k_dtw (adp_dtw_assign), k_dtw_pairs (adp_dtw_pairwise), k_dtw_knn (adp_dtw_knn,
pruned and not) and k_dtw_align (adp_dtw_align) all run the wavefront of adapted_amd/csrc/dtw_wave.h, and the cluster oracle, the
lower bounds of k_dtw_knn and the templates code rely on their agreeing in every bit.  No tolerance.  The widths cover the register
tiles C = 1, 1, 2, 4, 8 and the seams between them."""
import numpy as np
import pytest

import fingerprint_oracle as fo

pytestmark = pytest.mark.gpu

ROWS = 9


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def _rows(E, seed):
    """nine finite rows of width E; counts 1, E, E - 1, min(E, 63) and random ones (every count 1 at E = 1)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((ROWS, E))
    cnt = rng.integers(1, E + 1, ROWS).astype(np.int32)
    cnt[:4] = [1, E, max(E - 1, 1), min(E, 63)]
    return X, cnt


@pytest.mark.parametrize("band", [0, 3])
@pytest.mark.parametrize("E", [1, 64, 65, 129, 257])
def test_one_pair_one_distance(eng, E, band):
    X, cnt = _rows(E, 1000 * E + band)
    D = eng.dtw_assign(X, cnt, X, cnt, band)[0]
    assert D.dtype == np.float64 and D.shape == (ROWS, ROWS)
    assert fo.same(D, fo.dtw(X, cnt, X, cnt, band))
    bits = D.view(np.uint64)

    pw = eng.dtw_pairwise(X, cnt, band)
    assert pw.dtype == np.float64 and np.array_equal(pw.view(np.uint64), bits)

    order = np.stack([np.lexsort((np.arange(ROWS), D[p])) for p in range(ROWS)])
    want = np.take_along_axis(D, order, axis=1)
    for prune in (True, False):
        idx, dist = eng.dtw_knn(X, cnt, X, cnt, ROWS, band, prune=prune)
        assert np.array_equal(idx, order), prune
        assert np.array_equal(dist.view(np.uint64), want.view(np.uint64)), prune

    for j in range(ROWS):
        got = eng.dtw_align(X, cnt, np.full(ROWS, j, dtype=np.int32), X, cnt, band, want_path=False)["dist"]
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(D[:, j]).view(np.uint64)), j
