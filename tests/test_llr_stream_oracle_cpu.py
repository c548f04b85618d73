"""The numpy restatement of the LLR stream's side outputs (llr_stream_oracle.py) against independent statements of the same
things, and the batches of tests/test_gpu_llr_stream.py (llr_stream_cases.py) against the coverage they were made for -- all with
the CPU oracle alone: what the GPU tests feed the kernels reaches every listed edge."""
import numpy as np
import pytest

import llr_stream_cases as lc
import llr_stream_oracle as so


# ---------------------------------------------------------------- the restatement
def test_maxima_without_a_plateau_is_find_peaks(oracle_mod):
    ref = lc.reference(oracle_mod, lc.batch("pad", "full_wave")) + lc.reference(oracle_mod, lc.seam_batch())
    seen = 0
    for s in ref:
        if s["cand"] < 0:
            continue
        n = s["n_valid"]
        idx, h, plateau = so.maxima(s["g2"], n, n - 2)
        if plateau:
            continue
        x = np.nan_to_num(s["g2"])
        assert idx.tolist() == oracle_mod.find_peaks(x).tolist()
        assert h.tobytes() == x[idx].tobytes()
        seen += 1
    assert seen >= 64


def test_maxima_on_hand_made_rows():
    inf, nan = np.inf, np.nan
    g = np.array([0.0, 1.0, 0.5, 2.0, 2.0, 1.0, nan, -1.0, inf, 3.0, 0.0, 0.0])
    idx, h, plateau = so.maxima(g, g.size, g.size - 2)
    assert idx.tolist() == [1, 8] and h.tolist() == [1.0, so.F64_MAX] and plateau      # (3, 4): a plateau
    idx, _, plateau = so.maxima(np.array([-1.0, 0.0, 0.0, 0.0]), 4, 2)                  # x[1] == 0 < E - ot: a plateau
    assert idx.size == 0 and plateau
    idx, _, plateau = so.maxima(np.array([0.0, -1.0, 0.0, 0.0]), 4, 2)                  # the zeros behind the computed range never peak
    assert idx.size == 0 and not plateau
    assert so.maxima(np.array([1.0, 2.0]), 2, 0)[2] is False
    idx, _, _ = so.maxima(np.array([0.0, 5.0, 1.0, 9.0, 9.5]), 3, 1)                    # only g[:n] counts
    assert idx.tolist() == [1]


def test_checkpoints_restart(oracle_mod):
    rng = np.random.default_rng(5)
    for s in lc.reference(oracle_mod, lc.batch("pad", "edges_mixed")):
        n, down = s["n_valid"], s["down"]
        ck, tail = s["ck"], s["tail"]
        x = down[:n].astype(np.float64)
        c, c2 = np.cumsum(x), np.cumsum(x * x)
        assert ck.shape == ((n + 15) // 16, 2) and ck[0].tolist() == [0.0, 0.0]
        assert np.array_equal(tail, [c[n - 2], c2[n - 2]] if n > 1 else [0.0, 0.0], equal_nan=True)
        for j in sorted(set(rng.integers(1, n + 1, 24).tolist()) | {1, n}):
            q = (j - 1) // 16                           # the checkpoint in front of sample j - 1
            a, b = ck[q]
            for v in x[16 * q: j]:                      # sequential restart, as k_gains does
                a += v
                b += v * v
            assert np.array_equal([a, b], [c[j - 1], c2[j - 1]], equal_nan=True), (n, j)


def test_summaries_on_hand_made_blocks():
    inf, nan = np.inf, np.nan
    g = np.concatenate([np.full(64, nan), np.arange(64.0), np.arange(5.0) - 2.0])
    g[64 + 7] = -inf
    g[64 + 9] = nan
    bmax, bmin = so.summaries(g, g.size, False)
    assert bmax.tolist() == [inf, inf, 2.0] and bmin.tolist() == [inf, -inf, -2.0]   # all NaN; one -inf and one NaN; ragged
    bmax, bmin = so.summaries(g, g.size, True)
    assert bmax.tolist() == [0.0, 63.0, 2.0] and bmin.tolist() == [0.0, -so.F64_MAX, -2.0]
    bmax, bmin = so.summaries(g, 64 + 8, False)                                          # blocks below ceil(n / 64) only
    assert bmax.tolist() == [inf, 7.0 - 1.0] and bmin.tolist() == [inf, -inf]


def test_t1_and_nanstd_sums():
    nan = np.nan
    assert so.t1(np.array([0.0, -1.0, 2.0, nan, 0.0])) == (2, 3)
    assert so.t1(np.array([0.0, -1.0, 0.0])) == (0, 2)
    assert so.nanstd_sums(np.array([1.0, nan, 2.0, 1e-30])) == (1, 3.0, 5.0)
    k, s1, s2 = so.nanstd_sums(np.array([1.0, np.inf, nan, -np.inf]))
    assert k == 1 and np.isnan(s1) and s2 == np.inf


# ---------------------------------------------------------------- the inputs
def test_geometries():
    g = lc.geom_of("pad")
    assert g.ds == 10 and g.L % 64 == 1 and 2048 < g.L < 2112 and g.Lp == 2112
    g = lc.geom_of("full")
    assert g.ds == 10 and g.L == 2112 == g.Lp
    assert lc.geom_of("short").L == 100
    assert [lc.geom_of(k).ds for k in ("ds3", "ds7", "ds32")] == [3, 7, 32]
    for k in lc.GEOMS:
        g = lc.geom_of(k)
        assert g.L == -(-(g.T - g.off) // g.ds) and g.m >= g.T and 512 * g.ds * 4 <= 65536   # (the pooling tile fits 64 KiB of LDS)
    # the scalar path: k_norm_pool vectorises a row only when its segment starts on a 16-byte boundary of the (aligned) matrix
    g = lc.geom_of("scalar")
    assert g.ds == 10 and (g.m % 4 or g.off % 4) and all(lc.scalar_path_rows("scalar", 256))
    assert 0 in lc.scalar_path_rows("pad", 4) and 0 in lc.scalar_path_rows("ds3", 4)    # elsewhere some rows do vectorise


@pytest.mark.parametrize("geom, name, kinds", lc.LAYOUTS)
def test_layouts_reach_their_lengths_and_waves(oracle_mod, geom, name, kinds):
    lc.check_layout(oracle_mod, geom, name, kinds)


def test_all_edge_lengths_are_covered(oracle_mod):
    for geom in ("pad", "full"):
        L = lc.geom_of(geom).L
        for name in ("edges_uniform", "edges_mixed"):
            nv = set(lc.nvalid_of(lc.reference(oracle_mod, lc.batch(geom, name))))
            assert {1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 143, 144, 145, 1023, 1024, 1025, L - 1, L} <= nv, (geom, name)
    nv = set(lc.nvalid_of(lc.reference(oracle_mod, lc.batch("short", "edges_uniform"))))
    assert {1, 2, 15, 16, 17, 31, 32, 33, 99, 100} <= nv


def test_seam_reads(oracle_mod):
    lc.check_seam(oracle_mod)


def test_plateau_reads(oracle_mod):
    lc.check_plateau(oracle_mod)


@pytest.mark.parametrize("geom", ["pad", "full", "ds3", "ds7", "ds32", "scalar"])
def test_d1_batch_ends_around_the_edges(oracle_mod, geom):
    b = lc.d1_batch(geom)
    g = lc.geom_of(geom)
    ends = set((b.lens - g.off).tolist())
    for blk in (lc.NP_TILE, 2, g.L - 1):
        assert {blk * g.ds - 1, blk * g.ds, blk * g.ds + 1} <= ends
    nv = lc.nvalid_of(lc.reference(oracle_mod, b))
    assert {lc.NP_TILE - 1, lc.NP_TILE, g.L - 2, g.L - 1, g.L, 1, 2, 3} <= set(nv)
