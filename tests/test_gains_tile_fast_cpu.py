"""The coverage conditions of tests/test_gpu_gains_tile_fast.py's batches, from the CPU oracle's pooled signal alone: which tiles
of k_gains are interior at the "tall" geometry, and where the constant stretches make the fast body's flag rise in some lanes of
an interior tile and not in others."""
import numpy as np
import pytest

import gains_tile_fast_cases as gc
import llr_stream_cases as lc


def test_the_tall_geometry_has_two_interior_tiles_and_the_old_ones_at_most_one():
    g = lc.geom_of(gc.GEOM)
    assert (g.L, g.m) == (4100, 43500)
    assert gc.interior_tiles(g.L, 0, 5, 5) == [1, 2]
    for cand in (0, 500, 1023):
        assert gc.interior_tiles(g.L, cand, 1, 1) == [1, 2, 3]      # (pass 2's offsets are 1 and 1: 3072 + 1024 <= 4098)
    assert gc.interior_tiles(g.L, 1024, 1, 1) == [2, 3]
    # the stage tests' geometries: none in pass 1 but "full"'s tile 1 (1024 + 1024 <= 2111 - 5), and none with two
    assert {nm: gc.interior_tiles(lc.geom_of(nm).L, 0, 5, 5) for nm in lc.GEOMS if nm != gc.GEOM and gc.interior_tiles(lc.geom_of(nm).L, 0, 5, 5)} == {"full": [1]}


@pytest.mark.parametrize("name", ["noise", "prefix", "suffix", "constant", "mixed"])
def test_where_the_flag_rises(oracle_mod, name):
    b = gc.batch(name)
    ref = lc.reference(oracle_mod, b)
    n_cand_low = n_flagged = n_never = 0
    for r, s in enumerate(ref):
        n = s["n_valid"]
        assert n == lc.geom_of(gc.GEOM).L
        vh, vt, vs = gc.variances(s["down"], n, 0)
        ok = gc.log_ok(vh) & gc.log_ok(vt)
        f1, f2 = gc.lanes_flagged(ok, 1), gc.lanes_flagged(ok, 2)
        kind = gc.kind_of(name, r)
        if kind == "noise":       # every lane of both interior tiles clean: committed
            assert gc.log_ok(vs) and not f1.any() and not f2.any()
        elif kind == "prefix":    # the head variance is 0 or below in part of tile 1: some lanes flagged, others not.  (The variance of a
            # constant stretch is rounding noise around 0: for some reads it stays a tiny positive number throughout, and their tile commits.)
            assert gc.log_ok(vs) and not f1.all() and not f2.any() and f1.any() == bool((vh[gc.TILE: gc.PREFIX_END] <= 0).any())
            n_flagged += bool(f1.any())
        elif kind == "suffix":    # the same on the tail variance in tile 2
            assert gc.log_ok(vs) and not f2.all() and not f1.any() and f2.any() == bool((vt[gc.SUFFIX_START: 3 * gc.TILE] <= 0).any())
            n_flagged += bool(f2.any())
        else:                     # a wholly constant read: the whole window's variance is rounding noise around 0 -- where it is 0 or below,
            n_never += not gc.log_ok(vs)   # vs is not finite and the fast body is never entered
        if s["cand"] >= 0 and s["cand"] < 1024:
            n_cand_low += 1
    if name in ("prefix", "suffix"):
        assert n_flagged >= gc.N // 4     # (the sign of the rounding noise is about a coin toss per read)
    if name == "constant":
        assert n_never >= gc.N // 4
    if name == "mixed":
        assert n_flagged >= gc.N // 16
    if name == "noise":
        assert n_cand_low >= 8    # pass 2 meets interior tiles 1 and 2 as well


def test_the_dropped_minibatch(oracle_mod):
    b = gc.batch("dropped")
    ref = lc.reference(oracle_mod, b)
    assert b.minibatch == 32 and all(s is not None for s in ref[:32]) and all(s is None for s in ref[32:])
