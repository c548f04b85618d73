"""What the kernels of the LLR path's phase C hand to each other, fetched buffer by buffer (adp_debug_fetch 13-21) and compared
with the numpy restatement in llr_stream_oracle.py: the checkpoints and tails of k_cumsum / k_cumsum_gather, the per-64-point
summaries, T1 pair and nanstd sums of k_gains<1>, the sanitised summaries and maxima lists of k_gains<2>, and the pooled signal of
k_norm_pool's three load paths.  A failure names the buffer, the read and its length.

The batches come from llr_stream_cases.py, whose coverage conditions tests/test_llr_stream_oracle_cpu.py asserts without a GPU and
which are repeated here.  The truth for n_valid, down, the traces and the indices is the CPU oracle (1e-9 on the traces: the
project's bar, device log against glibc's); everything derived from a trace is taken from the DEVICE's own trace and must then
match bit for bit.  Before every stage the engine runs an unrelated batch of full-length reads through the whole phase, so that
nothing stale passes for a result; only what a kernel defines is compared (ck[q] for q < ceil(n / 16), summary blocks below
ceil(n / 64), nothing of a dropped minibatch's reads)."""
import math
import os

import numpy as np
import pytest

import llr_stream_cases as lc
import llr_stream_oracle as so

pytestmark = pytest.mark.gpu

SWITCHES = ("ADP_CUMSUM_GATHER", "ADP_NP_PREFETCH", "ADP_PK_VALUES", "ADP_PK_PREFIX", "ADP_GROUPS", "ADP_SP_FUSED", "ADP_SERIES_PIPE_LLR", "ADP_N1_S0")
U = 2.0 ** -53


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engine_of():
    """one engine of 256 reads per geometry, shared by the tests of this file"""
    from adapted_amd import lib

    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = lib.Engine(lc.spc_of(geom), 256, lc.geom_of(geom).m, device=0)
        return made[geom]
    yield get
    for e in made.values():
        e.close()


def _run(eng, b, stage, env=None, tails_nan=False):
    """the decoy through the whole phase, then the batch up to `stage`"""
    n = b.lens.size
    dsig, dlen = lc.decoy(b.geom, n)
    _with_env({}, lambda: eng.debug_llr_upto(dsig, dlen, n, n, 7))
    _with_env(env or {}, lambda: eng.debug_llr_upto(b.sig, b.lens, n, b.minibatch, stage, tails_nan=tails_nan))


def _same(a, b):
    """the same bits; a NaN only has to be a NaN (its payload is nobody's input)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes())


def _check_inputs(eng, b, ref):
    """n_valid and down[:n_valid] are the oracle's; the dropped minibatches are the ones meant to be -> n_valid"""
    n = len(ref)
    nv = eng.debug_fetch(1, n)
    assert nv.tolist() == lc.nvalid_of(ref)
    status = eng.debug_fetch(21, -(-n // b.minibatch))
    assert [int(s) != 0 for s in status] == [ref[k] is None for k in range(0, n, b.minibatch)], status
    down = eng.debug_fetch(2, n)
    for r, s in enumerate(ref):
        if s is not None:
            assert _same(down[r, : nv[r]], s["down"]), ("down", r, int(nv[r]))
    return nv


def _check_trace(a, b, what):
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), what
    fin = np.isfinite(b)
    assert np.allclose(a[fin], b[fin], rtol=1e-9, atol=1e-9), (what, float(np.max(np.abs(a[fin] - b[fin]))))


# ---------------------------------------------------------------- a. checkpoints and tails
@pytest.mark.parametrize("geom, name, kinds", lc.LAYOUTS)
def test_checkpoints_and_tails_at_the_edge_lengths(engine_of, oracle_mod, geom, name, kinds):
    """ck[r][q < ceil(n / 16)] and tail[r] are np.cumsum's values bit for bit, from k_cumsum_gather and k_cumsum sharing the launch
    by csum_uniform (the default) and from k_cumsum alone (ADP_CUMSUM_GATHER=0)"""
    b, ref = lc.check_layout(oracle_mod, geom, name, kinds)
    eng, n = engine_of(geom), len(ref)
    for env in ({}, {"ADP_CUMSUM_GATHER": "0"}):
        _run(eng, b, 3, env)
        nv = _check_inputs(eng, b, ref)
        assert lc.wave_kinds(nv, n) == kinds
        ck, tail = eng.debug_fetch(13, n), eng.debug_fetch(14, n)
        for r, s in enumerate(ref):
            if s is None:
                continue
            nq = (s["n_valid"] + so.CK - 1) // so.CK
            if not _same(ck[r, :nq], s["ck"]):
                q = [q for q in range(nq) if not _same(ck[r, q], s["ck"][q])]
                raise AssertionError(("ck", env, "read", r, "n", s["n_valid"], "first bad q", q[0], ck[r, q[0]].tolist(), s["ck"][q[0]].tolist()))
            assert _same(tail[r], s["tail"]), ("tail", env, "read", r, "n", s["n_valid"], tail[r].tolist(), s["tail"].tolist())


# ---------------------------------------------------------------- b. pass 1
def _batch(geom, name):
    return lc.seam_batch() if name == "seam" else lc.plateau_batch() if name == "plateau" else lc.batch(geom, name)


PASS1 = [(g, nm) for g, nm, _ in lc.LAYOUTS] + [("pad", "seam"), ("pad", "plateau")]
PASS2 = [("pad", "seam"), ("pad", "plateau"), ("pad", "edges_mixed"), ("pad", "ragged_long"), ("full", "full_wave"), ("pad", "half_dropped")]


def _check_pass1(eng, b, ref, nv):
    """trace against the oracle's g1; bmax / bmin / T1 / NaN count bit for bit from the device's own trace; the two sums within the
    bound of a float64 sum of N terms in any order (N 2^-53 sum|g|; N + 1 for the squares, which are rounded once more)"""
    n = len(ref)
    g1, t1, gstat = eng.debug_fetch(3, n), eng.debug_fetch(7, n), eng.debug_fetch(17, n)
    bmax, bmin = eng.debug_fetch(15, n), eng.debug_fetch(16, n)
    for r, s in enumerate(ref):
        if s is None:
            continue
        k = s["n_valid"]
        a = g1[r, :k]
        _check_trace(a, s["g1"], ("g1", r, k))
        nb = (k + so.SUMBLK - 1) // so.SUMBLK
        wmax, wmin = so.summaries(a, k, False)
        assert _same(bmax[r, :nb], wmax), ("bmax", r, k, np.flatnonzero(bmax[r, :nb] != wmax)[:4])
        assert _same(bmin[r, :nb], wmin), ("bmin", r, k, np.flatnonzero(bmin[r, :nb] != wmin)[:4])
        assert tuple(int(v) for v in t1[r]) == so.t1(a), ("t1", r, k, t1[r])
        nnan, s1, s2 = so.nanstd_sums(a)
        assert gstat[r, 2] == nnan, ("gstat nan count", r, k, gstat[r, 2], nnan)
        v = a[~np.isnan(a)]
        if np.isfinite(v).all():
            e1 = v.size * U * math.fsum(np.abs(v).tolist())
            e2 = (v.size + 1) * U * s2
            assert abs(gstat[r, 0] - s1) <= e1, ("gstat sum", r, k, gstat[r, 0], s1, e1)
            assert abs(gstat[r, 1] - s2) <= e2, ("gstat sum of squares", r, k, gstat[r, 1], s2, e2)
        else:   # the same non-finite class as np.sum over the non-NaN values
            for got, want in ((gstat[r, 0], s1), (gstat[r, 1], s2)):
                assert (np.isnan(got) and np.isnan(want)) or (np.isinf(got) and got == want), ("gstat class", r, k, got, want)
    return g1, t1, gstat, bmax, bmin


@pytest.mark.parametrize("geom, name", PASS1)
def test_pass1_side_outputs(engine_of, oracle_mod, geom, name):
    b = _batch(geom, name)
    ref = lc.reference(oracle_mod, b)
    eng = engine_of(b.geom)
    _run(eng, b, 4)
    nv = _check_inputs(eng, b, ref)
    if b.name.startswith("edges"):
        assert {11, 12} <= set(nv.tolist()) or lc.geom_of(b.geom).L < 12      # an empty and a one-point computed range
    if b.name == "edges_mixed":                                                # the NaN hole: whole NaN blocks
        s = ref[lc.WAVE - 1]
        assert np.isposinf(so.summaries(s["g1"], s["n_valid"], False)[1]).any()
    _check_pass1(eng, b, ref, nv)


# ---------------------------------------------------------------- c. pass 2
@pytest.mark.parametrize("geom, name", PASS2)
def test_pass2_trace_summaries_and_maxima(engine_of, oracle_mod, geom, name):
    """reads with a candidate: trace against the oracle's g2, sanitised summaries and the list of strict maxima (positions, heights,
    npk; npk = -1 exactly at a plateau) bit for bit from the device's trace, poly(A) index the oracle's -- through k_polya_peak's
    recount for the plateau reads.  Reads without one keep pass 1's trace; T1 and the nanstd sums stay pass 1's for every read."""
    b = _batch(geom, name)
    plateau_reads = ()
    if b.name == "seam":
        ref = lc.check_seam(oracle_mod)
    elif b.name == "plateau":
        ref, plateau_reads = lc.check_plateau(oracle_mod)
    else:
        ref = lc.reference(oracle_mod, b)
    eng, n = engine_of(b.geom), len(ref)
    _run(eng, b, 4)
    nv = _check_inputs(eng, b, ref)
    g1, t1, gstat, bmax1, bmin1 = _check_pass1(eng, b, ref, nv)
    _run(eng, b, 6)
    aidx, g2, t1b, gstatb = eng.debug_fetch(4, n), eng.debug_fetch(3, n), eng.debug_fetch(7, n), eng.debug_fetch(17, n)
    bmax, bmin = eng.debug_fetch(15, n), eng.debug_fetch(16, n)
    npk, pk, pkv = eng.debug_fetch(18, n), eng.debug_fetch(19, n), eng.debug_fetch(20, n)
    n_cand = 0
    for r, s in enumerate(ref):
        if s is None:
            continue
        k = s["n_valid"]
        nb = (k + so.SUMBLK - 1) // so.SUMBLK
        assert int(aidx[r]) == s["cand"], ("adapter_idx", r, k, int(aidx[r]), s["cand"])
        assert t1b[r].tobytes() == t1[r].tobytes() and gstatb[r].tobytes() == gstat[r].tobytes(), ("t1 / gstat changed by pass 2", r, k)
        a = g2[r, :k]
        if s["cand"] < 0:
            assert a.tobytes() == g1[r, :k].tobytes(), ("trace of a read without a candidate", r, k)
            assert bmax[r, :nb].tobytes() == bmax1[r, :nb].tobytes() and bmin[r, :nb].tobytes() == bmin1[r, :nb].tobytes(), ("summaries", r, k)
            continue
        n_cand += 1
        _check_trace(a, s["g2"], ("g2", r, k, s["cand"]))
        wmax, wmin = so.summaries(a, k, True)
        assert _same(bmax[r, :nb], wmax), ("bmax", r, k, s["cand"], np.flatnonzero(bmax[r, :nb] != wmax)[:4])
        assert _same(bmin[r, :nb], wmin), ("bmin", r, k, s["cand"], np.flatnonzero(bmin[r, :nb] != wmin)[:4])
        idx, h, plateau = so.maxima(a, k, k - 2)
        assert (int(npk[r]) == -1) == plateau, ("npk", r, k, s["cand"], int(npk[r]), plateau)
        if not plateau:
            assert int(npk[r]) == idx.size, ("npk", r, k, s["cand"], int(npk[r]), idx.size)
            assert pk[r, : idx.size].tolist() == idx.tolist(), ("pk", r, k, s["cand"], sorted(set(pk[r, : idx.size].tolist()) ^ set(idx.tolist()))[:6])
            assert _same(pkv[r, : idx.size], h), ("pkv", r, k, s["cand"])
    assert n_cand >= 8
    for r in plateau_reads:
        assert int(npk[r]) == -1, ("the oracle's plateau on the device", r)
    _run(eng, b, 7)
    pidx = eng.debug_fetch(5, n)
    for r, s in enumerate(ref):
        if s is not None:
            assert int(pidx[r]) == (max(s["polya_idx"], 0) if s["cand"] >= 0 else 0), ("polya_idx", r, s["n_valid"], int(pidx[r]), s["polya_idx"])


# ---------------------------------------------------------------- d. D1
_PF0 = {"ADP_NP_PREFETCH": "0"}


@pytest.mark.parametrize("geom, env", [("pad", {}), ("pad", _PF0), ("full", {}), ("full", _PF0), ("ds3", {}), ("ds7", {}), ("ds32", {}), ("scalar", {})],
                         ids=lambda v: v if isinstance(v, str) else ("pf0" if v else "default"))
def test_d1_load_paths(engine_of, oracle_mod, geom, env):
    """down[:n_valid] and n_valid bit for bit: the prefetching float4 path (ds = 10), the plain float4 path (ADP_NP_PREFETCH=0, other
    pooling factors), the scalar path (no row's segment on a 16-byte boundary), with and without ADP_TAILS_NAN, for reads that end one
    sample before, at and one sample after a pooled block's and a 512-block tile's edge.  The pooled signal that the start-peak-fused
    kernel leaves behind a whole detect call is the same bytes."""
    b = lc.d1_batch(geom)
    g = lc.geom_of(geom)
    ref = lc.reference(oracle_mod, b)
    eng, n = engine_of(geom), len(ref)
    if geom == "scalar":
        assert (g.m % 4 or g.off % 4) and all(lc.scalar_path_rows(geom, n))
    ends = set((b.lens - g.off).tolist())
    for blk in (lc.NP_TILE, 2, g.L - 1):
        assert {blk * g.ds - 1, blk * g.ds, blk * g.ds + 1} <= ends
    first = None
    for tails_nan in (False, True):
        _run(eng, b, 2, env, tails_nan=tails_nan)
        _check_inputs(eng, b, ref)
        down = eng.debug_fetch(2, n)[:, : g.L]
        if first is None:
            first = down
        assert _same(down, first), "ADP_TAILS_NAN changes the pooled signal"
    if g.ds == 10 and g.off % g.ds == 0 and not env:
        dsig, dlen = lc.decoy(geom, n)
        eng.debug_llr_upto(dsig, dlen, n, n, 7)
        rows, mbs = _with_env({}, lambda: eng.detect_llr_rows(b.sig, b.lens, n, n, with_start_peak=True))
        assert (mbs == 0).all()
        assert eng.debug_fetch(2, n)[:, : g.L].tobytes() == first.tobytes(), "the start-peak-fused pooling pass leaves another pooled signal"


# ---------------------------------------------------------------- the selectors themselves
def test_a_fetch_beyond_a_buffer_is_refused():
    """every stream selector copies at most its buffer: one read more than the call's workspace holds is ADP_ERR_INVALID, and a handle
    made without the maxima's heights (ADP_PK_VALUES=0) says so instead of copying from nothing"""
    from adapted_amd import lib

    b = lc.batch("short", "ragged_short")
    n = 8
    for env in ({}, {"ADP_PK_VALUES": "0"}):
        def run():
            eng = lib.Engine(lc.spc_of("short"), n, lc.geom_of("short").m, device=0)
            try:
                eng.debug_llr_upto(b.sig[:n], b.lens[:n], n, n, 7)
                for what in (13, 14, 15, 16, 17, 18, 19) + (() if env else (20,)):
                    assert eng.debug_fetch(what, n).shape[0] == n
                    with pytest.raises(lib.HipLibraryError):
                        eng.debug_fetch(what, n + 1)
                if env:
                    with pytest.raises(lib.HipLibraryError):
                        eng.debug_fetch(20, n)
                assert eng.debug_fetch(21, 1).tolist() == [0]
                with pytest.raises(lib.HipLibraryError):
                    eng.debug_fetch(21, 2)
            finally:
                eng.close()
        _with_env(env, run)
