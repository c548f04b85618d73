"""k_gains' fast body for interior tiles (llr_stream.h, ADP_GAINS_TILE_FAST): at a geometry whose reads have interior tiles
(gains_tile_fast_cases.py) every case runs with the switch at 1 and at 0.  Each run: the traces against the CPU oracle at 1e-9, the
derived buffers against llr_stream_oracle's restatement from the device's own trace; between the two runs everything bit for bit
(traces, bmax / bmin, gstat, T1, npk / pk / pkv, poly(A) index, the final rows).  The two tallies (debug counters 76 / 77: tiles
committed by the fast body, tiles run again by the plain one) say which path a case took."""
import os

import numpy as np
import pytest

import gains_tile_fast_cases as gc
import llr_stream_cases as lc
import llr_stream_oracle as so
import test_gpu_llr_stream as ts

pytestmark = pytest.mark.gpu

SWITCH = "ADP_GAINS_TILE_FAST"


def _with_switch(value, fn):
    old = os.environ.get(SWITCH)
    try:
        os.environ.pop(SWITCH, None)
        if value is not None:
            os.environ[SWITCH] = value
        return ts._with_env({}, fn)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


@pytest.fixture(scope="module")
def engine():
    from adapted_amd import lib

    eng = lib.Engine(lc.spc_of(gc.GEOM), gc.N, lc.geom_of(gc.GEOM).m, device=0)
    yield eng
    eng.close()


def _tallies(eng):
    c = eng.debug_counters(80)
    return int(c[76]), int(c[77])


def _run_case(eng, b, ref):
    """-> everything compared between the switch settings, and the tallies of pass 1 and of both passes"""
    n = len(ref)
    out = {}
    dsig, dlen = lc.decoy(gc.GEOM, n)
    eng.debug_llr_upto(dsig, dlen, n, n, 7)
    t0 = _tallies(eng)
    eng.debug_llr_upto(b.sig, b.lens, n, b.minibatch, 4)
    t1 = _tallies(eng)
    nv = ts._check_inputs(eng, b, ref)
    out["pass1"] = ts._check_pass1(eng, b, ref, nv)
    eng.debug_llr_upto(dsig, dlen, n, n, 7)
    t2 = _tallies(eng)
    eng.debug_llr_upto(b.sig, b.lens, n, b.minibatch, 6)
    t3 = _tallies(eng)
    aidx, g2 = eng.debug_fetch(4, n), eng.debug_fetch(3, n)
    bmax, bmin = eng.debug_fetch(15, n), eng.debug_fetch(16, n)
    npk, pk, pkv = eng.debug_fetch(18, n), eng.debug_fetch(19, n), eng.debug_fetch(20, n)
    keep = []
    for r, s in enumerate(ref):
        if s is None:
            continue
        k = s["n_valid"]
        nb = (k + so.SUMBLK - 1) // so.SUMBLK
        assert int(aidx[r]) == s["cand"], ("adapter_idx", r, int(aidx[r]), s["cand"])
        a = g2[r, :k]
        keep.append((a.copy(), bmax[r, :nb].copy(), bmin[r, :nb].copy(), int(npk[r])))
        if s["cand"] < 0:
            continue
        ts._check_trace(a, s["g2"], ("g2", r, k, s["cand"]))
        wmax, wmin = so.summaries(a, k, True)
        assert ts._same(bmax[r, :nb], wmax), ("bmax", r, s["cand"], np.flatnonzero(bmax[r, :nb] != wmax)[:4])
        assert ts._same(bmin[r, :nb], wmin), ("bmin", r, s["cand"], np.flatnonzero(bmin[r, :nb] != wmin)[:4])
        idx, h, plateau = so.maxima(a, k, k - 2)
        assert (int(npk[r]) == -1) == plateau, ("npk", r, s["cand"], int(npk[r]), plateau)
        if not plateau:
            assert int(npk[r]) == idx.size and pk[r, : idx.size].tolist() == idx.tolist(), ("pk", r, s["cand"])
            assert ts._same(pkv[r, : idx.size], h), ("pkv", r, s["cand"])
            keep.append((pk[r, : idx.size].copy(), pkv[r, : idx.size].copy()))
    out["pass2"] = keep
    eng.debug_llr_upto(b.sig, b.lens, n, b.minibatch, 7)
    pidx = eng.debug_fetch(5, n)
    for r, s in enumerate(ref):
        if s is not None:
            assert int(pidx[r]) == (max(s["polya_idx"], 0) if s["cand"] >= 0 else 0), ("polya_idx", r, int(pidx[r]), s["polya_idx"])
    out["polya"] = [int(pidx[r]) for r, s in enumerate(ref) if s is not None]
    rows, mbs = eng.detect_llr_rows(b.sig, b.lens, n, b.minibatch, with_start_peak=True)
    out["rows"] = (rows.tobytes(), mbs.tobytes())
    p1 = (t1[0] - t0[0], t1[1] - t0[1])
    both = (t3[0] - t2[0], t3[1] - t2[1])
    return out, p1, both


def _flat(x):
    if isinstance(x, (tuple, list)):
        return [v for y in x for v in _flat(y)]
    return [x]


@pytest.mark.parametrize("name", gc.NAMES)
def test_fast_body_and_plain_body_agree(engine, oracle_mod, name):
    b = gc.batch(name)
    ref = lc.reference(oracle_mod, b)
    on, p1_on, both_on = _with_switch(None, lambda: _run_case(engine, b, ref))
    off, p1_off, both_off = _with_switch("0", lambda: _run_case(engine, b, ref))
    print("tallies (committed, redone) %-9s pass 1 %s  both passes %s  switch off %s %s" % (name, p1_on, both_on, p1_off, both_off))
    assert p1_off == (0, 0) and both_off == (0, 0)
    n_live = sum(s is not None for s in ref)
    n_in = len(gc.reads_entering(ref))    # reads with a finite vs: both interior tiles of pass 1 go to the fast body first
    assert sum(p1_on) == 2 * n_in, (p1_on, n_in, n_live)
    if name in ("noise", "dropped"):      # every interior tile committed, in pass 2 as well
        assert n_in == n_live and p1_on[1] == 0 and both_on[1] == 0 and both_on[0] > p1_on[0]
    elif name in ("prefix", "suffix"):    # one of the two interior tiles is redone in pass 1 (for the reads test_gains_tile_fast_cpu.py counts)
        assert n_in == n_live and p1_on[0] >= n_live and p1_on[1] >= 1 and both_on[1] >= p1_on[1]
    elif name == "constant":              # vs is not finite for the reads whose variance is 0 or below: never entered
        assert n_in < n_live
    else:                                 # a workgroup's four reads: noise, prefix, suffix, constant
        assert 3 * (n_live // 4) <= n_in < n_live and p1_on[1] >= 1
    a, c = _flat([on["pass1"], on["pass2"], on["polya"], on["rows"]]), _flat([off["pass1"], off["pass2"], off["polya"], off["rows"]])
    assert len(a) == len(c)
    for k, (x, y) in enumerate(zip(a, c)):
        same = (x.shape == y.shape and x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y
        assert same, ("the two switch settings differ", name, k)
