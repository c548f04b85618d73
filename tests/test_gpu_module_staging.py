"""Every staging branch of the module entry points (include/adapted_hip.h: adp_c_llr_*, adp_llr_trace_*, adp_llr_spike_peak,
adp_mvs_*) through the C ABI: device inputs (ADP_IN_DEVICE) and device outputs (ADP_OUT_DEVICE) give the same bits as the host
forms the other module tests pin against the reference.  Then one engine that alternates the families with shrinking and
growing batches: every result equals the same call on a fresh engine (nothing of one call's workspace reaches the next)."""
import ctypes as C

import numpy as np
import pytest

import mvs_module_cases as M

pytestmark = pytest.mark.gpu


def _ptr(a):
    return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class _Mem:
    """the arrays of one call form: host arrays as they are, or (dev) device copies of them; freed together"""

    def __init__(self, eng):
        self.eng, self.bufs = eng, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.eng.dev_free(p)

    def on(self, a, dev):
        a = np.ascontiguousarray(a)
        if not dev:
            return a
        p = self.eng.dev_alloc(max(a.nbytes, 256))
        self.bufs.append(p)
        self.eng.h2d(p, a)
        return p

    def back(self, x, like):
        if not isinstance(x, int):
            return x
        out = np.empty_like(like)
        self.eng.d2h(out, x)
        return out


def _call(eng, name, *args):
    rc = getattr(eng.lib, name)(eng._h, *args)
    assert rc == 0, "%s: %d %s" % (name, rc, eng.lib.adp_last_error().decode())


def _engine():
    from adapted_amd.detect import _c_llr

    return _c_llr._engine()


def _fresh():
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    return lib.Engine(spc, 1, spc.sig_preload_size)


def _reads(n, L, seed, dtype=np.float64):
    """n synthetic reads (adapted_amd/synth.py) of lengths in [L // 4, L], zero-padded to [n, L], with NaN holes and constant runs"""
    from adapted_amd.synth import synth_read

    rng = np.random.default_rng(seed)
    lens = rng.integers(max(1, L // 4), L + 1, n).astype(np.int32)
    lens[0] = L
    x = np.zeros((n, L), dtype=dtype)
    for r in range(n):
        m = int(lens[r])
        y = synth_read(seed, r, m, m).astype(np.float64)
        if r % 4 == 1:
            y[int(rng.integers(0, m))] = np.nan
        elif r % 4 == 2 and m > 20:
            a = int(rng.integers(0, m // 2))
            y[a: a + m // 3] = y[a]
        x[r, :m] = y
    return x, lens


def _ranges(lens, seed):
    rng = np.random.default_rng(seed)
    st = np.array([int(rng.integers(0, max(1, ln // 8))) for ln in lens.tolist()], dtype=np.int32)
    en = np.array([ln - int(rng.integers(0, max(1, ln // 8))) for ln in lens.tolist()], dtype=np.int32)
    return st, np.maximum(en, st)


# ---- adp_c_llr_trace ----------------------------------------------------------------------------------------------------------
def _trace_args(stride=2, early_stopping=1):
    from adapted_amd import lib

    return lib.AdpTraceArgs(5, 5, stride, early_stopping, 300, 100, 0, 50, 10)


def _c_llr_trace(eng, raw, lens, st, en, in_dev, out_dev, with_c=True, sums=None, args=None):
    """-> (gain, c, c2) as host arrays (c, c2 None when they are not outputs)"""
    from adapted_amd import lib

    n, L = (raw if sums is None else sums[0]).shape
    nan = np.full((n, L), np.nan)
    flags = (lib.ADP_IN_DEVICE if in_dev else 0) | (lib.ADP_OUT_DEVICE if out_dev else 0)
    with _Mem(eng) as m:
        g = m.on(nan.copy(), out_dev)
        if sums is None:
            rp = m.on(raw, in_dev)
            c, c2 = (m.on(nan.copy(), out_dev), m.on(nan.copy(), out_dev)) if with_c else (None, None)
        else:
            flags |= lib.ADP_TRACE_FROM_SUMS
            rp, c, c2 = None, m.on(sums[0], in_dev), m.on(sums[1], in_dev)
        _call(eng, "adp_c_llr_trace", _ptr(rp), _ptr(lens), _ptr(st), _ptr(en), int(n), int(L), C.byref(args or _trace_args()), flags,
              _ptr(g), _ptr(c), _ptr(c2))
        out = m.back(g, nan)
        if sums is None and with_c:
            return out, m.back(c, nan), m.back(c2, nan)
        return out, None, None


@pytest.fixture(scope="module")
def trace_in():
    raw, lens = _reads(12, 9000, 3)
    st, en = _ranges(lens, 4)
    return raw, lens, st, en


@pytest.mark.parametrize("with_c", [True, False], ids=["c_out", "c_null"])
@pytest.mark.parametrize("out_dev", [False, True], ids=["out_host", "out_dev"])
@pytest.mark.parametrize("in_dev", [False, True], ids=["in_host", "in_dev"])
def test_c_llr_trace_raw(trace_in, in_dev, out_dev, with_c):
    eng = _engine()
    raw, lens, st, en = trace_in
    g0, c0, c20 = _c_llr_trace(eng, raw, lens, st, en, False, False)
    assert (g0 != 0).any() and np.isfinite(c0).any()
    g, c, c2 = _c_llr_trace(eng, raw, lens, st, en, in_dev, out_dev, with_c=with_c)
    assert _bits(g) == _bits(g0)
    if with_c:
        assert _bits(c) == _bits(c0) and _bits(c2) == _bits(c20)


@pytest.mark.parametrize("out_dev", [False, True], ids=["out_host", "out_dev"])
@pytest.mark.parametrize("in_dev", [False, True], ids=["in_host", "in_dev"])
def test_c_llr_trace_from_sums(trace_in, in_dev, out_dev):
    eng = _engine()
    raw, lens, st, en = trace_in
    g0, c0, c20 = _c_llr_trace(eng, raw, lens, st, en, False, False)
    g, _, _ = _c_llr_trace(eng, None, lens, st, en, in_dev, out_dev, sums=(c0, c20))
    assert _bits(g) == _bits(g0)


# ---- adp_c_llr_best_split / adp_c_llr_detect ------------------------------------------------------------------------------------
def _best_split(eng, c, c2, lens, st, en, oh, ot, in_dev):
    from adapted_amd import lib

    n, L = c.shape
    x = np.zeros(n, dtype=np.int64)
    g = np.zeros(n)
    with _Mem(eng) as m:
        _call(eng, "adp_c_llr_best_split", _ptr(m.on(c, in_dev)), _ptr(m.on(c2, in_dev)), *(_ptr(a) for a in (lens, st, en, oh, ot)),
              int(n), int(L), lib.ADP_IN_DEVICE if in_dev else 0, _ptr(x), _ptr(g))
    return x, g


def test_c_llr_best_split_host_and_device_sums(trace_in):
    eng = _engine()
    raw, lens, st, en = trace_in
    _, c, c2 = _c_llr_trace(eng, raw, lens, st, en, False, False)
    oh = np.full(lens.size, 40, dtype=np.int32)
    ot = np.full(lens.size, 25, dtype=np.int32)
    x0, g0 = _best_split(eng, c, c2, lens, st, en, oh, ot, False)
    assert (x0 >= 0).any()
    x1, g1 = _best_split(eng, c, c2, lens, st, en, oh, ot, True)
    assert _bits(x1) == _bits(x0) and _bits(g1) == _bits(g0)


def _c_llr_detect(eng, raw, lens, in_dev, details, polya=True):
    from adapted_amd import lib

    n, L = raw.shape
    flags = (lib.ADP_IN_DEVICE if in_dev else 0) | (lib.ADP_CLLR_F32 if raw.dtype == np.float32 else 0) | (lib.ADP_CLLR_POLYA if polya else 0)
    rows = np.zeros((n, 4), dtype=np.int64)
    splits = np.zeros((n, 4), dtype=np.int64) if details else None
    stats = np.zeros((n, 8)) if details else None
    with _Mem(eng) as m:
        _call(eng, "adp_c_llr_detect", _ptr(m.on(raw, in_dev)), _ptr(lens), int(n), int(L), 500, 50, 100, flags, _ptr(rows),
              _ptr(splits), _ptr(stats))
    return rows, splits, stats


@pytest.mark.parametrize("details", [True, False], ids=["details", "rows_only"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_c_llr_detect_host_and_device(dtype, details):
    eng = _engine()
    raw, lens = _reads(16, 12000, 5, dtype)
    r0, s0, t0 = _c_llr_detect(eng, raw, lens, False, True)
    assert (r0[:, 1] > 0).any()
    r1, s1, t1 = _c_llr_detect(eng, raw, lens, True, details)
    assert _bits(r1) == _bits(r0)
    if details:
        assert _bits(s1) == _bits(s0) and _bits(t1) == _bits(t0)
    r2, _, _ = _c_llr_detect(eng, raw, lens, False, details)
    assert _bits(r2) == _bits(r0)


# ---- adp_llr_trace_bounds / adp_llr_trace_peaks / adp_llr_spike_peak ------------------------------------------------------------
@pytest.fixture(scope="module")
def traces(trace_in):
    """(smooth traces: stride 1, no early stop; strided ones with an early stop; lens), a NaN run inside read 1"""
    raw, lens, st, en = trace_in
    g1, _, _ = _c_llr_trace(_engine(), raw, lens, st, en, False, False, args=_trace_args(1, 0))
    g2, _, _ = _c_llr_trace(_engine(), raw, lens, st, en, False, False)
    for g in (g1, g2):
        g[1, lens[1] // 2: lens[1] // 2 + 40] = np.nan
    return g1, g2, lens


def _bounds(eng, tr, lens, in_dev, interp):
    """-> (start, end, early_stop, the trace after the call)"""
    from adapted_amd import lib

    n, L = tr.shape
    mo = np.full(n, 5, dtype=np.int32)
    tt = np.full(n, 7, dtype=np.int32)
    out = [np.zeros(n, dtype=np.int32) for _ in range(3)]
    flags = (lib.ADP_IN_DEVICE if in_dev else 0) | (lib.ADP_LLR_INTERP if interp else 0)
    with _Mem(eng) as m:
        t = m.on(tr.copy(), in_dev)
        _call(eng, "adp_llr_trace_bounds", _ptr(t), _ptr(lens), _ptr(mo), _ptr(tt), 4, int(n), int(L), flags, *(_ptr(a) for a in out))
        return out + [m.back(t, tr)]


@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interp"])
def test_llr_trace_bounds_host_and_device(traces, interp):
    eng = _engine()
    _, g, lens = traces
    h = _bounds(eng, g, lens, False, interp)
    d = _bounds(eng, g, lens, True, interp)
    for a, b in zip(h, d):
        assert _bits(a) == _bits(b)
    assert (_bits(h[3]) != _bits(g)) == interp


def _peak_args():
    from adapted_amd import lib

    return lib.AdpPeakArgs(prominence=0.5, width=20.0, rel_height=0.5, plateau_t=0.9, split_t=0.9, split_prominence=1.0, plateau_on=1,
                           plateau_s=10, plateau_window=500, split_on=1, split_s=10, split_window=500)


def _peaks(eng, tr, lens, lo, hi, in_dev, given, cap=8):
    from adapted_amd import lib

    n, L = tr.shape
    pk = np.zeros((n, cap), dtype=np.int64)
    cnt = np.zeros(n, dtype=np.int64)
    flags = (lib.ADP_IN_DEVICE if in_dev else 0) | (lib.ADP_LLR_GIVEN_PEAK if given else 0)
    with _Mem(eng) as m:
        _call(eng, "adp_llr_trace_peaks", _ptr(m.on(tr, in_dev)), _ptr(lens), _ptr(lo), _ptr(hi), int(n), int(L), C.byref(_peak_args()),
              flags, int(cap), _ptr(pk), _ptr(cnt))
    return pk, cnt


@pytest.mark.parametrize("given", [False, True], ids=["find", "given_peak"])
def test_llr_trace_peaks_host_and_device(traces, given):
    eng = _engine()
    g, _, lens = traces
    lo, hi = _ranges(lens, 6)
    if given:
        lo = np.minimum(lo + 100, lens - 1).astype(np.int32)
    p0, c0 = _peaks(eng, g, lens, lo, hi, False, given)
    assert (c0 > 0).any()
    p1, c1 = _peaks(eng, g, lens, lo, hi, True, given)
    assert _bits(p1) == _bits(p0) and _bits(c1) == _bits(c0)


def _spike(eng, tr, lens, in_dev):
    from adapted_amd import lib

    n, L = tr.shape
    out = np.zeros(n, dtype=np.int64)
    with _Mem(eng) as m:
        _call(eng, "adp_llr_spike_peak", _ptr(m.on(tr, in_dev)), _ptr(lens), int(n), int(L), C.byref(lib.AdpSpikeArgs(10.0, 1.0, 10.0, 0.5, 0.99)),
              lib.ADP_IN_DEVICE if in_dev else 0, _ptr(out))
    return out


def test_llr_spike_peak_host_and_device(traces):
    eng = _engine()
    g, _, lens = traces
    assert _bits(_spike(eng, g, lens, True)) == _bits(_spike(eng, g, lens, False))


# ---- adp_mvs_check / adp_mvs_detect_at_loc / adp_mvs_detect --------------------------------------------------------------------
def _mvs_in(n, seed, dtype):
    rng = np.random.default_rng(seed)
    rows, pos = [], []
    for r in range(n):
        ln = int(rng.integers(5000, 12000))
        x, a, p = M.pa_read(int(rng.integers(1 << 30)), ln, decoys=r % 3, nan_at=(int(rng.integers(0, ln)),) if r % 5 == 1 else ())
        rows.append(x.astype(dtype))
        pos.append((a + int(rng.integers(-30, 30)), p + int(rng.integers(-30, 30)), a + int(rng.integers(-60, 60))))
    X = np.zeros((n, max(r.size for r in rows)), dtype=dtype)
    for i, r in enumerate(rows):
        X[i, :r.size] = r
    return X, np.array([r.size for r in rows], dtype=np.int32), np.maximum(np.array(pos, dtype=np.int64), 0)


def _mvs_args(streaming=False):
    from adapted_amd.config.schema import MVSPolyAConfig, StreamingConfig
    from adapted_amd.detect import mvs

    return mvs._args(None, StreamingConfig()) if streaming else mvs._args(MVSPolyAConfig(), None, True, True)


def _mvs(eng, which, X, lens, pos, in_dev):
    from adapted_amd import lib

    n, L = X.shape
    flags = (lib.ADP_IN_DEVICE if in_dev else 0) | (lib.ADP_MVS_F64 if X.dtype == np.float64 else 0)
    with _Mem(eng) as m:
        sp = _ptr(m.on(X, in_dev))
        if which == "check":
            info, vals = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 5))
            ae, pe = np.ascontiguousarray(pos[:, 0]), np.ascontiguousarray(pos[:, 1])
            _call(eng, "adp_mvs_check", sp, _ptr(lens), _ptr(ae), _ptr(pe), int(n), int(L), C.byref(_mvs_args()), flags, _ptr(info), _ptr(vals))
            return info, vals
        if which == "at_loc":
            info, idx, vals = np.zeros((n, 8), dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros((n, 5))
            loc = np.ascontiguousarray(pos[:, 2])
            _call(eng, "adp_mvs_detect_at_loc", sp, _ptr(lens), _ptr(loc), int(n), int(L), C.byref(_mvs_args()), flags, _ptr(info),
                  _ptr(idx), _ptr(vals))
            return info, idx, vals
        out = np.zeros(n, dtype=np.int64)
        _call(eng, "adp_mvs_detect", sp, _ptr(lens), int(n), int(L), C.byref(_mvs_args(True)), flags, _ptr(out))
        return (out,)


@pytest.mark.parametrize("which", ["check", "at_loc", "detect"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_mvs_host_and_device(which, dtype):
    eng = _engine()
    X, lens, pos = _mvs_in(24, 7, dtype)
    h = _mvs(eng, which, X, lens, pos, False)
    assert any((a != 0).any() for a in h)
    d = _mvs(eng, which, X, lens, pos, True)
    for a, b in zip(h, d):
        assert _bits(a) == _bits(b)


# ---- one engine, the families in turn ----------------------------------------------------------------------------------------
def test_alternating_families_equal_fresh_engines():
    """large and small batches of every family in turn on one engine, host and device forms mixed: every result is the one a
    fresh engine gives for the same call"""
    big_raw, big_lens = _reads(48, 40000, 21)
    sm_raw, sm_lens = _reads(6, 3000, 22, np.float32)
    tr_raw, tr_lens = _reads(10, 15000, 23)
    tr_st, tr_en = _ranges(tr_lens, 24)
    mX, mlens, mpos = _mvs_in(3, 25, np.float32)
    MX, Mlens, Mpos = _mvs_in(40, 26, np.float64)
    g, c, c2 = _c_llr_trace(_engine(), tr_raw, tr_lens, tr_st, tr_en, False, False, args=_trace_args(1, 0))
    lo, hi = _ranges(tr_lens, 27)
    steps = [
        lambda e: _c_llr_detect(e, big_raw, big_lens, False, True),
        lambda e: _mvs(e, "check", mX, mlens, mpos, False),
        lambda e: _peaks(e, g, tr_lens, lo, hi, True, False),
        lambda e: _c_llr_trace(e, None, tr_lens, tr_st, tr_en, False, False, sums=(c, c2)),
        lambda e: _mvs(e, "detect", MX, Mlens, Mpos, True),
        lambda e: _c_llr_detect(e, sm_raw, sm_lens, True, False, polya=False),
        lambda e: _bounds(e, g, tr_lens, False, True),
        lambda e: _mvs(e, "at_loc", MX, Mlens, Mpos, False),
        lambda e: _c_llr_trace(e, big_raw, big_lens, *_ranges(big_lens, 28), True, False),
        lambda e: _spike(e, g, tr_lens, False),
        lambda e: _best_split(e, c, c2, tr_lens, tr_st, tr_en, np.full(10, 30, np.int32), np.full(10, 30, np.int32), True),
        lambda e: _mvs(e, "check", mX, mlens, mpos, True),
    ]
    eng = _fresh()
    try:
        got = [step(eng) for step in steps]
    finally:
        eng.close()
    for i, step in enumerate(steps):
        one = _fresh()
        try:
            want = step(one)
        finally:
            one.close()
        got_i = got[i] if isinstance(got[i], (tuple, list)) else (got[i],)
        want = want if isinstance(want, (tuple, list)) else (want,)
        assert len(got_i) == len(want)
        for a, b in zip(got_i, want):
            assert (a is None) == (b is None), i
            if a is not None:
                assert _bits(a) == _bits(b), i
