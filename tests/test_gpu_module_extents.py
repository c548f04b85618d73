"""The extent of every host output of the module entry points (adapted_amd/csrc/modules.hip), through the C ABI: each output is an
array 64 elements longer than its documented extent, and the call is made twice on one engine, over outputs filled with 0x00
bytes and with 0xA5 bytes.  The documented extent is byte-equal in both runs (the call wrote all of it) and equal to what the
matching lib.Engine method returns; the 64 elements behind it keep their fill; and with profiling on, the call's launches are the
list written here.  A copy whose byte count disagrees with its piece fails one of the three.

Extents a call leaves as they were, by design, are named where the case is made (`untouched`):
  - adp_llr_trace_bounds' trace without ADP_LLR_INTERP: an input then;
  - adp_normalize's medmad_io with ADP_SS_CLIP: an input then;
  - adp_normalize's rows in device memory (ADP_OUT_DEVICE) behind each read's end: the zeros there are the host form's (`written`).
Outputs that are not passed at all (NULL c_io / c2_io of adp_c_llr_trace, splits_out / stats_out of adp_c_llr_detect, pos_out of
adp_segment_events with cap == 0, lengths / levels / norm of adp_event_levels, dist_out of adp_dtw_assign) have cases of their
own: the other outputs' extents hold without them.  Outputs in device memory (ADP_OUT_DEVICE: adp_normalize, adp_pool_mean,
adp_event_levels' counts and fingerprints, adp_adapter_front's rows) are copied back and held to the same three checks.

Shapes: 3 reads of lengths 0, 131 and L = 256 (adp_c_llr_detect wants len >= 1: 1, 131, 256); 4 segments, one empty; cap 3;
max_events 4; 3 queries against 2 templates, also with ADP_DTW_SCRATCH_MIB=1 -- which holds 65536 such rows, so that call is one
batch; 33 queries against 4096 templates are two batches of it (32 rows of 4096 distances are 1 MiB); 3 rows of m = 400 for the
adapter front, with window 10 / min_obs_adapter 50."""
import ctypes as C

import numpy as np
import pytest

import adapter_front_oracle as O

pytestmark = pytest.mark.gpu

PAD, N, L = 64, 3, 256
LENS = np.array([0, 131, L], dtype=np.int32)
# segments (row, start, end): inside a read, over its end (clipped), empty, a whole row
SEG_ROWS, SEG_STARTS, SEG_ENDS = [1, 2, 1, 2], [8, 100, 50, 0], [120, 400, 50, 256]
NS, CAP, EMAX = 4, 3, 4


@pytest.fixture(scope="module")
def eng():
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    e = lib.Engine(spc, 4, spc.sig_preload_size)
    e.set_profiling(True)
    yield e
    e.close()


def _signal(dtype, n=N, width=L, seed=1):
    """rows of 16-sample steps between 80 and 110 pA with noise of sd 2, multiples of 0.25 pA; two open-pore spikes in row 1"""
    rng = np.random.default_rng(seed)
    x = np.where((np.arange(width) // 16) % 2 == 0, 80.0, 110.0)[None, :] + rng.normal(0.0, 2.0, (n, width))
    x = np.round(x * 4.0) / 4.0
    x[1, 40] = x[1, 90] = 250.0
    return np.ascontiguousarray(x, dtype=dtype)


def _flag64(dtype):
    from adapted_amd import lib

    return lib.ADP_MVS_F64 if np.dtype(dtype) == np.float64 else 0


def _segs():
    from adapted_amd import lib

    s = np.zeros(NS, dtype=lib.SEG_DTYPE)
    s["row"], s["start"], s["end"] = SEG_ROWS, SEG_STARTS, SEG_ENDS
    return s


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _out(shape, dtype, init=None, dev=False):
    """a host output of a documented extent; `init`: what its extent holds before the call (an input / output); `dev`: in device memory"""
    return (shape, np.dtype(dtype), init, dev)


def _extents(eng, name, outs, args_of, want, kernels, untouched=(), written=None):
    """the call `name(handle, *args_of(buffers))` twice, over 0x00 and over 0xA5; want: {key: the Engine method's array};
    written: {key: a mask of the elements the call writes}, for an extent it writes in part by design -- the others keep their fill"""
    written = written or {}
    heads = {k: [] for k in outs}
    for fill in (0x00, 0xA5):
        host, arg, devs = {}, {}, []
        try:
            for k, (shape, dt, init, dev) in outs.items():
                n = int(np.prod(shape))
                host[k] = np.frombuffer(bytes([fill]) * ((n + PAD) * dt.itemsize), dtype=dt).copy()
                if init is not None:
                    host[k][:n] = np.ascontiguousarray(init, dtype=dt).reshape(-1)
                arg[k] = host[k]
                if dev:
                    arg[k] = eng.dev_alloc(host[k].nbytes)
                    devs.append((k, arg[k]))
                    eng.h2d(arg[k], host[k])
            rc = getattr(eng.lib, name)(eng._h, *args_of(arg))
            assert rc == 0, "%s: %d %s" % (name, rc, eng.lib.adp_last_error().decode())
            names = [k for k, _ in eng.kernel_times()]
            for k, p in devs:
                eng.d2h(host[k], p)
        finally:
            for _, p in devs:
                eng.dev_free(p)
        assert names == kernels, (name, names)
        for k, (shape, dt, init, dev) in outs.items():
            n = int(np.prod(shape))
            tail = host[k][n:].tobytes()
            assert tail == bytes([fill]) * len(tail), (name, k, "written behind its extent, fill 0x%02x" % fill)
            heads[k].append(host[k][:n].tobytes())
            if k in untouched:
                was = bytes([fill]) * (n * dt.itemsize) if init is None else _bits(np.ascontiguousarray(init, dtype=dt))
                assert heads[k][-1] == was, (name, k, "is left as it was by design")
    for k in outs:
        if k in untouched:
            continue
        if k in written:
            mask = np.asarray(written[k], dtype=bool).reshape(-1)
            got = [np.frombuffer(h, dtype=outs[k][1]) for h in heads[k]]
            for fill, g in zip((0x00, 0xA5), got):
                assert g[~mask].tobytes() == bytes([fill]) * (g[~mask].nbytes), (name, k, "written where it is left alone by design")
            assert got[0][mask].tobytes() == got[1][mask].tobytes(), (name, k, "part of the extent is not written")
            assert got[0][mask].tobytes() == np.ascontiguousarray(want[k], dtype=outs[k][1]).reshape(-1)[mask].tobytes(), (name, k, "differs from the Engine method")
            continue
        assert heads[k][0] == heads[k][1], (name, k, "part of the extent is not written")
        assert heads[k][0] == _bits(np.ascontiguousarray(want[k], dtype=outs[k][1])), (name, k, "differs from the Engine method")


# ---- adp_c_llr_trace / adp_c_llr_best_split / adp_c_llr_detect ------------------------------------------------------------------
def _trace_args():
    from adapted_amd import lib

    return lib.AdpTraceArgs(5, 5, 2, 1, 300, 100, 0, 50, 10)


_ST, _EN = np.array([0, 10, 20], dtype=np.int32), np.array([0, 120, 250], dtype=np.int32)


@pytest.fixture(scope="module")
def sums(eng):
    """(gains, c, c2) of the float64 signal, from the Engine method"""
    return eng.c_llr_trace(_signal(np.float64), LENS, _ST, _EN, _trace_args(), return_c_c2=True)


@pytest.mark.parametrize("form", ["raw_c", "raw_null_c", "from_sums"])
def test_c_llr_trace(eng, sums, form):
    from adapted_amd import lib

    raw, a = _signal(np.float64), _trace_args()
    _, c, c2 = sums
    if form == "from_sums":
        want = {"gain": eng.c_llr_trace(None, LENS, _ST, _EN, a, sums=(c, c2))}
        _extents(eng, "adp_c_llr_trace", {"gain": _out((N, L), "f8")},
                 lambda b: (None, LENS, _ST, _EN, N, L, C.byref(a), lib.ADP_TRACE_FROM_SUMS, b["gain"], c, c2), want, ["k_trace_gains"])
        return
    outs = {"gain": _out((N, L), "f8")}
    if form == "raw_c":
        outs.update(c=_out((N, L), "f8"), c2=_out((N, L), "f8"))
    w = eng.c_llr_trace(raw, LENS, _ST, _EN, a, return_c_c2=True)
    _extents(eng, "adp_c_llr_trace", outs, lambda b: (raw, LENS, _ST, _EN, N, L, C.byref(a), 0, b["gain"], b.get("c"), b.get("c2")),
             dict(zip(("gain", "c", "c2"), w)), ["k_trace_cumsum", "k_trace_gains"])


def test_c_llr_best_split(eng, sums):
    _, c, c2 = sums
    oh, ot = np.full(N, 7, dtype=np.int32), np.full(N, 5, dtype=np.int32)
    want = dict(zip(("x", "gain"), eng.c_llr_best_split(c, c2, LENS, _ST, _EN, oh, ot)))
    _extents(eng, "adp_c_llr_best_split", {"x": _out((N,), "i8"), "gain": _out((N,), "f8")},
             lambda b: (c, c2, LENS, _ST, _EN, oh, ot, N, L, 0, b["x"], b["gain"]), want, ["k_split_part", "k_split_reduce"])


_SPLITS = ["k_split_part", "k_split_reduce"]


@pytest.mark.parametrize("dtype,polya,details", [(np.float64, True, True), (np.float32, True, True), (np.float32, False, False)],
                         ids=["f64_polya_details", "f32_polya_details", "f32_rows_only"])
def test_c_llr_detect(eng, dtype, polya, details):
    from adapted_amd import lib

    raw, lens = _signal(dtype), np.array([1, 131, L], dtype=np.int32)  # (the call wants len >= 1)
    flags = (lib.ADP_CLLR_F32 if dtype == np.float32 else 0) | (lib.ADP_CLLR_POLYA if polya else 0)
    w = eng.c_llr_detect(raw, lens, 20, 5, 10, polya=polya, details=details)
    outs = {"rows": _out((N, 4), "i8")}
    if details:
        outs.update(splits=_out((N, 4), "i8"), stats=_out((N, 8), "f8"))
    kernels = ["k_trace_cumsum", "k_cd_plan"] + _SPLITS + ["k_cd_plan"] + _SPLITS + ["k_cd_medians"] + (_SPLITS + ["k_cd_finish"] if polya else [])
    _extents(eng, "adp_c_llr_detect", outs, lambda b: (raw, lens, N, L, 20, 5, 10, flags, b["rows"], b.get("splits"), b.get("stats")),
             dict(zip(("rows", "splits", "stats"), w)) if details else {"rows": w}, kernels)


# ---- adp_llr_trace_bounds / adp_llr_trace_peaks / adp_llr_spike_peak ------------------------------------------------------------
@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interp"])
def test_llr_trace_bounds(eng, sums, interp):
    from adapted_amd import lib

    mo, tt = np.full(N, 5, dtype=np.int32), np.full(N, 7, dtype=np.int32)
    tr = sums[0].copy()
    w = eng.llr_trace_bounds(tr, LENS, mo, tt, 2, interp)  # (tr: interpolated in place with `interp`)
    want = dict(zip(("start", "end", "early"), w), trace=tr)
    outs = {"trace": _out((N, L), "f8", init=sums[0]), "start": _out((N,), "i4"), "end": _out((N,), "i4"), "early": _out((N,), "i4")}
    _extents(eng, "adp_llr_trace_bounds", outs,
             lambda b: (b["trace"], LENS, mo, tt, 2, N, L, lib.ADP_LLR_INTERP if interp else 0, b["start"], b["end"], b["early"]),
             want, ["k_trace_bounds"], untouched=() if interp else ("trace",))


def _peak_args():
    from adapted_amd import lib

    return lib.AdpPeakArgs(prominence=0.5, width=2.0, rel_height=0.5, plateau_t=0.9, split_t=0.9, split_prominence=1.0, plateau_on=1,
                           plateau_s=10, plateau_window=50, split_on=1, split_s=10, split_window=50)


def test_llr_trace_peaks(eng, sums):
    tr, a = sums[0], _peak_args()
    want = dict(zip(("peaks", "count"), eng.llr_trace_peaks(tr, LENS, _ST, _EN, a, cap=CAP)))
    _extents(eng, "adp_llr_trace_peaks", {"peaks": _out((N, CAP), "i8"), "count": _out((N,), "i8")},
             lambda b: (tr, LENS, _ST, _EN, N, L, C.byref(a), 0, CAP, b["peaks"], b["count"]), want, ["k_trace_blocksum", "k_trace_peaks"])


def test_llr_spike_peak(eng, sums):
    from adapted_amd import lib

    tr, a = sums[0], lib.AdpSpikeArgs(10.0, 1.0, 10.0, 0.5, 0.99)
    _extents(eng, "adp_llr_spike_peak", {"out": _out((N,), "i8")}, lambda b: (tr, LENS, N, L, C.byref(a), 0, b["out"]),
             {"out": eng.llr_spike_peak(tr, LENS, a)}, ["k_trace_blocksum", "k_trace_spike"])


# ---- adp_mvs_check / adp_mvs_detect_at_loc / adp_mvs_detect --------------------------------------------------------------------
def _mvs_args(streaming=False):
    from adapted_amd.config.schema import MVSPolyAConfig, StreamingConfig
    from adapted_amd.detect import mvs

    return mvs._args(None, StreamingConfig()) if streaming else mvs._args(MVSPolyAConfig(), None, True, True)


DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
_POS = np.array([0, 60, 120], dtype=np.int64), np.array([0, 110, 230], dtype=np.int64)


@DTYPES
def test_mvs_check(eng, dtype):
    sig, a = _signal(dtype), _mvs_args()
    want = dict(zip(("info", "vals"), eng.mvs_check(sig, LENS, _POS[0], _POS[1], a)))
    _extents(eng, "adp_mvs_check", {"info": _out((N, 8), "i4"), "vals": _out((N, 5), "f8")},
             lambda b: (sig, LENS, _POS[0], _POS[1], N, L, C.byref(a), _flag64(dtype), b["info"], b["vals"]), want, ["k_mvs_check"])


@DTYPES
def test_mvs_detect_at_loc(eng, dtype):
    sig, a = _signal(dtype), _mvs_args()
    want = dict(zip(("info", "idx", "vals"), eng.mvs_detect_at_loc(sig, LENS, _POS[0], a)))
    _extents(eng, "adp_mvs_detect_at_loc", {"info": _out((N, 8), "i4"), "idx": _out((N,), "i8"), "vals": _out((N, 5), "f8")},
             lambda b: (sig, LENS, _POS[0], N, L, C.byref(a), _flag64(dtype), b["info"], b["idx"], b["vals"]), want, ["k_mvs_at_loc"])


@DTYPES
def test_mvs_detect(eng, dtype):
    sig, a = _signal(dtype), _mvs_args(True)
    _extents(eng, "adp_mvs_detect", {"out": _out((N,), "i8")}, lambda b: (sig, LENS, N, L, C.byref(a), _flag64(dtype), b["out"]),
             {"out": eng.mvs_detect(sig, LENS, a)}, ["k_mvs_stream"])


# ---- the signal statistics: adp_seg_stats, adp_med_mad, adp_normalize, adp_pool_mean, adp_real_range, adp_open_pores ----------
@DTYPES
def test_seg_stats(eng, dtype):
    sig, segs = _signal(dtype), _segs()
    want = dict(zip(("stats", "count"), eng.seg_stats(sig, LENS, SEG_ROWS, SEG_STARTS, SEG_ENDS)))
    _extents(eng, "adp_seg_stats", {"stats": _out((NS, 4), "f8"), "count": _out((NS,), "i8")},
             lambda b: (sig, LENS, N, L, segs, NS, _flag64(dtype), b["stats"], b["count"]), want, ["k_seg_stats"])


@pytest.mark.parametrize("dtype,whole,regime", [(np.float32, False, None), (np.float64, False, None), (np.float64, True, "wave"),
                                                (np.float32, True, "grid"), (np.float64, True, "grid")],
                         ids=["f32_rows", "f64_rows", "f64_whole_wave", "f32_whole_grid", "f64_whole_grid"])
def test_med_mad(eng, dtype, whole, regime):
    sig = _signal(dtype)
    lens, rows = (None, 1) if whole else (LENS, N)
    flags = _flag64(dtype) | eng._ss_flags(False, whole, regime)
    kernels = ["k_pop_hist", "k_pop_pick"] * (2 * np.dtype(dtype).itemsize) if regime == "grid" else ["k_row_med_mad"]
    _extents(eng, "adp_med_mad", {"out": _out((rows, 2), "f8")}, lambda b: (sig, lens, N, L, flags, b["out"]),
             {"out": eng.med_mad(sig, lens, whole=whole, regime=regime)}, kernels)


@pytest.mark.parametrize("dtype,whole,clip,out_dev", [(np.float32, False, False, False), (np.float64, False, False, True),
                                                      (np.float64, True, False, False), (np.float32, False, True, False),
                                                      (np.float32, True, True, True)],
                         ids=["f32_rows", "f64_rows_out_dev", "f64_whole", "f32_rows_clip", "f32_whole_clip_out_dev"])
def test_normalize(eng, dtype, whole, clip, out_dev):
    from adapted_amd import lib

    sig = _signal(dtype)
    lens, rows = (None, 1) if whole else (LENS, N)
    mm_in = np.tile([95.0, 12.0], (rows, 1)) if clip else None
    flags = _flag64(dtype) | eng._ss_flags(False, whole, None) | (lib.ADP_SS_CLIP if clip else 0) | (lib.ADP_OUT_DEVICE if out_dev else 0)
    want = dict(zip(("out", "medmad", "status"), eng.normalize(sig, lens, 5.0, whole=whole, clip_medmad=mm_in)))
    outs = {"out": _out((N, L), dtype, dev=out_dev), "medmad": _out((rows, 2), "f8", init=mm_in), "status": _out((rows,), "i4")}
    _extents(eng, "adp_normalize", outs, lambda b: (sig, lens, N, L, 5.0, flags, b["medmad"], b["out"], b["status"]), want,
             ([] if clip else ["k_row_med_mad"]) + ["k_clip_scale"], untouched=("medmad",) if clip else (),
             written={"out": np.arange(L)[None, :] < LENS[:, None]} if out_dev and not whole else None)


@pytest.mark.parametrize("dtype,pool,out_dev", [(np.float32, 3, False), (np.float64, 3, True), (np.float64, 200, False), (np.float32, 200, True)],
                         ids=["f32_pool3", "f64_pool3_out_dev", "f64_pool200", "f32_pool200_out_dev"])
def test_pool_mean(eng, dtype, pool, out_dev):
    from adapted_amd import lib

    sig, n_out = _signal(dtype), -(-L // pool)
    flags = _flag64(dtype) | (lib.ADP_OUT_DEVICE if out_dev else 0)
    _extents(eng, "adp_pool_mean", {"out": _out((N, n_out), dtype, dev=out_dev)}, lambda b: (sig, N, L, pool, flags, b["out"]),
             {"out": eng.pool_mean(sig, pool)}, ["k_pool_mean" if pool <= 128 else "k_pool_mean_wave"])


@DTYPES
def test_real_range(eng, dtype):
    from adapted_amd import lib

    sig, segs = _signal(dtype), _segs()
    a = lib.AdpRealRangeArgs((60.0, 130.0), (60.0, 130.0), (5.0, 200.0), 10, 100)
    want = dict(zip(("info", "vals"), eng.real_range(sig, LENS, SEG_ROWS, SEG_STARTS, SEG_ENDS, a)))
    _extents(eng, "adp_real_range", {"info": _out((NS, 2), "i4"), "vals": _out((NS, 3), "f8")},
             lambda b: (sig, LENS, N, L, segs, NS, C.byref(a), _flag64(dtype), b["info"], b["vals"]), want, ["k_real_range"])


@DTYPES
def test_open_pores(eng, dtype):
    sig, segs = _signal(dtype), _segs()
    pos, cnt = eng.open_pores(sig, LENS, SEG_ROWS, SEG_STARTS, SEG_ENDS, 200.0, 300.0, 1.0, cap=CAP)
    assert pos.shape == (NS, CAP) and 1 <= cnt[:, 0].max() <= CAP  # (the spikes of row 1: no list is longer than cap, no repeat)
    _extents(eng, "adp_open_pores", {"pos": _out((NS, CAP), "i8"), "count": _out((NS, 3), "i8")},
             lambda b: (sig, LENS, N, L, segs, NS, 200.0, 300.0, 1.0, _flag64(dtype), CAP, b["pos"], b["count"]),
             {"pos": pos, "count": cnt}, ["k_open_pores"])


# ---- adp_start_peak / adp_adapter_start ---------------------------------------------------------------------------------------------
@DTYPES
def test_start_peak(eng, dtype):
    from adapted_amd import lib

    sig, a = _signal(dtype), lib.AdpStartPeakArgs(200.0, 2, 100, 5, 5)
    full = np.array([0, 131, 4 * L], dtype=np.int32)  # (a full length may exceed the row)
    want = dict(zip(("info", "vals"), eng.start_peak(sig, full, a)))
    _extents(eng, "adp_start_peak", {"info": _out((N, 5), "i4"), "vals": _out((N, 2), "f8")},
             lambda b: (sig, full, N, L, C.byref(a), _flag64(dtype), b["info"], b["vals"]), want, ["k_startpeak_mod"])


@DTYPES
def test_adapter_start(eng, dtype):
    from adapted_amd import lib

    sig, a = _signal(dtype), lib.AdpAdapterStartArgs(5.0, 90.0, 10, 50)
    want = dict(zip(("info", "out", "cand", "diff"), eng.adapter_start(sig, LENS, a)))
    _extents(eng, "adp_adapter_start", {"info": _out((N, 4), "i4"), "out": _out((N,), "i8"), "cand": _out((N,), "i8"), "diff": _out((N,), "f8")},
             lambda b: (sig, LENS, N, L, C.byref(a), _flag64(dtype), b["info"], b["out"], b["cand"], b["diff"]), want, ["k_adapter_start"])


# ---- adp_segment_events / adp_event_levels / adp_dtw_assign -----------------------------------------------------------------------
def _event_args():
    from adapted_amd import lib

    return lib.AdpEventArgs(4.0, 1e-3, 8, 8)


@pytest.mark.parametrize("cap", [CAP, 0], ids=["cap3", "cap0_null_pos"])
@DTYPES
def test_segment_events(eng, dtype, cap):
    sig, segs, a = _signal(dtype), _segs(), _event_args()
    w = eng.segment_events(sig, LENS, SEG_ROWS, SEG_STARTS, SEG_ENDS, a, cap=cap)
    assert w[1][:, 0].max() > CAP  # (more boundaries than cap: the lists are cut, the counts are not)
    outs = {"info": _out((NS, 2), "i8"), "stats": _out((NS, 2), "f8")}
    if cap:
        outs["pos"] = _out((NS, cap), "i8")
    _extents(eng, "adp_segment_events", outs,
             lambda b: (sig, LENS, N, L, segs, NS, C.byref(a), _flag64(dtype), cap, b.get("pos"), b["info"], b["stats"]),
             dict(zip(("pos", "info", "stats"), w)), ["k_ev_scores", "k_ev_bounds"])


@pytest.mark.parametrize("form", ["host", "out_dev", "null_optionals"])
@DTYPES
def test_event_levels(eng, dtype, form):
    from adapted_amd import lib

    sig, segs, a = _signal(dtype), _segs(), _event_args()
    w = eng.event_levels(sig, LENS, SEG_ROWS, SEG_STARTS, SEG_ENDS, a, EMAX)
    dev = form == "out_dev"
    outs = {"info": _out((NS, 2), "i8"), "stats": _out((NS, 2), "f8"), "count": _out((NS,), "i4", dev=dev), "status": _out((NS,), "i4"),
            "fingerprints": _out((NS, EMAX), "f8", dev=dev)}
    if form != "null_optionals":
        outs.update(lengths=_out((NS, EMAX), "i4"), levels=_out((NS, EMAX), "f8"), norm=_out((NS, 2), "f8"))
    flags = _flag64(dtype) | (lib.ADP_OUT_DEVICE if dev else 0)
    _extents(eng, "adp_event_levels", outs,
             lambda b: (sig, LENS, N, L, segs, NS, C.byref(a), flags, EMAX, b["info"], b["stats"], b["count"], b["status"], b.get("lengths"),
                        b.get("levels"), b["fingerprints"], b.get("norm")), w, ["k_ev_scores", "k_ev_bounds", "k_ev_levels"])


def _dtw_in(nq, nt, E, seed):
    rng = np.random.default_rng(seed)
    q, t = rng.normal(0.0, 1.0, (nq, E)), rng.normal(0.0, 1.0, (nt, E))
    qc, tc = rng.integers(0, E + 1, nq).astype(np.int32), rng.integers(1, E + 1, nt).astype(np.int32)
    qc[0] = E
    return q, qc, t, tc


@pytest.mark.parametrize("nq,nt,E,mib,batches,dist", [(3, 2, 4, None, 1, True), (3, 2, 4, 1, 1, True), (3, 2, 4, 1, 1, False), (33, 4096, 2, 1, 2, True)],
                         ids=["3x2", "3x2_1mib", "3x2_1mib_null_dist", "33x4096_1mib_two_batches"])
def test_dtw_assign(eng, monkeypatch, nq, nt, E, mib, batches, dist):
    if mib is not None:
        monkeypatch.setenv("ADP_DTW_SCRATCH_MIB", str(mib))
    q, qc, t, tc = _dtw_in(nq, nt, E, 5)
    want = dict(zip(("dist", "best", "bestdist"), eng.dtw_assign(q, qc, t, tc, band=1, want_dist=dist)))
    outs = {"best": _out((nq, 2), "i4"), "bestdist": _out((nq, 2), "f8")}
    if dist:
        outs["dist"] = _out((nq, nt), "f8")
    _extents(eng, "adp_dtw_assign", outs, lambda b: (q, qc, nq, E, t, tc, nt, E, 1, 0, b.get("dist"), b["best"], b["bestdist"]), want,
             ["k_dtw", "k_dtw_best"] * batches)


# ---- adp_adapter_front / adp_adapter_front_i16 --------------------------------------------------------------------------------------
M = 400
FRONT = O.params(window=10, min_obs_adapter=50, min_shift=5.0, min_pA_current=90.0, min_adapter_len=150)


def _front_in():
    """3 rows of m = 400: a lead of 150 pA before the 80 pA adapter (multiples of 0.25 pA), read 1 ends inside the row -> (sig, full
    lengths, the rows of a detect call)"""
    rng = np.random.default_rng(9)
    sig = np.full((3, M), 80.0)
    sig[0, :120], sig[1, 11:90], sig[2, :60] = 150.0, 150.0, 150.0
    sig = (np.round((sig + rng.normal(0.0, 2.0, sig.shape)) * 4.0) / 4.0).astype(np.float32)
    full = np.array([M, 390, 5 * M], dtype=np.int32)
    sig[1, 390:] = np.nan
    return sig, full, O.make_rows([(0, 380), (11, 350), (None, 300)])


def _front_args():
    from adapted_amd.adapter_front import AdapterFrontParams

    return AdapterFrontParams(FRONT.window, FRONT.min_obs_adapter, FRONT.min_shift, FRONT.min_pA_current, FRONT.min_adapter_len).args()


_FRONT_KERNELS = ["k_adapter_front", "k_seg_stats_sig", "k_adapter_front_patch"]


def _front_outs(rows, rows_dev):
    from adapted_amd import lib

    return {"rows": _out((3,), lib.ROW_DTYPE, init=rows, dev=rows_dev), "info": _out((3, 4), "i4"), "shift": _out((3,), "i8"),
            "cand": _out((3,), "i8"), "diff": _out((3,), "f8")}


@pytest.mark.parametrize("rows_dev", [False, True], ids=["host_rows", "device_rows"])
def test_adapter_front(eng, rows_dev):
    from adapted_amd import lib

    sig, full, rows = _front_in()
    patched = rows.copy()
    want = dict(zip(("info", "shift", "cand", "diff"), eng.adapter_front(sig, None, patched, _front_args(), m=M)), rows=patched)
    assert want["info"][:, 3].any() and patched.tobytes() != rows.tobytes()  # (a row is patched)
    a = _front_args()
    _extents(eng, "adp_adapter_front", _front_outs(rows, rows_dev),
             lambda b: (sig, None, 3, M, b["rows"], C.byref(a), lib.ADP_OUT_DEVICE if rows_dev else 0, b["info"], b["shift"], b["cand"], b["diff"]),
             want, _FRONT_KERNELS)


@pytest.mark.parametrize("rows_dev", [False, True], ids=["host_rows", "device_rows"])
def test_adapter_front_i16(eng, rows_dev):
    from adapted_amd import lib

    sig, full, rows = _front_in()
    scale, offset = np.full(3, 0.25, dtype=np.float32), np.array([-100, 0, 40], dtype=np.float32)
    adc = np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]
    raw = adc.astype(np.int16)
    assert (raw == adc).all()
    d_raw, d_len, d_scale, d_off = eng.dev_alloc(raw.nbytes + 64), eng.dev_alloc(256), eng.dev_alloc(256), eng.dev_alloc(256)
    try:
        for p, x in ((d_raw, raw), (d_len, full), (d_scale, scale), (d_off, offset)):
            eng.h2d(p, x)
        patched, a = rows.copy(), _front_args()
        want = dict(zip(("info", "shift", "cand", "diff"), eng.adapter_front_i16(d_raw, d_len, d_scale, d_off, patched, a, n=3, m=M)), rows=patched)
        assert want["info"][:, 3].any()
        flags = lib.ADP_IN_DEVICE | (lib.ADP_OUT_DEVICE if rows_dev else 0)
        _extents(eng, "adp_adapter_front_i16", _front_outs(rows, rows_dev),
                 lambda b: (d_raw, d_len, d_scale, d_off, 3, M, b["rows"], C.byref(a), flags, b["info"], b["shift"], b["cand"], b["diff"]),
                 want, _FRONT_KERNELS)
    finally:
        for p in (d_raw, d_len, d_scale, d_off):
            eng.dev_free(p)
