"""What reaches the library from every Python entry of the CNN primary (and from Engine's four detect methods), without a GPU: a
bare lib.Engine whose ``lib`` is a recorder (tests/call_recorder.py).  For each entry: the function called, n, m, the minibatch,
the flag word -- spelled out here from include/adapted_hip.h's meaning of each bit --, whether the rows go in as host arrays or as
pointers, and whether the predictions are asked for.  And every refusal of a host-side form, with its message."""
import copy

import numpy as np
import pytest

from call_recorder import detect_calls, head_kind, names, recorder_engine

N, M = 5, 32
DSIG, DLEN, DRAW, DSCALE, DOFF = 10000, 20000, 30000, 40000, 50000


@pytest.fixture(scope="module")
def ctx():
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.detect import cnn

    spc = get_chemistry_specific_config("RNA004")
    assert spc.cnn_boundaries.fallback_to_llr_short_reads
    return dict(spc=spc, k=max(1, int(spc.cnn_boundaries.polya_cand_k)), weights=cnn.load_cnn_weights(spc.cnn_boundaries.model_name),
                sig=np.arange(N * M, dtype=np.float32).reshape(N, M), lens=np.full(N, 100, dtype=np.int32))


def _flags():
    from adapted_amd import lib

    return dict(IN=lib.ADP_IN_DEVICE, OUT=lib.ADP_OUT_DEVICE, SP=lib.ADP_WITH_START_PEAK, NAN=lib.ADP_TAILS_NAN, FB=lib.ADP_CNN_FALLBACK,
                LLR2=lib.ADP_CNN_SECOND_LLR, TRUNC=lib.ADP_FLAG_TRUNCATED)


def test_the_flag_bits_are_the_headers():
    f = _flags()
    assert f == dict(IN=1, OUT=2, SP=4, NAN=32, FB=1 << 17, LLR2=1 << 18, TRUNC=1 << 19)


# (entry, keywords, the flags expected beside ADP_CNN_FALLBACK): the host-batch entries take (eng, sig, lens, model, spc, **kw), the
# resident ones (eng, dsig, dlen, n, lens_host, model, spc, **kw)
_OPTION_ROWS = [
    ("detect_rows", {}, ()),
    ("detect_rows_start_peak", {}, ("SP",)),
    ("detect_rows_truncated", {}, ("TRUNC",)),
    ("detect_rows_truncated", {"with_start_peak": True}, ("TRUNC", "SP")),
    ("detect_rows_second_opinion", {}, ("LLR2",)),
    ("detect_rows_second_opinion", {"with_start_peak": True}, ("LLR2", "SP")),
    ("detect_rows_second_opinion", {"flag_truncated": True}, ("LLR2", "TRUNC")),
    ("detect_rows_second_opinion", {"second_opinion": False}, ()),
    ("detect_rows_second_opinion", {"second_opinion": False, "flag_truncated": True, "with_start_peak": True}, ("TRUNC", "SP")),
]


@pytest.mark.parametrize("entry,kw,bits", _OPTION_ROWS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else None)
def test_host_batch_entries(ctx, entry, kw, bits):
    from adapted_amd.detect import cnn

    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    rows = getattr(cnn, entry)(eng, ctx["sig"], ctx["lens"], ctx["weights"], ctx["spc"], **kw)
    assert rows.shape == (N,) and names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn"]
    (c,) = detect_calls(eng)
    assert head_kind(c) == "host" and np.array_equal(c["head"][0], ctx["sig"])
    assert (c["n"], c["m"], c["minibatch"], c["rows"], c["bounds"]) == (N, M, N, "host", None)
    assert c["flags"] == f["FB"] | sum(f[b] for b in bits)
    getattr(cnn, entry)(eng, ctx["sig"], ctx["lens"], ctx["weights"], ctx["spc"], **kw)
    assert names(eng)[2:] == ["adp_detect_cnn"], "the weights are handed over once per model"


@pytest.mark.parametrize("minibatch", [None, 2])
@pytest.mark.parametrize("entry,kw,bits", _OPTION_ROWS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else None)
def test_resident_entries(ctx, entry, kw, bits, minibatch):
    from adapted_amd.detect import cnn

    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    fn = getattr(cnn, entry.replace("detect_rows", "detect_rows_device"))
    rows = fn(eng, DSIG, DLEN, N, ctx["lens"], ctx["weights"], ctx["spc"], minibatch, **kw)
    assert rows.shape == (N,) and names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn"]
    (c,) = detect_calls(eng)
    assert head_kind(c) == "pointers" and c["head"] == (DSIG, DLEN)
    assert (c["n"], c["m"], c["minibatch"], c["rows"], c["bounds"]) == (N, M, minibatch or N, "host", None)
    assert c["flags"] == f["IN"] | f["FB"] | sum(f[b] for b in bits)


@pytest.mark.parametrize("kw,bits", [({}, ()), ({"with_start_peak": True}, ("SP",)), ({"second_opinion": True}, ("LLR2",)),
                                     ({"with_start_peak": True, "second_opinion": True, "minibatch": 2}, ("SP", "LLR2"))])
def test_resident_int16_entry(ctx, kw, bits):
    from adapted_amd.detect import cnn

    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    rows = cnn.detect_rows_device_i16(eng, DRAW, DLEN, DSCALE, DOFF, N, ctx["lens"], ctx["weights"], ctx["spc"], **kw)
    assert rows.shape == (N,) and names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn_i16"]
    (c,) = detect_calls(eng)
    assert head_kind(c) == "pointers" and c["head"] == (DRAW, DLEN, DSCALE, DOFF)
    assert (c["n"], c["m"], c["minibatch"], c["rows"], c["bounds"]) == (N, M, kw.get("minibatch") or N, "host", None)
    assert c["flags"] == f["IN"] | f["FB"] | sum(f[b] for b in bits)


def test_host_applied_fallback_of_a_host_batch(ctx):
    """detect_rows(..., "hip", "host"): the rows in front of the fallback and the predictions, then the fallback's own calls on
    the selected reads' samples"""
    from adapted_amd.detect import cnn

    eng = recorder_engine(ctx["spc"], M)
    cnn.detect_rows(eng, ctx["sig"], ctx["lens"], ctx["weights"], ctx["spc"], "hip", "host")
    assert names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn"], "all-zero predictions select nobody"
    (c,) = detect_calls(eng)
    assert head_kind(c) == "host" and c["flags"] == 0 and (c["n"], c["minibatch"]) == (N, N)
    assert c["bounds"] == (np.dtype(np.int64), (N, 1 + ctx["k"]))

    eng = recorder_engine(ctx["spc"], M, bounds=(3000, 9000))  # failed rows, short reads, a long poly(A) range: every read is selected
    lens = ctx["lens"].copy()
    lens[3] = 2 * ctx["spc"].core.max_obs_adapter  # ... but this one is not short
    cnn.detect_rows(eng, ctx["sig"], lens, ctx["weights"], ctx["spc"], "hip", "host")
    assert names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn", "adp_llr_refine_polya"]
    _, sub, sub_lens, n, m, ranges, flags, _, _ = eng.lib.calls[-1][1]
    assert (n, m, flags) == (4, M, 0) and np.array_equal(sub, ctx["sig"][[0, 1, 2, 4]]) and sub_lens.tolist() == [100] * 4
    assert ranges.tolist() == [[3000, 9000]] * 4


def test_host_applied_fallback_of_a_resident_batch(ctx):
    """detect_rows_device(..., fallback="host"): one copy back per selected read, from its row of the resident matrix"""
    from adapted_amd import lib
    from adapted_amd.detect import cnn

    eng = recorder_engine(ctx["spc"], M, bounds=(3000, 9000))
    lens = ctx["lens"].copy()
    lens[0] = 2 * ctx["spc"].core.max_obs_adapter
    cnn.detect_rows_device(eng, DSIG, DLEN, N, lens, ctx["weights"], ctx["spc"], 2, "host")
    assert names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn"] + ["adp_memcpy_d2h"] * 4 + ["adp_llr_refine_polya"]
    (c,) = detect_calls(eng)
    assert head_kind(c) == "pointers" and c["flags"] == lib.ADP_IN_DEVICE and (c["n"], c["minibatch"]) == (N, 2)
    assert c["bounds"] == (np.dtype(np.int64), (N, 1 + ctx["k"]))
    copies = [a for name, a in eng.lib.calls if name == "adp_memcpy_d2h"]
    assert [(a[2], a[3]) for a in copies] == [(DSIG + i * M * 4, M * 4) for i in (1, 2, 3, 4)]
    assert eng.lib.calls[-1][1][3] == 4 and eng.lib.calls[-1][1][2].tolist() == [100] * 4


def test_only_the_host_batch_entries_look_at_polya_cand_k(ctx):
    from adapted_amd.detect import cnn

    spc = copy.deepcopy(ctx["spc"])
    spc.cnn_boundaries.polya_cand_k = 0
    for entry in ("detect_rows", "detect_rows_start_peak", "detect_rows_truncated", "detect_rows_second_opinion"):
        eng = recorder_engine(spc, M)
        with pytest.raises(ValueError, match="polya_cand_k must be >= 1"):
            getattr(cnn, entry)(eng, ctx["sig"], ctx["lens"], ctx["weights"], spc)
        assert names(eng) == []
        getattr(cnn, entry.replace("detect_rows", "detect_rows_device"))(eng, DSIG, DLEN, N, ctx["lens"], ctx["weights"], spc)
        assert names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn"]
    eng = recorder_engine(spc, M)
    cnn.detect_rows_device_i16(eng, DRAW, DLEN, DSCALE, DOFF, N, ctx["lens"], ctx["weights"], spc)
    assert names(eng) == ["adp_cnn_set_weights", "adp_detect_cnn_i16"]


@pytest.mark.parametrize("n", [0, 1, N])
@pytest.mark.parametrize("kw,bits", [({}, ()), ({"flag_truncated": True}, ("TRUNC",)), ({"with_start_peak": True}, ("SP",)),
                                     ({"flag_truncated": True, "with_start_peak": True}, ("TRUNC", "SP"))])
def test_combined_detect_cnn_and_cnn_llr(ctx, monkeypatch, n, kw, bits):
    from adapted_amd.container_types import DetectResults
    from adapted_amd.detect import cnn, combined

    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    asked = []
    monkeypatch.setattr(combined, "get_engine", lambda spc, n, m, device=0: asked.append((n, m, device)) or eng)
    sig, lens = ctx["sig"][:n], ctx["lens"][:n]
    if n == 0:  # goes to the engine as it is; no result to unwrap
        with pytest.raises(IndexError):
            cnn.combined_detect_cnn(sig, lens, ctx["weights"], ctx["spc"], **kw)
    else:
        res = cnn.combined_detect_cnn(sig, lens, ctx["weights"], ctx["spc"], **kw)
        assert isinstance(res, DetectResults) if n == 1 else (isinstance(res, list) and len(res) == n)
    (c,) = detect_calls(eng)
    assert asked == [(n, M, 0)] and head_kind(c) == "host" and (c["n"], c["minibatch"], c["bounds"]) == (n, n, None)
    assert c["flags"] == f["FB"] | sum(f[b] for b in bits)

    del eng.lib.calls[:], asked[:]
    res = cnn.combined_detect_cnn_llr(sig, lens, ctx["weights"], ctx["spc"], **kw)
    assert isinstance(res, list) and len(res) == n
    if n == 0:
        assert asked == [] and names(eng) == []
    else:
        (c,) = detect_calls(eng)
        assert head_kind(c) == "host" and (c["n"], c["minibatch"], c["bounds"]) == (n, n, None)
        assert c["flags"] == f["FB"] | f["LLR2"] | sum(f[b] for b in bits)


def _bare_pipeline(ctx, eng, **attrs):
    from adapted_amd import pipeline

    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.primary, p.with_start_peak, p.second_opinion, p.flag_truncated = "cnn", False, None, False
    p.native_i16 = p.ragged = p.i16 = False
    p.model, p.spc, p.eng = ctx["weights"], ctx["spc"], eng
    p.mb, p.N, p.m, p.dsig16 = 2, 8, M, None
    p.slots = [{"ds": 1000, "dl": 2000, "dcal": 3000, "do": 4000, "lens": np.arange(8, dtype=np.int32)}]
    for k, v in attrs.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("attrs,bits", [({}, ()), ({"with_start_peak": True}, ("SP",)), ({"second_opinion": "llr"}, ("LLR2",)),
                                        ({"flag_truncated": True}, ("TRUNC",)),
                                        ({"with_start_peak": True, "second_opinion": "llr", "flag_truncated": True}, ("SP", "LLR2", "TRUNC"))])
def test_pipeline_detect_with_the_cnn_primary(ctx, attrs, bits):
    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    rows, mbs = _bare_pipeline(ctx, eng, **attrs)._detect(0, N)
    assert rows.shape == (N,) and mbs is None
    assert names(eng) == ["adp_copy_wait", "adp_cnn_set_weights", "adp_detect_cnn"] and eng.lib.calls[0][1][1] == 0
    (c,) = detect_calls(eng)
    assert c["head"] == (1000, 2000) and (c["n"], c["m"], c["minibatch"], c["rows"], c["bounds"]) == (N, M, 2, "host", None)
    assert c["flags"] == f["IN"] | f["FB"] | sum(f[b] for b in bits)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("attrs,bits", [({}, ()), ({"with_start_peak": True, "second_opinion": "llr"}, ("SP", "LLR2"))])
def test_pipeline_detect_on_the_native_int16_plan(ctx, attrs, bits, ragged):
    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    p = _bare_pipeline(ctx, eng, native_i16=True, i16=True, ragged=ragged, dsig16=7000 if ragged else None, **attrs)
    rows, mbs = p._detect(0, N)
    assert rows.shape == (N,) and mbs is None
    assert names(eng) == ["adp_copy_wait"] + (["adp_expand_ragged_i16"] if ragged else []) + ["adp_cnn_set_weights", "adp_detect_cnn_i16"]
    if ragged:
        assert eng.lib.calls[1][1][1:] == (1000, 4000, 2000, N, M, 7000)
    (c,) = detect_calls(eng)
    assert c["head"] == (7000 if ragged else 1000, 2000, 3000, 3000 + 8 * 4)
    assert (c["n"], c["m"], c["minibatch"], c["rows"], c["bounds"]) == (N, M, 2, "host", None)
    assert c["flags"] == f["IN"] | f["FB"] | sum(f[b] for b in bits)


def test_engine_detect_llr_rows_keywords(ctx):
    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    for kw, want in (({}, 0), ({"with_start_peak": True}, f["SP"]), ({"tails_nan": True}, f["NAN"]), ({"flag_truncated": True}, f["TRUNC"]),
                     ({"with_start_peak": True, "tails_nan": True, "flag_truncated": True}, f["SP"] | f["NAN"] | f["TRUNC"])):
        for ptrs in (False, True):
            for rows_dev in (None, 6000):
                del eng.lib.calls[:]
                head = (DSIG, DLEN) if ptrs else (ctx["sig"], ctx["lens"])
                rows, mbs = eng.detect_llr_rows(*head, N, 2, device_ptrs=ptrs, rows_dev=rows_dev, **kw)
                (c,) = detect_calls(eng)
                assert c["fn"] == "adp_detect_llr" and head_kind(c) == ("pointers" if ptrs else "host")
                assert (c["n"], c["m"], c["minibatch"]) == (N, M, 2) and c["bounds"] == (np.dtype(np.int32), (3,))
                assert c["flags"] == want | (f["IN"] if ptrs else 0) | (f["OUT"] if rows_dev else 0), (kw, ptrs, rows_dev)
                assert (rows is None and c["rows"] == 6000) if rows_dev else (rows.shape == (N,) and c["rows"] == "host")
                assert mbs.shape == (3,) and mbs.dtype == np.int32


def test_engine_detect_llr_rows_i16_keywords(ctx):
    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    for sp in (False, True):
        for rows_dev in (None, 6000):
            del eng.lib.calls[:]
            rows, mbs = eng.detect_llr_rows_i16(DRAW, DLEN, DSCALE, DOFF, N, 2, with_start_peak=sp, rows_dev=rows_dev)
            (c,) = detect_calls(eng)
            assert c["fn"] == "adp_detect_llr_i16" and c["head"] == (DRAW, DLEN, DSCALE, DOFF)
            assert (c["n"], c["m"], c["minibatch"]) == (N, M, 2) and c["bounds"] == (np.dtype(np.int32), (3,))
            assert c["flags"] == f["IN"] | (f["SP"] if sp else 0) | (f["OUT"] if rows_dev else 0)
            assert (rows is None and c["rows"] == 6000) if rows_dev else (rows.shape == (N,) and c["rows"] == "host")


_CNN_KW = [({}, ()), ({"fallback": True}, ("FB",)), ({"second_opinion": True}, ("LLR2",)), ({"with_start_peak": True}, ("SP",)),
           ({"fallback": True, "second_opinion": True, "with_start_peak": True}, ("FB", "LLR2", "SP"))]


def test_engine_detect_cnn_rows_keywords(ctx):
    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    for kw, bits in _CNN_KW + [({"flag_truncated": True}, ("TRUNC",)), ({"flag_truncated": True, "fallback": True}, ("TRUNC", "FB"))]:
        for ptrs in (False, True):
            for rows_dev in (None, 6000):
                for want_bounds in (True, False):
                    del eng.lib.calls[:]
                    head = (DSIG, DLEN) if ptrs else (ctx["sig"], ctx["lens"])
                    rows, bounds = eng.detect_cnn_rows(*head, N, 2, device_ptrs=ptrs, rows_dev=rows_dev, want_bounds=want_bounds, **kw)
                    (c,) = detect_calls(eng)
                    assert c["fn"] == "adp_detect_cnn" and head_kind(c) == ("pointers" if ptrs else "host")
                    assert (c["n"], c["m"], c["minibatch"]) == (N, M, 2)
                    assert c["flags"] == sum(f[b] for b in bits) | (f["IN"] if ptrs else 0) | (f["OUT"] if rows_dev else 0), (kw, ptrs, rows_dev)
                    assert (rows is None and c["rows"] == 6000) if rows_dev else (rows.shape == (N,) and c["rows"] == "host")
                    assert c["bounds"] == ((np.dtype(np.int64), (N, 1 + ctx["k"])) if want_bounds else None)
                    assert (bounds is None) == (not want_bounds)


def test_engine_detect_cnn_rows_i16_keywords(ctx):
    f = _flags()
    eng = recorder_engine(ctx["spc"], M)
    for kw, bits in _CNN_KW:
        for rows_dev in (None, 6000):
            for want_bounds in (True, False):
                del eng.lib.calls[:]
                rows, bounds = eng.detect_cnn_rows_i16(DRAW, DLEN, DSCALE, DOFF, N, 2, rows_dev=rows_dev, want_bounds=want_bounds, **kw)
                (c,) = detect_calls(eng)
                assert c["fn"] == "adp_detect_cnn_i16" and c["head"] == (DRAW, DLEN, DSCALE, DOFF)
                assert (c["n"], c["m"], c["minibatch"]) == (N, M, 2)
                assert c["flags"] == f["IN"] | sum(f[b] for b in bits) | (f["OUT"] if rows_dev else 0), (kw, rows_dev)
                assert (rows is None and c["rows"] == 6000) if rows_dev else (rows.shape == (N,) and c["rows"] == "host")
                assert c["bounds"] == ((np.dtype(np.int64), (N, 1 + ctx["k"])) if want_bounds else None)


BAD_MODE = r'^fallback must be "device" or "host"$'
SP_CONV = r'^with_start_peak runs inside the library call: conv must be "hip"$'
SP_FALLBACK = r'^with_start_peak runs inside the library call: fallback must be "device"$'
IN_CALL_CONV = r'^the LLR second opinion / the truncation look runs inside the library call: conv must be "hip"$'
IN_CALL_FALLBACK = r'^the LLR second opinion / the truncation look runs inside the library call: fallback must be "device"$'
I16_FORM = r'^int16 rows are read inside the library call: conv must be "hip" and fallback "device"$'


def test_every_refusal_of_a_host_side_form_with_its_message(ctx):
    """engine, model and configuration are None: a refusal looks at none of them"""
    from adapted_amd.detect import cnn

    sig, lens = ctx["sig"], ctx["lens"]
    host = [(cnn.detect_rows_start_peak, {}, True), (cnn.detect_rows_truncated, {}, False), (cnn.detect_rows_truncated, {"with_start_peak": True}, True),
            (cnn.detect_rows_second_opinion, {}, False), (cnn.detect_rows_second_opinion, {"with_start_peak": True}, True),
            (cnn.detect_rows_second_opinion, {"second_opinion": False}, False)]  # (refused whatever the options say)
    for fn, kw, sp in host:
        for bad, msg in ((dict(conv="torch"), SP_CONV if sp else IN_CALL_CONV), (dict(fallback="host"), SP_FALLBACK if sp else IN_CALL_FALLBACK),
                         (dict(fallback="nowhere"), BAD_MODE), (dict(conv="torch", fallback="nowhere"), SP_CONV if sp else IN_CALL_CONV)):
            with pytest.raises(ValueError, match=msg):
                fn(None, sig, lens, None, None, **bad, **kw)
    resident = [(cnn.detect_rows_device_start_peak, {}, True), (cnn.detect_rows_device_truncated, {}, False),
                (cnn.detect_rows_device_truncated, {"with_start_peak": True}, True), (cnn.detect_rows_device_second_opinion, {}, False),
                (cnn.detect_rows_device_second_opinion, {"with_start_peak": True}, True),
                (cnn.detect_rows_device_second_opinion, {"second_opinion": False}, False)]
    for fn, kw, sp in resident:
        for mode, msg in (("host", SP_FALLBACK if sp else IN_CALL_FALLBACK), ("nowhere", BAD_MODE)):
            with pytest.raises(ValueError, match=msg):
                fn(None, DSIG, DLEN, N, lens, None, None, None, mode, **kw)
    for bad, msg in ((dict(conv="torch"), I16_FORM), (dict(fallback="host"), I16_FORM), (dict(fallback="nowhere"), BAD_MODE),
                     (dict(conv="torch", fallback="nowhere"), I16_FORM), (dict(conv="torch", with_start_peak=True), I16_FORM)):
        with pytest.raises(ValueError, match=msg):
            cnn.detect_rows_device_i16(None, DRAW, DLEN, DSCALE, DOFF, N, lens, None, None, **bad)
    with pytest.raises(ValueError, match=SP_CONV):
        cnn.combined_detect_cnn(sig, lens, None, None, conv="torch", with_start_peak=True)
    with pytest.raises(ValueError, match=SP_CONV):
        cnn.combined_detect_cnn(sig, lens, None, None, conv="torch", with_start_peak=True, flag_truncated=True)


def test_refusals_of_the_entries_that_have_the_host_side_forms(ctx, monkeypatch):
    from adapted_amd.detect import cnn, combined

    eng = recorder_engine(ctx["spc"], M)
    with pytest.raises(ValueError, match=BAD_MODE):
        cnn.detect_rows(eng, ctx["sig"], ctx["lens"], ctx["weights"], ctx["spc"], "hip", "nowhere")
    with pytest.raises(ValueError, match=BAD_MODE):
        cnn.detect_rows_device(eng, DSIG, DLEN, N, ctx["lens"], ctx["weights"], ctx["spc"], None, "nowhere")
    assert detect_calls(eng) == []
    monkeypatch.setattr(combined, "get_engine", lambda *a, **kw: eng)
    with pytest.raises(ValueError, match=IN_CALL_CONV):
        cnn.combined_detect_cnn(ctx["sig"], ctx["lens"], ctx["weights"], ctx["spc"], conv="torch", flag_truncated=True)
    assert detect_calls(eng) == []
