"""The host side of the CNN primary over raw int16 rows (adp_detect_cnn_i16), without a GPU: the new header against its prototype
table, the binding, the plan that decides whether the detect kernels read the raw rows themselves, and the way the option travels
from the command line to the operator."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototypes(path):
    """a header, comments stripped -> {name: (return kind, [parameter kinds])} in lib.PROTOTYPES' vocabulary"""
    with open(path) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)

    def kind(decl, named):
        m = re.fullmatch(r"(?:const\s+)?(\w+?)(?:_t)?\s*((?:\*\s*)*)" + (r"\w+" if named else ""), decl.strip())
        assert m, decl
        return m.group(1) + "*" * m.group(2).count("*")

    out = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\**)\s*(adp_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        out[name] = (kind(ret, False), [] if params.strip() == "void" else [kind(q, True) for q in params.split(",")])
    return out


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(os.path.join(ROOT, "include", "adapted_hip_i16.h"))
    assert sorted(declared) == sorted(lib.I16_PROTOTYPES) == ["adp_detect_cnn_i16"]
    assert not set(lib.I16_PROTOTYPES) & (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES))
    assert "adp_detect_llr_i16" in lib.PROTOTYPES and "adp_detect_cnn_i16" not in lib.EXPORTS
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        assert '#include "adapted_hip_i16.h"' in fh.read()
    L = lib.load()
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.I16_PROTOTYPES[name].split(":")
        assert got_ret == ret and got_params.split() == params, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for q, t in zip(params, fn.argtypes):
            if q in lib._SCALARS:
                assert t is lib._SCALARS[q], (name, q)
            elif q[:-1] in lib._ELEMENTS:
                assert isinstance(t, lib._Pointer) and t.element == q[:-1], (name, q)
            else:
                assert t is ctypes.c_void_p and q == "adp_handle*", (name, q)
    # the LLR twin's parameters up to the last one, which is the predictions instead of the minibatch status
    llr = lib.PROTOTYPES["adp_detect_llr_i16"].split()
    assert lib.I16_PROTOTYPES["adp_detect_cnn_i16"].split()[:-1] == llr[:-1] and llr[-1] == "int32*"
    assert declared["adp_detect_cnn_i16"][1][-1] == "int64*"


def test_null_handle_is_refused_and_wrong_types_never_enter_the_library():
    from adapted_amd import lib

    L = lib.load()
    assert L.adp_detect_cnn_i16(None, None, None, None, None, 4, 8, 4, lib.ADP_IN_DEVICE, None, None) == -1  # ADP_ERR_INVALID
    assert b"bad argument" in L.adp_last_error()
    with pytest.raises(ctypes.ArgumentError):
        L.adp_detect_cnn_i16(None, np.zeros(8, dtype=np.float32), None, None, None, 1, 8, 1, 0, None, None)  # float32 for int16 *raw
    with pytest.raises(ctypes.ArgumentError):
        L.adp_detect_cnn_i16(None, None, None, None, None, 1, 8, 1, 0, None, np.zeros(2, dtype=np.int32))  # int32 for int64 *bounds_out


def test_native_int16_plan_truth_table():
    from adapted_amd.pipeline import native_int16_plan as plan

    for primary in ("llr", "cnn", "start_peak"):
        for i16 in (False, True, "native"):
            for m in (17500, 17503):
                for trunc in (False, True):
                    want = bool(i16) and m % 4 == 0 and not trunc and (primary == "llr" or (primary == "cnn" and i16 == "native"))
                    got = plan(primary, i16, m, trunc)
                    assert got is want, (primary, i16, m, trunc, got)
    assert plan("cnn", "native", 17500, False) and not plan("cnn", True, 17500, False)  # True keeps the float32 route for the CNN
    assert plan("llr", True, 17500, False) and plan("llr", "native", 17500, False)
    assert not plan("start_peak", "native", 17500, False)


def test_pipeline_constructor_uses_the_plan(monkeypatch):
    """HostPipeline with a stand-in engine: native_i16 is the plan's answer, and with it and padded slots no matrix is allocated"""
    from adapted_amd import lib, pipeline
    from adapted_amd.config import get_chemistry_specific_config

    allocs = []

    class Eng:
        def __init__(self, *a, **kw):
            pass

        def dev_alloc(self, nbytes):
            allocs.append(nbytes)
            return 4096 * len(allocs)

    monkeypatch.setattr(lib, "Engine", Eng)
    spc = get_chemistry_specific_config("RNA004")
    m = 17500
    for i16, ragged, native, matrix in (("native", False, True, None), ("native", True, True, 2), (True, False, False, 4), (False, False, False, None),
                                        (False, True, False, 4)):
        del allocs[:]
        p = pipeline.HostPipeline(spc, 8, m, primary="cnn", int16_input=i16, ragged=ragged, second_opinion="llr", with_start_peak=True)
        assert p.native_i16 is native and p.i16 is bool(i16), (i16, ragged)
        assert allocs == ([] if matrix is None else [8 * m * matrix]), (i16, ragged, allocs)
        assert (p.dsig16 is None) == (matrix is None)
    p = pipeline.HostPipeline(spc, 8, 17503, primary="cnn", int16_input="native")
    assert not p.native_i16 and p.dsig16 is not None
    with pytest.raises(ValueError, match="int16_input"):
        pipeline.HostPipeline(spc, 8, m, primary="cnn", int16_input="raw")


@pytest.mark.parametrize("ragged", [False, True])
def test_pipeline_hands_the_slot_and_the_options_to_the_int16_operator(ragged):
    """HostPipeline._detect of a bare object with native_i16 and the CNN primary, read where the library is called (a bare engine
    whose library is a recorder, tests/call_recorder.py)"""
    from adapted_amd import lib, pipeline
    from adapted_amd.config import get_chemistry_specific_config
    from call_recorder import detect_calls, names, recorder_engine

    spc = get_chemistry_specific_config("RNA004")
    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.primary, p.with_start_peak, p.second_opinion, p.flag_truncated = "cnn", True, "llr", False
    p.native_i16, p.i16, p.ragged = True, True, ragged
    p.model, p.spc = None, spc
    p.mb, p.N = 16, 32
    p.dsig16 = 7000 if ragged else None
    p.eng = recorder_engine(spc, 64)
    p.slots = [{"ds": 1000, "dl": 2000, "dcal": 3000, "do": 4000, "lens": np.arange(32, dtype=np.int32)}]
    rows, mbs = p._detect(0, 16)
    assert rows.shape == (16,) and rows.dtype == lib.ROW_DTYPE and mbs is None
    (c,) = detect_calls(p.eng)
    assert c["fn"] == "adp_detect_cnn_i16", "the float32 operators must not run on the native plan"
    # with_start_peak True, second_opinion True (and the fallback inside the call, the rows resident)
    assert c["flags"] == lib.ADP_IN_DEVICE | lib.ADP_CNN_FALLBACK | lib.ADP_WITH_START_PEAK | lib.ADP_CNN_SECOND_LLR
    assert c["head"] == (7000 if ragged else 1000, 2000, 3000, 3000 + 32 * 4) and (c["n"], c["m"], c["minibatch"]) == (16, 64, 16)
    calls = p.eng.lib.calls
    assert calls[0] == ("adp_copy_wait", (None, 0))
    if ragged:
        assert calls[1] == ("adp_expand_ragged_i16", (None, 1000, 4000, 2000, 16, 64, 7000))
    assert names(p.eng) == ["adp_copy_wait"] + (["adp_expand_ragged_i16"] if ragged else []) + ["adp_cnn_set_weights", "adp_detect_cnn_i16"], \
        "no calibration pass on the native plan"


def test_the_llr_primary_keeps_its_int16_call(monkeypatch):
    """a bare object as the existing tests build them, native_i16 with the LLR primary: detect_llr_rows_i16, as before"""
    from adapted_amd import pipeline

    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.primary, p.with_start_peak, p.second_opinion, p.flag_truncated = "llr", False, None, False
    p.native_i16, p.i16, p.ragged = True, True, False
    p.mb, p.N = 16, 16

    class Eng:
        def copy_wait(self, j):
            pass

        def detect_llr_rows_i16(self, *a, **kw):
            return ("llr", a, kw)

    p.eng = Eng()
    p.slots = [{"ds": 1, "dl": 2, "dcal": 3, "lens": np.zeros(16, np.int32)}]
    assert p._detect(0, 16) == ("llr", (1, 2, 3, 3 + 64, 16, 16), {"with_start_peak": False})


@pytest.mark.parametrize("ingest", [False, True])
def test_run_detect_constructs_the_pipeline_with_the_native_plan(monkeypatch, tmp_path, ingest):
    from adapted_amd import main, pipeline
    from adapted_amd.config import get_chemistry_specific_config

    seen = {}

    class Stop(Exception):
        pass

    def recorder(*a, **kw):
        seen.update(kw)
        raise Stop()

    monkeypatch.setattr(pipeline, "HostPipeline", recorder)
    spc = get_chemistry_specific_config("RNA004")
    with pytest.raises(Stop):
        main.run_detect([], set(), set(), spc, str(tmp_path), 16, 4000, 0, int16_ingest=ingest)
    assert seen["int16_input"] == ("native" if ingest else False) and seen["primary"] == "cnn"
    assert isinstance(seen["int16_input"], str) == ingest


def test_cli_help_says_both_primaries_read_the_raw_samples(capsys):
    from adapted_amd import main

    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["detect", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    para = text[text.rindex("--int16_ingest"):]
    assert "LLR" in para and "CNN" in para and "raw samples" in para


def test_new_names_and_their_parameters():
    from adapted_amd import lib, pipeline
    from adapted_amd.detect import cnn

    assert list(inspect.signature(lib.Engine.detect_cnn_rows_i16).parameters) == [
        "self", "raw_dev", "len_dev", "scale_dev", "offset_dev", "n", "minibatch", "rows_dev", "want_bounds", "with_start_peak", "fallback",
        "second_opinion"]
    d = {k: v.default for k, v in inspect.signature(lib.Engine.detect_cnn_rows_i16).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"rows_dev": None, "want_bounds": True, "with_start_peak": False, "fallback": False, "second_opinion": False}
    names = list(inspect.signature(cnn.detect_rows_device_i16).parameters)
    assert names[:12] == ["eng", "draw", "dlen", "dscale", "doffset", "n", "lens_host", "model", "spc", "minibatch", "with_start_peak", "second_opinion"]
    assert names[12:] == ["fallback", "conv"]  # (the forms the call does not have, named so that they can be refused)
    for bad in (dict(fallback="host"), dict(conv="torch"), dict(fallback="nowhere")):
        with pytest.raises(ValueError):
            cnn.detect_rows_device_i16(None, 0, 0, 0, 0, 1, None, None, None, **bad)
    assert list(inspect.signature(pipeline.native_int16_plan).parameters) == ["primary", "int16_input", "m", "flag_truncated"]
    # what the existing tests pin stays pinned
    assert list(inspect.signature(pipeline.HostPipeline.__init__).parameters)[-1] == "second_opinion"
    assert list(inspect.signature(lib.Engine.detect_cnn_rows).parameters)[-2:] == ["fallback", "second_opinion"]
    assert lib.load().adp_abi_version() == 3
