"""ADP_CNN_SECOND_RESEGMENT (include/adapted_hip_second_resegment.h) without a GPU: the header against the binding and the untouched
ABI surface, the command line with its refusals, the values of the ``second_opinion`` arguments down to the flag word, the
pipeline's wiring on its three plans (a bare HostPipeline over a recording engine, tests/call_recorder.py), and what the writers
make of a row that carries ``reserved_`` bits 0 and 5 together."""
import csv
import glob
import os
import re

import numpy as np
import pytest

import resegment_cases as R
from call_recorder import detect_calls, names, recorder_engine
from test_cnn_fallback_cpu import _flag_values
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = 1 << 18 | 1 << 23


def _strip(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_defines_its_guard_and_the_flag_only():
    from adapted_amd import lib

    path = os.path.join(ROOT, "include", "adapted_hip_second_resegment.h")
    with open(path) as fh:
        own = fh.read()
    code = [ln.strip() for ln in _strip(own).splitlines() if ln.strip()]
    assert code == ["#ifndef ADAPTED_HIP_SECOND_RESEGMENT_H", "#define ADAPTED_HIP_SECOND_RESEGMENT_H", "#define ADP_CNN_SECOND_RESEGMENT (1 << 23)",
                    "#endif"], code
    assert _prototypes(path) == {} and lib.SECOND_RESEGMENT_PROTOTYPES == {}
    assert lib.ADP_CNN_SECOND_RESEGMENT == 1 << 23
    # the selector it names is the next free one of adp_debug_fetch
    assert "adp_debug_fetch(h, 26, int32[3], 12)" in own and "debug_second_resegment" in vars(lib.Engine)


def test_flag_is_a_single_bit_no_other_flag_of_the_headers_has():
    from adapted_amd import lib

    text = ""
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        with open(path) as fh:
            text += _strip(fh.read()) + "\n"
    flags = _flag_values(text)
    v = flags.pop("ADP_CNN_SECOND_RESEGMENT")
    assert v == 1 << 23 and v & (v - 1) == 0
    assert v not in flags.values(), [k for k, w in flags.items() if w == v]
    # every flag of a `flags` argument is a single bit, and this one lies above all of them
    words = {k: w for k, w in flags.items() if w >= 1 << 17 and w & (w - 1) == 0}
    assert {"ADP_CNN_FALLBACK", "ADP_CNN_SECOND_LLR", "ADP_FLAG_TRUNCATED", "ADP_POLYA_TRUNCATED", "ADP_LLR_RESEGMENT", "ADP_KNN_NO_PRUNE"} <= set(words)
    assert sorted(words.values()) == [1 << b for b in range(17, 23)] and v > max(words.values())
    for other in (lib.ADP_IN_DEVICE, lib.ADP_OUT_DEVICE, lib.ADP_WITH_START_PEAK, lib.ADP_TOPK_NONE, lib.ADP_BOUNDS_HOST, lib.ADP_TAILS_NAN,
                  lib.ADP_CNN_FALLBACK, lib.ADP_CNN_SECOND_LLR, lib.ADP_FLAG_TRUNCATED, lib.ADP_POLYA_TRUNCATED, lib.ADP_LLR_RESEGMENT,
                  lib.ADP_KNN_NO_PRUNE):
        assert lib.ADP_CNN_SECOND_RESEGMENT & other == 0


def test_adapted_hip_h_includes_it_once_and_keeps_its_surface():
    from adapted_amd import lib

    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        raw = fh.read()
    text = _strip(raw)
    assert text.count('#include "adapted_hip_second_resegment.h"') == 1
    assert text.index('#include "adapted_hip_resegment.h"') < text.index('#include "adapted_hip_second_resegment.h"') < text.index("adp_set_profiling")
    assert text.index('extern "C"') < text.index('#include "adapted_hip_second_resegment.h"')
    protos = re.findall(r"^(?:const\s+)?\w+\s*\**\s*(adp_\w+)\s*\([^)]*\)\s*;", text, re.M)
    assert len(protos) == len(set(protos)) == 62 and set(protos) == set(lib.PROTOTYPES)
    assert re.search(r"^#define\s+ADP_ABI_VERSION\s+3\s*$", text, re.M)


def test_parser_takes_the_choice_and_records_it():
    from adapted_amd import main

    args = main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004", "--second_opinion", "llr_resegment", "--start_peak",
                                           "--int16_ingest", "--native_csv", "--adapter_front", "--adapter_front_revalidate"])
    assert args.second_opinion == "llr_resegment" and vars(args)["second_opinion"] == "llr_resegment"  # (command.json is vars(args))
    main._check_second_opinion(args)
    assert main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004", "--second_opinion", "llr"]).second_opinion == "llr"
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004", "--second_opinion", "cnn"])


def _config(tmp_path, change):
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    change(spc)
    spc.update_primary_method()
    fn = str(tmp_path / "cfg.toml")
    spc.to_toml(fn)
    return fn


def _llr(spc):
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False


def _overwrite(spc):
    spc.mvs_polya.mvs_detect_overwrite = True


@pytest.mark.parametrize("change,extra,says", [(_llr, [], "CNN primary"), (lambda spc: None, ["--flag_truncated"], "truncation look"),
                                               (_overwrite, [], "mvs_detect_overwrite")])
def test_cli_refuses_before_a_gpu_is_touched(tmp_path, change, extra, says):
    from adapted_amd import main

    out = tmp_path / "out"
    out.mkdir()
    with pytest.raises(SystemExit) as e:
        main.main(["detect", "-i", str(tmp_path / "none.npz"), "-o", str(out), "--config", _config(tmp_path, change),
                   "--second_opinion", "llr_resegment"] + extra)
    assert "--second_opinion llr_resegment" in str(e.value) and says in str(e.value)
    assert not list(out.iterdir())  # no run directory was made


def test_llr_resegment_under_the_cnn_primary_points_to_the_choice(tmp_path):
    from adapted_amd import main

    with pytest.raises(SystemExit) as e:
        main.main(["detect", "-i", str(tmp_path / "none.npz"), "-o", str(tmp_path), "-c", "RNA004", "--llr_resegment"])
    assert "--llr_resegment" in str(e.value) and "LLR primary" in str(e.value) and "--second_opinion llr_resegment" in str(e.value)
    assert not list(tmp_path.iterdir())


def test_argument_values_reach_the_flag_word():
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.detect import cnn

    assert lib.second_opinion_flags("llr_resegment") == BOTH == lib.ADP_CNN_SECOND_LLR | lib.ADP_CNN_SECOND_RESEGMENT
    assert lib.second_opinion_flags(True) == lib.second_opinion_flags("llr") == 1 << 18
    assert lib.second_opinion_flags(False) == lib.second_opinion_flags(None) == 0
    assert lib._flag_word(fallback=True, second_opinion="llr_resegment", with_start_peak=True) == BOTH | lib.ADP_CNN_FALLBACK | lib.ADP_WITH_START_PEAK
    spc = get_chemistry_specific_config("RNA004")
    m, n = 64, 4
    sig, lens = np.zeros((n, m), dtype=np.float32), np.full(n, m, dtype=np.int32)
    weights = None  # (the configuration's model)
    for value, bits in (("llr_resegment", BOTH), (True, 1 << 18), ("llr", 1 << 18), (False, 0)):
        eng = recorder_engine(spc, m)
        eng.detect_cnn_rows(sig, lens, n, n, fallback=True, second_opinion=value)
        eng.detect_cnn_rows_i16(1000, 2000, 3000, 4000, n, n, fallback=True, second_opinion=value)
        cnn.detect_rows_second_opinion(eng, sig, lens, weights, spc, second_opinion=value)
        cnn.detect_rows_device_second_opinion(eng, 1000, 2000, n, lens, weights, spc, n, second_opinion=value)
        cnn.detect_rows_device_i16(eng, 1000, 2000, 3000, 4000, n, lens, weights, spc, n, second_opinion=value)
        calls = detect_calls(eng)
        assert [c["fn"] for c in calls] == ["adp_detect_cnn", "adp_detect_cnn_i16", "adp_detect_cnn", "adp_detect_cnn", "adp_detect_cnn_i16"]
        for c in calls:
            assert c["flags"] & BOTH == bits and c["flags"] & lib.ADP_CNN_FALLBACK, (value, c["fn"], c["flags"])
    eng = recorder_engine(spc, m)
    for call in (lambda: eng.detect_cnn_rows(sig, lens, n, n, second_opinion="x"),
                 lambda: eng.detect_cnn_rows_i16(1000, 2000, 3000, 4000, n, n, second_opinion="x"),
                 lambda: cnn.detect_rows_second_opinion(eng, sig, lens, weights, spc, second_opinion="x"),
                 lambda: lib.second_opinion_flags("cnn")):
        with pytest.raises(ValueError, match="second_opinion"):
            call()
    assert not detect_calls(eng)
    assert lib.second_resegment_unsupported(spc) is None and "truncation look" in lib.second_resegment_unsupported(spc, True)
    assert "CNN primary" in lib.second_resegment_unsupported(R.spc_of())


@pytest.mark.parametrize("plan", ["float32", "int16 calibrated", "int16 native"])
@pytest.mark.parametrize("value", ["llr_resegment", "llr", None])
def test_pipeline_hands_the_value_through(plan, value):
    from adapted_amd import lib, pipeline
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.primary, p.with_start_peak, p.second_opinion, p.flag_truncated = "cnn", False, value, False
    p.native_i16, p.i16, p.ragged = plan == "int16 native", plan != "float32", False
    p.model, p.spc = None, spc
    p.mb, p.N = 16, 32
    p.dsig16 = 7000 if plan == "int16 calibrated" else None
    p.eng = recorder_engine(spc, 64)
    p.slots = [{"ds": 1000, "dl": 2000, "dcal": 3000, "do": 4000, "lens": np.arange(32, dtype=np.int32)}]
    rows, mbs = p._detect(0, 16)
    assert rows.shape == (16,) and mbs is None
    (c,) = detect_calls(p.eng)
    assert c["fn"] == ("adp_detect_cnn_i16" if plan == "int16 native" else "adp_detect_cnn")
    want = {"llr_resegment": BOTH, "llr": 1 << 18, None: 0}[value]
    assert c["flags"] == lib.ADP_IN_DEVICE | lib.ADP_CNN_FALLBACK | want
    assert ("adp_calibrate_i16" in names(p.eng)) == (plan == "int16 calibrated")
    assert c["head"][0] == (7000 if plan == "int16 calibrated" else 1000)


def test_pipeline_constructor_takes_the_value_and_keeps_the_native_plan(monkeypatch):
    from adapted_amd import lib, pipeline
    from adapted_amd.config import get_chemistry_specific_config

    class Eng:
        def __init__(self, *a, **kw):
            pass

        def dev_alloc(self, nbytes):
            return 4096

    monkeypatch.setattr(lib, "Engine", Eng)
    spc = get_chemistry_specific_config("RNA004")
    p = pipeline.HostPipeline(spc, 8, R.M, primary="cnn", int16_input="native", second_opinion="llr_resegment")
    assert p.second_opinion == "llr_resegment" and p.native_i16, "the phase has an int16 form: the slot is not calibrated first"
    with pytest.raises(ValueError, match="CNN primary"):
        pipeline.HostPipeline(R.spc_of(), 8, R.M, primary="llr", second_opinion="llr_resegment")
    with pytest.raises(ValueError, match="truncation look"):
        pipeline.HostPipeline(spc, 8, R.M, primary="cnn", second_opinion="llr_resegment", flag_truncated=True)
    over = get_chemistry_specific_config("RNA004")
    over.mvs_polya.mvs_detect_overwrite = True
    with pytest.raises(ValueError, match="mvs_detect_overwrite"):
        pipeline.HostPipeline(over, 8, R.M, primary="cnn", second_opinion="llr_resegment")
    with pytest.raises(ValueError, match="second_opinion"):
        pipeline.HostPipeline(spc, 8, R.M, primary="cnn", second_opinion="x")


def _hand_made_rows(code):
    from adapted_amd import lib

    rows = lib.empty_rows(2)
    cols = ("{primary}_adapter_end", "{primary}_polya_end", "adapter_start", "adapter_end", "polya_end")
    for r, vals in zip(rows, ((3140, 4040, 1900, 3140, 4040), (3000, 3900, 0, 3000, 3900))):
        for c, v in zip(cols, vals):
            r["col"][lib.COLS.index(c)] = v
        r["present"] = sum(1 << lib.COLS.index(c) for c in cols)
        r["n_cand"], r["n_open_pores"] = 1, 0
        r["cand"][0] = vals[1]
    rows["success"] = 1
    rows["reserved_"] = [lib.ROW_FROM_SECOND_LLR | lib.ROW_RESEGMENTED | code << lib.ROW_FIRST_FAIL_SHIFT, 0]
    return rows


def test_writers_name_such_a_row_as_an_llr_row_and_say_so(tmp_path):
    from adapted_amd import lib
    from adapted_amd.container_types import ReadResult
    from adapted_amd.output import CSV_COLUMNS, save_detected_boundaries

    assert lib.ROW_FROM_SECOND_LLR | lib.ROW_RESEGMENTED == 1 | 32
    codes = [c for c in range(16) if lib.FAIL_REASONS[c]]
    assert {2, 4, 6, 7, 8} <= set(codes)
    table, offsets = lib.csv_string_table()
    for code in codes:
        kept, plain = lib.rows_to_results(_hand_made_rows(code), "cnn")
        text = "resegmented: first pass failed (%s)" % lib.FAIL_REASONS[code].rstrip(": ")
        assert kept.llr_detect_log == text and kept.success and kept.fail_reason is None and kept.adapter_start == 1900
        assert (kept.llr_adapter_end, kept.llr_polya_end, kept.polya_candidates.tolist()) == (3140, 4040, [4040])
        assert kept.cnn_adapter_end is None and kept.cnn_polya_end is None
        assert (plain.cnn_adapter_end, plain.cnn_polya_end, plain.llr_adapter_end, plain.llr_detect_log) == (3000, 3900, None, None)
        # the native CSV's text table holds the same cell for the code (include/adapted_hip_csv.h: entries 19 .. 34)
        at = 19 + code
        assert bytes(table[offsets[at]:offsets[at + 1]]).decode() == text
        fn = str(tmp_path / ("detected_boundaries_%d.csv" % code))
        save_detected_boundaries([ReadResult(read_id="read-%d" % i, success=True, fail_reason=None, detect_results=r) for i, r in enumerate((kept, plain))], fn)
        with open(fn, newline="") as fh:
            lines = list(csv.reader(fh))  # (a reason may hold a comma: the cell is quoted then)
        assert lines[0] == CSV_COLUMNS
        cell = {name: [ln[lines[0].index(name)] for ln in lines[1:]] for name in ("llr_detect_log", "adapter_start", "llr_adapter_end", "llr_polya_end",
                                                                                 "cnn_adapter_end")}
        assert cell["llr_detect_log"] == [text, ""] and cell["adapter_start"] == ["1900", "0"]
        # (pandas prints a column that is empty on some lines as floats)
        assert float(cell["llr_adapter_end"][0]) == 3140 and float(cell["llr_polya_end"][0]) == 4040
        assert cell["cnn_adapter_end"][0] == "" and float(cell["cnn_adapter_end"][1]) == 3000
        assert lib.rows_csv_text(_hand_made_rows(code), ["read-0", "read-1"], "cnn") == open(fn, "rb").read()
    marks = _hand_made_rows(7)["reserved_"]
    assert lib.resegment_log(marks) == "LLR re-segmentation: 1 reads kept (first failure: MVS polya check failed: 1)"
