"""The LLR second opinion of the CNN operator inside adp_detect_cnn (ADP_CNN_SECOND_LLR): what can be checked without a GPU --
the flag's bit in the header and in the binding, the untouched ABI surface, the new Python names, how a marked row is named, and
the command line's acceptance and refusal of --second_opinion."""
import inspect
import os
import re

import numpy as np
import pytest

from test_cnn_fallback_cpu import _flag_values, _header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_flag_with_bit_18_and_the_binding_carries_it():
    from adapted_amd import lib

    flags = _flag_values(_header_text())
    assert flags.get("ADP_CNN_SECOND_LLR") == 1 << 18
    others = {k: w for k, w in flags.items() if k != "ADP_CNN_SECOND_LLR"}
    assert all(w & (w - 1) == 0 for w in others.values()), others
    assert (1 << 18) not in others.values(), [k for k, w in others.items() if w == 1 << 18]
    assert lib.ADP_CNN_SECOND_LLR == 1 << 18 and lib.ADP_CNN_FALLBACK == flags["ADP_CNN_FALLBACK"]


def test_no_new_exported_function_and_the_same_abi_version():
    from adapted_amd import lib

    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        raw = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    protos = re.findall(r"^(?:const\s+)?\w+\s*\**\s*(adp_\w+)\s*\([^)]*\)\s*;", text, re.M)
    assert len(protos) == len(set(protos)) == 62
    assert set(protos) == set(lib.PROTOTYPES)
    assert re.search(r"^#define\s+ADP_ABI_VERSION\s+3\s*$", text, re.M)
    # the row keeps its layout and the field its name; the header says what bit 0 means
    assert re.search(r"int32_t\s+reserved_;\s*/\*[^/]*ADP_CNN_SECOND_LLR", raw)
    assert lib.ROW_DTYPE.itemsize == 544 and lib.ROW_DTYPE.names[-1] == "reserved_"


def test_new_python_names_and_second_opinion_is_the_last_keyword():
    from adapted_amd import lib, pipeline
    from adapted_amd.detect import cnn, combined

    p = list(inspect.signature(lib.Engine.detect_cnn_rows).parameters.values())
    assert [q.name for q in p][-2:] == ["fallback", "second_opinion"] and p[-1].default is False
    assert callable(lib.Engine.debug_cnn_second_opinion)
    p = list(inspect.signature(pipeline.HostPipeline.__init__).parameters.values())
    assert p[-1].name == "second_opinion" and p[-1].default is None
    # the host entry points are new names beside the pinned ones, host and device-resident
    p = list(inspect.signature(cnn.detect_rows_second_opinion).parameters.values())
    assert [q.name for q in p][:5] == ["eng", "sig", "lens", "model", "spc"]
    p = list(inspect.signature(cnn.detect_rows_device_second_opinion).parameters.values())
    assert [q.name for q in p][:8] == ["eng", "dsig", "dlen", "n", "lens_host", "model", "spc", "minibatch"]
    p = list(inspect.signature(combined.combined_detect_cnn_llr).parameters.values())
    assert [q.name for q in p] == ["batch_of_signals", "full_signal_lens", "model", "spc", "device"] and p[-1].default == 0


def test_host_side_variants_have_no_second_opinion_form():
    """raised before the engine is looked at"""
    from adapted_amd.detect import cnn

    with pytest.raises(ValueError, match="conv"):
        cnn.detect_rows_second_opinion(None, np.zeros((1, 8), np.float32), np.zeros(1, np.int32), None, None, conv="torch")
    with pytest.raises(ValueError, match="fallback"):
        cnn.detect_rows_second_opinion(None, np.zeros((1, 8), np.float32), np.zeros(1, np.int32), None, None, fallback="host")
    with pytest.raises(ValueError, match="fallback"):
        cnn.detect_rows_device_second_opinion(None, 0, 0, 1, np.zeros(1, np.int32), None, None, None, "host")


def _hand_made_rows():
    from adapted_amd import lib

    rows = lib.empty_rows(3)
    for r, (ae, pe) in zip(rows, [(2880, 9810), (3010, 5230), (2950, 0)]):
        r["col"][lib.COLS.index("{primary}_adapter_end")] = ae
        r["col"][lib.COLS.index("{primary}_polya_end")] = pe
        r["col"][lib.COLS.index("adapter_end")] = ae
        r["present"] = sum(1 << lib.COLS.index(c) for c in ("{primary}_adapter_end", "{primary}_polya_end", "adapter_end"))
        r["n_cand"], r["n_open_pores"] = 0, 0
    rows["success"] = [1, 1, 0]
    rows["fail_code"] = [0, 0, 5]
    rows["reserved_"] = [0, 1, 0]
    return rows


def test_rows_to_results_names_a_marked_row_as_the_llr_path_does():
    from adapted_amd import lib

    res = lib.rows_to_results(_hand_made_rows(), "cnn")
    plain, marked, failed = res
    assert (plain.cnn_adapter_end, plain.cnn_polya_end) == (2880, 9810)
    assert plain.llr_adapter_end is None and plain.llr_polya_end is None and plain.llr_detect_log is None
    assert (marked.llr_adapter_end, marked.llr_polya_end) == (3010, 5230) and marked.llr_detect_log == ""
    assert marked.cnn_adapter_end is None and marked.cnn_polya_end is None
    assert marked.success and marked.adapter_end == 3010 and marked.fail_reason is None
    assert (failed.cnn_adapter_end, failed.cnn_polya_end) == (2950, 0) and failed.llr_adapter_end is None
    assert failed.fail_reason == "No polya detected (primary)"
    # without a marked row nothing changes, whatever the primary
    rows = _hand_made_rows()
    rows["reserved_"] = 0
    for primary in ("cnn", "llr", "start_peak"):
        got = lib.rows_to_results(rows, primary)
        assert all(getattr(g, primary + "_adapter_end") is not None for g in got)
        assert all(getattr(g, o + "_adapter_end") is None for g in got for o in ("cnn", "llr", "start_peak") if o != primary)


def test_cli_accepts_the_flag_with_the_cnn_primary_and_records_it():
    from adapted_amd import main

    args = main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004", "--second_opinion", "llr"])
    assert args.second_opinion == "llr" and vars(args)["second_opinion"] == "llr"   # (command.json is vars(args): `continue` repeats it)
    main._check_second_opinion(args)                                                 # RNA004's primary is the CNN
    assert main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004"]).second_opinion is None
    assert "second_opinion" in inspect.signature(main.run_detect).parameters


def test_cli_refuses_the_flag_without_the_cnn_primary_before_anything_runs(tmp_path):
    from adapted_amd import main

    with pytest.raises(SystemExit) as e:
        main.main(["detect", "-i", str(tmp_path / "none.npz"), "-o", str(tmp_path), "-c", "RNA002", "--second_opinion", "llr"])
    assert "CNN primary" in str(e.value)
    assert not list(tmp_path.iterdir())  # no run directory was made
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004", "--second_opinion", "cnn"])


def test_pipeline_refuses_a_second_opinion_for_another_primary():
    from adapted_amd import pipeline

    with pytest.raises(ValueError, match="CNN primary"):
        pipeline.HostPipeline(None, 16, 1024, primary="llr", second_opinion="llr")
    with pytest.raises(ValueError, match="second_opinion"):
        pipeline.HostPipeline(None, 16, 1024, primary="cnn", second_opinion="cnn")
