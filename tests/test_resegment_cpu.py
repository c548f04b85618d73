"""The re-segmentation of reads the LLR primary fails (ADP_LLR_RESEGMENT, include/adapted_hip_resegment.h) without a GPU: the
second segmentation restated from the checkers (tests/resegment_restated.py) against what the real reference stored
(tests/golden/resegment_*.npz), what the stored batches reach, the header against the binding, rows_to_results and the CSV text,
the command line with its refusals, and the pipeline's wiring with a stand-in engine."""
import inspect
import os
import re

import numpy as np
import pytest

import resegment_cases as R
import resegment_restated as rr
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,mb", R.RUNS)
def test_restated_second_segmentation_equals_the_reference(oracle_mod, name, mb):
    """c and p2 of every eligible read, from the reference's stored first rows and from the CPU oracle's own"""
    g = R.load(name, mb)
    sig, lens = R.batch(name)
    spc = R.spc_of()
    for first in (g["first"], None):
        elig, c, p2 = rr.second_segmentation(oracle_mod, sig, lens, spc, mb, first)
        assert elig.tolist() == g["eligible"].tolist()
        assert c.tolist() == g["c"].tolist() and p2.tolist() == g["p2"].tolist(), np.flatnonzero((c != g["c"]) | (p2 != g["p2"]))
    assert g["eligible"].sum() >= 3 and [R.eligible(r) for r in g["first"]] == g["eligible"].tolist()


def test_stored_batches_reach_every_outcome():
    for name, mb in R.RUNS:
        g = R.load(name, mb)
        cov = R.coverage(name, g)
        assert not [k for k in R.REQUIRED[name] if k not in cov], (name, mb, sorted(cov))
        exp, counts, kinds = R.expected(g)
        assert counts[0] >= counts[1] >= counts[2] and counts[2] == kinds.count("kept")
        for e, k in zip(exp, kinds):
            if k == "kept":
                assert e["success"] and e["_reserved"] & R.ROW_RESEGMENTED and e["llr_detect_log"].startswith("resegmented: first pass failed (")
                assert e["adapter_start"] > 0 and e["llr_adapter_end"] == e["adapter_end"] and e["polya_candidates"] == [e["llr_polya_end"]]
            elif e is not None:
                assert e["_reserved"] == 0 and e["llr_detect_log"] == ""
    g = R.load("main", 48)
    exp, counts, kinds = R.expected(g)
    assert counts == (24, 24, 21) and [r for r, k in enumerate(kinds) if k == "second_failed"] == [21, 22, 34]
    # (the read the issue quotes: truth (3141, 4043))
    assert (g["first"][1]["llr_adapter_end"], g["first"][1]["llr_polya_end"]) == (1900, 3140)
    assert (exp[1]["adapter_start"], exp[1]["adapter_end"], exp[1]["polya_end"]) == (1900, 3140, 4040)


def test_header_against_the_binding():
    from adapted_amd import lib

    path = os.path.join(ROOT, "include", "adapted_hip_resegment.h")
    assert _prototypes(path) == {} and lib.RESEGMENT_PROTOTYPES == {}  # (a flag, row bits and a debug selector: no entry point)
    with open(path) as fh:
        own = fh.read()
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_resegment.h"') == 1
    assert text.index('#include "adapted_hip_templates.h"') < text.index('#include "adapted_hip_resegment.h"') < text.index("adp_set_profiling")
    assert re.search(r"^#define\s+ADP_LLR_RESEGMENT\s+\(1 << 21\)", own, re.M) and lib.ADP_LLR_RESEGMENT == 1 << 21
    assert re.search(r"^#define\s+ADP_ROW_RESEGMENTED\s+32\s*$", own, re.M) and lib.ROW_RESEGMENTED == 32
    assert re.search(r"^#define\s+ADP_ROW_FIRST_FAIL_SHIFT\s+6\s*$", own, re.M) and (lib.ROW_FIRST_FAIL_SHIFT, lib.ROW_FIRST_FAIL_MASK) == (6, 15 << 6)
    assert (R.ROW_RESEGMENTED, R.ROW_FIRST_FAIL_SHIFT) == (lib.ROW_RESEGMENTED, lib.ROW_FIRST_FAIL_SHIFT)
    flags = [lib.ADP_IN_DEVICE, lib.ADP_OUT_DEVICE, lib.ADP_WITH_START_PEAK, lib.ADP_TOPK_NONE, lib.ADP_BOUNDS_HOST, lib.ADP_TAILS_NAN,
             lib.ADP_CNN_FALLBACK, lib.ADP_CNN_SECOND_LLR, lib.ADP_FLAG_TRUNCATED, lib.ADP_POLYA_TRUNCATED]
    assert all(lib.ADP_LLR_RESEGMENT & f == 0 for f in flags) and lib.ADP_LLR_RESEGMENT > max(flags)
    bits = lib.ROW_FROM_SECOND_LLR | lib.ROW_POLYA_TRUNCATED | lib.ROW_TRUNC_LOOKED | lib.ROW_ADAPTER_FRONT | lib.ROW_REVALIDATED
    assert (lib.ROW_RESEGMENTED | lib.ROW_FIRST_FAIL_MASK) & bits == 0 and max(lib.FAIL_REASONS) <= 15
    assert re.search(r"^#define\s+ADP_ABI_VERSION\s+3\s*$", text, re.M)
    assert lib._flag_word(resegment=True) == lib.ADP_LLR_RESEGMENT
    for text_of, code in R._FAIL_CODES:
        assert lib.FAIL_REASONS[code] == text_of and lib.first_fail_text(code) == R.fail_text(code)


def _hand_made_rows():
    from adapted_amd import lib

    rows = lib.empty_rows(3)
    cols = ("{primary}_adapter_end", "{primary}_polya_end", "adapter_start", "adapter_end", "polya_end")
    for r, vals in zip(rows, ((3140, 4040, 1900, 3140, 4040), (3000, 3900, 0, 3000, 3900), (1900, 3140, 0, 1900, 3140))):
        for c, v in zip(cols, vals):
            r["col"][lib.COLS.index(c)] = v
        r["present"] = sum(1 << lib.COLS.index(c) for c in cols)
        r["n_cand"], r["n_open_pores"] = 1, 0
        r["cand"][0] = vals[1]
    rows["success"] = [1, 1, 0]
    rows["fail_code"] = [0, 0, 2]
    rows["reserved_"] = [lib.ROW_RESEGMENTED | 7 << lib.ROW_FIRST_FAIL_SHIFT, 0, 0]
    return rows


def test_rows_to_results_and_the_csv_text(tmp_path):
    from adapted_amd import lib
    from adapted_amd.container_types import ReadResult
    from adapted_amd.output import CSV_COLUMNS, save_detected_boundaries

    kept, plain, failed = lib.rows_to_results(_hand_made_rows(), "llr")
    assert kept.llr_detect_log == "resegmented: first pass failed (MVS polya check failed)" and kept.success and kept.adapter_start == 1900
    assert (kept.llr_adapter_end, kept.llr_polya_end, kept.polya_candidates.tolist()) == (3140, 4040, [4040])
    assert plain.llr_detect_log == "" and failed.llr_detect_log == "" and failed.fail_reason == "adapter MAD check failed"
    assert kept.polya_truncated is None and kept.fail_reason is None
    for code, text in ((2, "adapter MAD check failed"), (4, "Real signal check failed")):
        rows = _hand_made_rows()
        rows["reserved_"][0] = lib.ROW_RESEGMENTED | code << lib.ROW_FIRST_FAIL_SHIFT
        assert lib.rows_to_results(rows, "llr")[0].llr_detect_log == "resegmented: first pass failed (%s)" % text
    fn = str(tmp_path / "detected_boundaries_0.csv")
    res = [kept, plain]
    save_detected_boundaries([ReadResult(read_id="read-%d" % i, success=True, fail_reason=None, detect_results=r) for i, r in enumerate(res)], fn)
    with open(fn) as fh:
        lines = [ln.rstrip("\n").split(",") for ln in fh]
    assert lines[0] == CSV_COLUMNS  # (no column is added)
    at = lines[0].index("llr_detect_log")
    assert [ln[at] for ln in lines[1:]] == ["resegmented: first pass failed (MVS polya check failed)", ""]
    assert [ln[lines[0].index("adapter_start")] for ln in lines[1:]] == ["1900", "0"]
    marks = _hand_made_rows()["reserved_"]
    assert lib.resegment_log(marks) == "LLR re-segmentation: 1 reads kept (first failure: MVS polya check failed: 1)"
    assert lib.resegment_log(np.zeros(4, dtype=np.int32)) == "LLR re-segmentation: 0 reads kept"
    both = np.array([32 | 2 << 6, 32 | 2 << 6, 32 | 4 << 6, 0], dtype=np.int32)
    assert lib.resegment_log(both) == "LLR re-segmentation: 3 reads kept (first failure: adapter MAD check failed: 2, Real signal check failed: 1)"


def _config(tmp_path, change):
    spc = R.spc_of()
    change(spc)
    spc.update_primary_method()
    fn = str(tmp_path / "cfg.toml")
    spc.to_toml(fn)
    return fn


def test_cli_takes_the_flag_and_records_it(tmp_path):
    from adapted_amd import main

    cfg = _config(tmp_path, lambda spc: None)
    args = main.build_parser().parse_args(["detect", "-i", "x.npz", "--config", cfg, "--llr_resegment", "--start_peak", "--int16_ingest",
                                           "--adapter_front", "--adapter_front_revalidate"])
    assert args.llr_resegment is True and vars(args)["llr_resegment"] is True  # (command.json is vars(args): `continue` repeats it)
    main._check_llr_resegment(args)
    assert main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004"]).llr_resegment is False
    assert inspect.signature(main.run_detect).parameters["llr_resegment"].default is False
    # `continue` takes what command.json recorded and checks it again
    src = inspect.getsource(main.main)
    assert src.count("_check_llr_resegment(args)") == 2 and 'llr_resegment=getattr(args, "llr_resegment", False)' in src


def _cnn(spc):
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = False, True


def _start_peak(spc):
    spc.llr_boundaries.llr_detect, spc.rna_start_peak.detect_rna_start_peak = False, True


def _overwrite(spc):
    spc.mvs_polya.mvs_detect_overwrite = True


@pytest.mark.parametrize("change,extra,says", [(_cnn, [], "LLR primary"), (_start_peak, [], "LLR primary"), (_overwrite, [], "mvs_detect_overwrite"),
                                               (lambda spc: None, ["--flag_truncated"], "truncation look"), (None, [], "LLR primary")])
def test_cli_refuses_before_a_gpu_is_touched(tmp_path, change, extra, says):
    """a primary other than llr (the preset alone, -c RNA004, selects the CNN), --flag_truncated, mvs_detect_overwrite"""
    from adapted_amd import main

    how = ["-c", "RNA004"] if change is None else ["--config", _config(tmp_path, change)]
    out = tmp_path / "out"
    out.mkdir()
    with pytest.raises(SystemExit) as e:
        main.main(["detect", "-i", str(tmp_path / "none.npz"), "-o", str(out)] + how + ["--llr_resegment"] + extra)
    assert "--llr_resegment" in str(e.value) and says in str(e.value)
    assert not list(out.iterdir())  # no run directory was made


def test_pipeline_passes_the_option_on_and_leaves_the_native_int16_plan(monkeypatch):
    from adapted_amd import lib, pipeline
    from adapted_amd.detect import combined

    calls, allocs = [], []

    class Eng:
        def __init__(self, *a, **kw):
            pass

        def dev_alloc(self, nbytes):
            allocs.append(nbytes)
            return 4096 * len(allocs)

        def detect_llr_rows(self, *a, **kw):
            calls.append(kw)
            return "rows", "mbs"

        def calibrate_i16(self, *a):
            calls.append("calibrate")

        def copy_wait(self, j):
            pass

    assert inspect.signature(lib.Engine.detect_llr_rows).parameters["resegment"].default is False
    assert "debug_resegment" in vars(lib.Engine)
    monkeypatch.setattr(lib, "Engine", Eng)
    spc = R.spc_of()
    off = pipeline.HostPipeline(spc, 8, R.M, primary="llr", int16_input=True)
    on = pipeline.HostPipeline(spc, 8, R.M, primary="llr", int16_input=True, resegment=True)
    assert off.native_i16 and off.dsig16 is None and not on.native_i16 and on.dsig16 is not None and on.resegment and not off.resegment
    assert inspect.signature(pipeline.native_int16_plan).parameters.keys() == {"primary", "int16_input", "m", "flag_truncated"}
    # the slot's call: calibrated to float32 first, then detect_llr_rows with the option
    on.slots[0] = {"ds": 1 << 20, "dl": 2 << 20, "dcal": 3 << 20, "lens": np.zeros(8, dtype=np.int32)}
    assert on._detect(0, 8) == ("rows", "mbs")
    assert calls[0] == "calibrate" and calls[1]["resegment"] is True and calls[1]["flag_truncated"] is False and calls[1]["device_ptrs"] is True
    plain = pipeline.HostPipeline(spc, 8, R.M, primary="llr")
    plain.slots[0] = dict(on.slots[0])
    plain._detect(0, 8)
    assert calls[-1]["resegment"] is False
    with pytest.raises(ValueError, match="LLR primary"):
        pipeline.HostPipeline(spc, 8, R.M, primary="cnn", resegment=True)
    with pytest.raises(ValueError, match="truncation look"):
        pipeline.HostPipeline(spc, 8, R.M, primary="llr", resegment=True, flag_truncated=True)
    over = R.spc_of()
    over.mvs_polya.mvs_detect_overwrite = True
    with pytest.raises(ValueError, match="mvs_detect_overwrite"):
        pipeline.HostPipeline(over, 8, R.M, primary="llr", resegment=True)
    assert lib.resegment_unsupported(R.spc_of()) is None
    assert inspect.signature(pipeline.HostPipeline.__init__).parameters["resegment"].default is False
    assert list(inspect.signature(combined.combined_detect_llr2_resegment).parameters) == ["batch_of_signals", "full_signal_lens", "spc", "device"]
    assert list(inspect.signature(combined.combined_detect_llr2).parameters) == ["batch_of_signals", "full_signal_lens", "spc", "device", "with_start_peak",
                                                                                "flag_truncated"]
