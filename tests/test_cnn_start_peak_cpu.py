"""The start-peak columns of the CNN primary (ADP_WITH_START_PEAK on adp_detect_cnn): what can be checked without a GPU -- the
overlay rule the GPU tests expect against the oracle's own LLR extension, the inputs' preconditions, the refusals of the host-side
variants before an engine is looked at, the new keyword through the layers, and the command line's help."""
import inspect
import math

import numpy as np
import pytest

import cnn_start_peak_cases as sc
from util import load_case


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b and type(a) is type(b)


@pytest.mark.parametrize("name,n,invalid", [("rna004_llr_default", 96, 14), ("rna004_llr_nan_holes", 24, None)])
def test_overlay_rule_equals_the_oracles_llr_extension(name, n, invalid, oracle_mod):
    _, spc, sig, lens, _ = load_case(name)
    assert sig.shape[0] == n
    tab = oracle_mod.start_peak_table(sig, lens, spc)
    if invalid is not None:
        assert int((tab["valid"] == 0).sum()) == invalid, "precondition: reads without a K1 result"
    bare = oracle_mod.detect_llr(sig, lens, spc, with_start_peak=False)
    want = oracle_mod.detect_llr(sig, lens, spc, with_start_peak=True)
    assert any(w != b for w, b in zip(want, bare)), "precondition: the extension changes rows"
    got = sc.overlay_dicts(bare, tab)
    diffs = [(i, k, g.get(k), w.get(k)) for i, (g, w) in enumerate(zip(got, want)) for k in set(g) | set(w) if not _same(g.get(k), w.get(k))]
    assert not diffs, diffs[:8]
    # the bare rows hold none of the fields
    assert all(b.get(c) is None for b in bare for c in sc.SP_COLS + ["start_peak_open_pore_type"])


def test_input_preconditions(oracle_mod):
    spc, sig, lens = sc.inputs("default")
    t = sc.table(oracle_mod, "default", sig, lens, spc)
    assert sig.shape == (48, 17500) and (int(t["valid"].sum()), int((t["valid"] == 0).sum())) == (42, 6)
    assert int((lens < sig.shape[1]).sum()) == 19
    assert spc.primary_method == "cnn" and spc.cnn_boundaries.fallback_to_llr_short_reads
    assert spc.rna_start_peak.downscale_factor == spc.core.downscale_factor and spc.core.min_obs_adapter % spc.core.downscale_factor == 0

    spc, sig, lens = sc.inputs("200k")
    t = sc.table(oracle_mod, "200k", sig, lens, spc)
    assert sig.shape == (12, 201500) and (int(t["valid"].sum()), int((t["valid"] == 0).sum())) == (11, 1)

    spc, sig, lens = sc.inputs("sp200k")
    t = sc.table(oracle_mod, "sp200k", sig, lens, spc)
    assert sig.shape == (20, 201500) and t["valid"].all() and sorted(t["flagged_type"].tolist()) == [0] * 19 + [2]
    assert spc.primary_method == "cnn" and spc.core.max_obs_trace == 200000

    spc, sig, lens = sc.inputs("handmade", oracle_mod)
    t = sc.table(oracle_mod, "handmade", sig, lens, spc)
    assert t["valid"].all() and int((lens == 1012).sum()) >= 1
    assert all(t[r]["flagged_type"] == 1 and t[r]["has_open_pore"] for r in sc.HAND_TYPE1)
    assert all(t[r]["flagged_type"] == 2 and t[r]["has_open_pore"] for r in sc.HAND_TYPE2)
    assert [int(lens[r]) for r in sc.HAND_BEHIND] == [8000, 3000]
    assert all(t[r]["flagged_type"] == 0 and not t[r]["has_open_pore"] for r in sc.HAND_BEHIND)
    # with the shipped section type 1 is out of reach at this window: the scan for the successor starts behind the open-pore range
    # (the successor lies at block start_peak_max_idx + offset2 or later, the open pore among the first m // ds raw samples)
    sp = sc.inputs("default")[0].rna_start_peak
    nxt_min, op_max = sp.start_peak_max_idx + sp.offset2, (sig.shape[1] // sp.downscale_factor) // sp.downscale_factor
    assert nxt_min - op_max > 2.0 + 0.01 * op_max

    spc, sig, lens = sc.inputs("m16003")
    assert sig.shape[1] % spc.core.downscale_factor != 0 and sc.table(oracle_mod, "m16003", sig, lens, spc)["valid"].sum() >= 40


def test_overlay_rows_follows_the_same_rule():
    """exception rows stay bare, invalid results give nothing, the open-pore column comes with a flag only"""
    from adapted_amd import lib
    from oracle import oracle

    rows = lib.empty_rows(4)
    rows["present"] = [1, 1, 1, 1]
    rows["fail_code"] = [0, 11, 0, 5]
    tab = np.zeros(4, dtype=oracle.SP_DTYPE)
    tab["valid"] = [1, 1, 0, 1]
    tab["flagged_type"] = [0, 2, 1, 2]
    tab["has_open_pore"] = [0, 1, 1, 1]
    tab["start_peak_idx"], tab["next_greater_idx"], tab["open_pore_idx"] = 120, 2600, 1540
    tab["start_peak_pa"], tab["next_greater_pa"] = np.float32(101.3), np.float32(104.7)
    out = sc.overlay_rows(rows, tab)
    assert out[1].tobytes() == rows[1].tobytes() and out[2].tobytes() == rows[2].tobytes()
    v, typ = sc.sp_view(out)
    assert typ.tolist() == [0, 0, 0, 2]
    assert v[0, :4].tolist() == [120.0, float(np.float32(101.3)), 2600.0, float(np.float32(104.7))] and np.isnan(v[0, 4])
    assert v[3].tolist() == [120.0, float(np.float32(101.3)), 2600.0, float(np.float32(104.7)), 1540.0]
    assert out[3]["fail_code"] == 5 and out[3]["success"] == rows[3]["success"]
    res = lib.rows_to_results(out, "cnn")
    assert res[3].start_peak_open_pore_type == sc.SP_TYPES[2] and res[3].start_peak_open_pore_idx == 1540
    assert res[3].fail_reason == "No polya detected (primary)", "the +<flag> suffix belongs to the start-peak primary alone"
    assert res[0].start_peak_idx == 120 and res[0].start_peak_open_pore_type is None and res[0].start_peak_open_pore_idx is None
    assert res[1].start_peak_idx is None and res[2].start_peak_idx is None


def test_host_side_variants_refuse_the_option_before_the_engine_is_looked_at():
    from adapted_amd.detect import cnn

    sig, lens = np.zeros((1, 8), np.float32), np.zeros(1, np.int32)
    for fn in (cnn.detect_rows_start_peak, cnn.detect_rows_truncated, cnn.detect_rows_second_opinion):
        kw = {} if fn is cnn.detect_rows_start_peak else {"with_start_peak": True}
        with pytest.raises(ValueError, match="with_start_peak.*conv"):
            fn(None, sig, lens, None, None, conv="torch", **kw)
        with pytest.raises(ValueError, match="with_start_peak.*fallback"):
            fn(None, sig, lens, None, None, fallback="host", **kw)
    for fn in (cnn.detect_rows_device_start_peak, cnn.detect_rows_device_truncated, cnn.detect_rows_device_second_opinion):
        kw = {} if fn is cnn.detect_rows_device_start_peak else {"with_start_peak": True}
        with pytest.raises(ValueError, match="with_start_peak.*fallback"):
            fn(None, 0, 0, 1, lens, None, None, None, "host", **kw)
    with pytest.raises(ValueError, match="with_start_peak.*conv"):
        cnn.combined_detect_cnn(sig, lens, None, None, conv="torch", with_start_peak=True)


def test_the_keyword_through_the_layers():
    from adapted_amd import lib, main, pipeline
    from adapted_amd.detect import cnn, combined

    for fn in (lib.Engine.detect_cnn_rows, cnn.detect_rows_truncated, cnn.detect_rows_device_truncated, cnn.detect_rows_second_opinion,
               cnn.detect_rows_device_second_opinion, cnn.combined_detect_cnn, cnn.combined_detect_cnn_llr, combined.combined_detect_cnn,
               pipeline.HostPipeline.__init__):
        assert inspect.signature(fn).parameters["with_start_peak"].default is False, fn
    # the forms beside detect_rows / detect_rows_device, which keep the parameters they were introduced with
    assert list(inspect.signature(cnn.detect_rows_start_peak).parameters) == list(inspect.signature(cnn.detect_rows).parameters)
    assert list(inspect.signature(cnn.detect_rows_device_start_peak).parameters) == list(inspect.signature(cnn.detect_rows_device).parameters)
    assert "start_peak" in inspect.signature(main.run_detect).parameters
    assert lib.ADP_WITH_START_PEAK == 4


def test_pipeline_hands_the_option_to_the_cnn_primary():
    """HostPipeline._detect with the CNN primary passes with_start_peak down, and nothing else: read where the library is called (a
    bare engine whose library is a recorder, tests/call_recorder.py)"""
    from adapted_amd import lib, pipeline
    from call_recorder import detect_calls, names, recorder_engine

    spc = sc.inputs("default")[0]
    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.primary, p.with_start_peak, p.second_opinion, p.flag_truncated = "cnn", True, None, False
    p.native_i16 = p.ragged = p.i16 = False
    p.model, p.spc = None, spc
    p.mb = 16
    p.eng = recorder_engine(spc, 64)
    p.slots = [{"ds": 1, "dl": 2, "lens": np.zeros(16, np.int32)}]
    rows, mbs = p._detect(0, 16)
    assert rows.shape == (16,) and rows.dtype == lib.ROW_DTYPE and mbs is None
    assert names(p.eng) == ["adp_copy_wait", "adp_cnn_set_weights", "adp_detect_cnn"]
    (c,) = detect_calls(p.eng)
    # flag_truncated False, second_opinion False, with_start_peak True; the fallback inside the call, the rows resident
    assert c["flags"] == lib.ADP_IN_DEVICE | lib.ADP_CNN_FALLBACK | lib.ADP_WITH_START_PEAK
    assert c["head"] == (1, 2) and (c["n"], c["m"], c["minibatch"]) == (16, 64, 16) and c["bounds"] is None


def test_cli_help_names_both_primaries(capsys):
    from adapted_amd import main

    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["detect", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    i = text.rindex("--start_peak")  # (the option's own paragraph, behind the usage line)
    para = text[i:text.index("--second_opinion", i)]
    assert "CNN" in para and "LLR" in para and "start_peak_open_pore_type" in para
    args = main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004", "--start_peak"])
    assert args.start_peak is True and vars(args)["start_peak"] is True
