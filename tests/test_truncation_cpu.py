"""ADP_FLAG_TRUNCATED without a GPU: the case set of tests/truncation_cases.py through the restated rule (every outcome the GPU
tests rely on must occur), the reads the rule must never flag, and the Python / CLI layers (rows_to_results, the CSV text, the
`truncated` subcommand, the refusals)."""
import inspect
import os
import re
from collections import Counter

import numpy as np
import pytest

import truncation_cases as tc
import truncation_restated as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _llr_look(oracle_mod, m_trace, n, mb, first=0, full_len=None):
    spc = tc.spc_of("llr", m_trace)
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, n, first=first, full_len=full_len)
    rows = tr.llr_first_rows(oracle_mod, sig, lens, spc, mb, key=("cpu", m, n, first, full_len))
    return (sig, lens, rows) + tr.look(oracle_mod, sig, lens, rows, spc, "llr")


def test_the_case_set_holds_every_outcome(oracle_mod):
    """48 reads at the default window as two minibatches of 24 (what the GPU tests run): per group of r % 4 the outcome the
    case set was made for, each at least three times, and flagged reads from passing and from failing first rows"""
    sig, lens, first, exp, counts, kinds = _llr_look(oracle_mod, None, 48, 24)
    by_group = [Counter(kinds[g::4]) for g in range(4)]
    print("counts %s, outcomes per group %s" % (counts, by_group))
    assert by_group[0]["t1_failed"] >= 3 and by_group[1]["t2_failed"] >= 3 and by_group[2]["t1_failed"] >= 3 and by_group[3]["flagged"] >= 3
    assert not any(k == "flagged" for g in range(3) for k in kinds[g::4])
    origin = Counter(bool(first[r]["success"]) for r in range(48) if kinds[r] == "flagged")
    assert origin[True] >= 3 and origin[False] >= 3, origin
    assert counts == (sum(k != "ineligible" for k in kinds), sum(k in ("t2_failed", "flagged") for k in kinds), sum(k == "flagged" for k in kinds))
    for r in range(48):
        e = exp[r]
        if kinds[r] == "flagged":
            assert e["success"] and e["polya_truncated"] is True and e["polya_end"] == sig.shape[1] and e["_reserved"] == 6
            assert all(e[k] is None for k in tr.RNA_FIELDS)
            assert e["llr_polya_end"] == first[r]["llr_polya_end"] and e["polya_candidates"] == first[r]["polya_candidates"]
            assert e["polya_len"] == sig.shape[1] - e["adapter_end"]
        else:
            assert tr.public(e) == dict(tr.public(first[r]), polya_truncated=False if first[r]["success"] else None) and e["_reserved"] == 4


def test_group_2_fails_t1_through_the_nan_alone(oracle_mod):
    """the same reads without their five NaN are group 3's kind: the window's NaN is what fails T1"""
    spc = tc.spc_of("llr")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 48)
    r = 2
    first = oracle_mod.detect_llr(sig[:24], lens[:24], spc)[r]
    el = tr.eligible(first, int(lens[r]), m, spc, "llr")
    assert el is not None and not tr.t1(sig[r], el[1], el[2])
    clean = np.array(sig[r])
    assert np.isnan(clean[m - 300:m - 295]).all()
    clean[m - 300:m - 295] = 108.0
    assert tr.t1(clean, el[1], el[2])


@pytest.mark.parametrize("max_obs_trace", [16000, 40000])
def test_every_eligible_read_whose_polya_reaches_the_end_is_flagged(oracle_mod, max_obs_trace):
    n = 240
    sig, lens, first, exp, counts, kinds = _llr_look(oracle_mod, max_obs_trace, n, 48)
    el = [r for r in range(3, n, 4) if kinds[r] != "ineligible"]
    print("max_obs_trace %d: counts %s, eligible reads of group 3: %d" % (max_obs_trace, counts, len(el)))
    assert len(el) >= 3 and all(kinds[r] == "flagged" for r in el)
    assert not any(kinds[r] == "flagged" for r in range(n) if r % 4 != 3)


@pytest.mark.parametrize("short_by", [0, 700])
def test_a_read_that_ends_inside_its_polya_is_never_flagged(oracle_mod, short_by):
    """full_len == m and full_len < m: the poly(A) of groups 2 and 3 reaches the read's end, and the read was not cut by the preload"""
    m = tc.spc_of("llr").sig_preload_size
    sig, lens, first, exp, counts, kinds = _llr_look(oracle_mod, None, 24, 24, full_len=m - short_by)
    assert counts == (0, 0, 0) and set(kinds) == {"ineligible"}
    assert all(e["polya_truncated"] is not True and e["_reserved"] == 4 for e in exp)
    # the very same signals with a longer read behind them are flagged (the rule looks at full_len alone here)
    if short_by == 0:
        longer = np.full(24, m + 1, dtype=np.int32)
        _, c2, k2 = tr.look(oracle_mod, sig, longer, oracle_mod.detect_llr(sig, longer, tc.spc_of("llr")), tc.spc_of("llr"), "llr")
        assert c2[2] >= 3 and all(k == "flagged" for k in k2[3::4])


def test_cnn_case_set_has_flagged_and_unflagged_reads(oracle_mod):
    """the CNN primary on the same signals (CPU conv stack of the oracle, shipped weights); and the batch from read 192 on, where
    read 7 fails the CNN path, passes the LLR path and is flagged -- a second-opinion row that keeps bit 0"""
    spc = tc.spc_of("cnn")
    m = spc.sig_preload_size
    w = np.load(os.path.join(ROOT, "adapted_amd", "models", "rna004_130bps@v0.2.4.npz"))
    for first0, with_second in ((0, False), (192, True)):
        sig, lens = tc.batch(m, 48, first=first0)
        preds = oracle_mod.cnn_predict(oracle_mod.cnn_forward(oracle_mod.cnn_prepare(sig, spc), w), spc)
        rows = oracle_mod.detect_cnn_from_preds(sig, lens, preds, spc)
        if with_second:
            rows = tr.second_llr(rows, oracle_mod.detect_llr(sig, lens, tc.llr_copy(spc)))
        exp, counts, kinds = tr.look(oracle_mod, sig, lens, rows, spc, "cnn")
        print("reads from %d on: counts %s, %s" % (first0, counts, Counter(kinds)))
        assert sum(k == "flagged" for k in kinds) >= 3 and sum(k != "flagged" for k in kinds) >= 3
        if with_second:
            both = [r for r in range(48) if exp[r]["_reserved"] == 7]
            assert both and all(exp[r]["llr_adapter_end"] is not None and exp[r].get("cnn_adapter_end") is None for r in both), both


def _hand_made_rows():
    from adapted_amd import lib

    rows = lib.empty_rows(4)
    cols = ("{primary}_adapter_end", "{primary}_polya_end", "adapter_end", "polya_end", "rna_preloaded_start", "rna_preloaded_len", "rna_preloaded_med")
    for r in rows:
        for c, v in zip(cols, (3000, 5200, 3000, 17500, 17500, 10, 99.5)):
            r["col"][lib.COLS.index(c)] = v
        r["present"] = sum(1 << lib.COLS.index(c) for c in cols)
        r["n_cand"], r["n_open_pores"] = 0, 0
    rows["success"] = [1, 1, 0, 1]
    rows["fail_code"] = [0, 0, 5, 0]
    rows["reserved_"] = [lib.ROW_POLYA_TRUNCATED | lib.ROW_TRUNC_LOOKED, lib.ROW_TRUNC_LOOKED, lib.ROW_TRUNC_LOOKED, 0]
    return rows


def test_rows_to_results_for_the_bit_combinations():
    from adapted_amd import lib

    assert (lib.ADP_FLAG_TRUNCATED, lib.ADP_POLYA_TRUNCATED, lib.ROW_POLYA_TRUNCATED, lib.ROW_TRUNC_LOOKED) == (1 << 19, 1 << 20, 2, 4)
    flagged, looked, failed, plain = lib.rows_to_results(_hand_made_rows(), "llr")
    assert flagged.polya_truncated is True and flagged.polya_end == 17500 and flagged.llr_polya_end == 5200
    assert all(getattr(flagged, k) is None for k in tr.RNA_FIELDS)
    assert looked.polya_truncated is False and looked.rna_preloaded_start == 17500 and looked.rna_preloaded_len == 10
    assert failed.polya_truncated is None and failed.success is False
    assert plain.polya_truncated is None and plain.rna_preloaded_med == np.float32(99.5)


def test_csv_text_of_a_true_and_a_false_row(tmp_path):
    from adapted_amd import lib
    from adapted_amd.container_types import ReadResult
    from adapted_amd.output import CSV_COLUMNS, save_detected_boundaries

    res = lib.rows_to_results(_hand_made_rows(), "llr")
    fn = str(tmp_path / "detected_boundaries_0.csv")
    save_detected_boundaries([ReadResult(read_id="read-%d" % i, success=True, fail_reason=None, detect_results=r) for i, r in enumerate(res) if r.success], fn)
    with open(fn) as fh:
        lines = [ln.rstrip("\n").split(",") for ln in fh]
    assert lines[0] == CSV_COLUMNS
    at = lines[0].index("polya_truncated")
    assert at == 17  # (the reference's scripts/get_truncated.sh reads column 18)
    assert [ln[at] for ln in lines[1:]] == ["True", "False", ""]
    assert [ln[0] for ln in lines[1:]] == ["read-0", "read-1", "read-3"]


def test_truncated_subcommand(tmp_path, capsys):
    from adapted_amd import main

    run = tmp_path / "run"
    (run / "boundaries").mkdir(parents=True)
    # the column is found by name: another order, and a file index of two digits that sorts behind 2 only as a number
    (run / "boundaries" / "detected_boundaries_10.csv").write_text("read_id,polya_truncated,polya_end\nc,True,9\nd,False,9\n")
    (run / "boundaries" / "detected_boundaries_2.csv").write_text("polya_end,read_id,signal_len,polya_truncated\n5,a,100,True\n5,b,100,\n7,e,100,True\n")
    (run / "boundaries" / "other.csv").write_text("read_id,polya_truncated\nz,True\n")
    main.main(["truncated", str(run)])
    out = run / "boundaries" / "truncated_read_ids.csv"
    assert out.read_text() == "read_id\na\ne\nc\n"
    assert "3 reads" in capsys.readouterr().out
    # the boundaries folder itself, as the reference's script takes it
    out.unlink()
    assert main.list_truncated(str(run / "boundaries")) == 3 and out.read_text() == "read_id\na\ne\nc\n"
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(SystemExit) as e:
        main.main(["truncated", str(empty)])
    assert e.value.code == 1 and "No detected_boundaries" in capsys.readouterr().out
    assert not list(empty.iterdir())


def test_cli_takes_the_flag_and_records_it():
    from adapted_amd import main

    args = main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004", "--flag_truncated"])
    assert args.flag_truncated is True and vars(args)["flag_truncated"] is True  # (command.json is vars(args): `continue` repeats it)
    main._check_flag_truncated(args)
    assert main.build_parser().parse_args(["detect", "-i", "x.npz", "-c", "RNA004"]).flag_truncated is False
    assert "flag_truncated" in inspect.signature(main.run_detect).parameters


def _config(tmp_path, name, change):
    spc = tc.spc_of("llr")
    change(spc)
    spc.update_primary_method()
    fn = str(tmp_path / (name + ".toml"))
    spc.to_toml(fn)
    return fn


def _no_check(spc):
    spc.mvs_polya.mvs_detect_check = False


def _overwrite(spc):
    spc.mvs_polya.mvs_detect_overwrite = True


def _start_peak(spc):
    spc.llr_boundaries.llr_detect, spc.rna_start_peak.detect_rna_start_peak = False, True


def _long_window(spc):
    spc.mvs_polya.median_shift_window = 5000


@pytest.mark.parametrize("change,says", [(_no_check, "mvs_detect_check"), (_overwrite, "mvs_detect_overwrite"), (_start_peak, "primaries"),
                                         (_long_window, "median_shift_window")])
def test_cli_refuses_unsupported_configurations_before_anything_runs(tmp_path, change, says):
    from adapted_amd import main

    cfg = _config(tmp_path, "cfg", change)
    out = tmp_path / "out"
    out.mkdir()
    with pytest.raises(SystemExit) as e:
        main.main(["detect", "-i", str(tmp_path / "none.npz"), "-o", str(out), "--config", cfg, "--flag_truncated"])
    assert "--flag_truncated" in str(e.value) and says in str(e.value)
    assert not list(out.iterdir())  # no run directory was made


def test_pipeline_and_keywords():
    from adapted_amd import lib, pipeline
    from adapted_amd.detect import cnn, combined

    with pytest.raises(ValueError, match="primaries"):
        pipeline.HostPipeline(tc.spc_of("llr"), 16, 1024, primary="start_peak", flag_truncated=True)
    spc = tc.spc_of("llr")
    spc.mvs_polya.mvs_detect_overwrite = True
    with pytest.raises(ValueError, match="mvs_detect_overwrite"):
        pipeline.HostPipeline(spc, 16, 1024, primary="llr", flag_truncated=True)
    assert lib.truncation_unsupported(tc.spc_of("llr")) is None and lib.truncation_unsupported(tc.spc_of("cnn")) is None
    for fn in (lib.Engine.detect_llr_rows, lib.Engine.detect_cnn_rows, combined.combined_detect_llr2, combined.combined_detect_cnn,
               cnn.combined_detect_cnn, cnn.combined_detect_cnn_llr, pipeline.HostPipeline.__init__):
        assert inspect.signature(fn).parameters["flag_truncated"].default is False, fn
    assert inspect.signature(lib.Engine.validate_rows).parameters["polya_truncated"].default is False
    with pytest.raises(ValueError, match="conv"):
        cnn.detect_rows_truncated(None, np.zeros((1, 8), np.float32), np.zeros(1, np.int32), None, tc.spc_of("cnn"), conv="torch")


def test_header_names_the_flags_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        raw = fh.read()
    assert re.search(r"^#define\s+ADP_FLAG_TRUNCATED\s+\(1 << 19\)", raw, re.M) and re.search(r"^#define\s+ADP_POLYA_TRUNCATED\s+\(1 << 20\)", raw, re.M)
    assert re.search(r"^#define\s+ADP_ROW_POLYA_TRUNCATED\s+2\s*$", raw, re.M) and re.search(r"^#define\s+ADP_ROW_TRUNC_LOOKED\s+4\s*$", raw, re.M)
    assert re.search(r"^#define\s+ADP_ABI_VERSION\s+3\s*$", raw, re.M)
