"""The native CSV writer on the GPU (adp_format_rows through Engine.format_csv; kernels: adapted_amd/csrc/csv_api.h): every text is
held byte for byte against the pandas writer -- output.save_detected_boundaries on lib.rows_to_results of the same rows
(lib.rows_csv_text) -- and, for the goldens, against the reference's CSV text.  No tolerances."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import native_csv_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GOLDENS = sorted(os.path.basename(p)[:-len(".rows.json")] for p in glob.glob(os.path.join(GOLD, "*.rows.json")))
# the float32 columns (23, 25, 27) of the pass files: each one without a None in some file and with one in another
PASS_MODES = {"llr": {23: 0, 25: 0, 27: 1}, "cnn": {23: 1, 25: 0, 27: 0}, "start_peak": {23: 0, 25: 3, 27: 0}}


@pytest.fixture(scope="module")
def eng():
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.update_primary_method()
    spc.update_sig_preload_size()
    e = lib.Engine(spc, 1, spc.sig_preload_size, device=0)
    yield e
    e.close()


@pytest.mark.parametrize("fail", [False, True])
@pytest.mark.parametrize("primary", ["llr", "cnn", "start_peak"])
def test_random_rows(eng, primary, fail):
    """257 rows (more than four waves, odd) of every kind: second-opinion, truncated, re-segmented and exception rows, every column
    in a state of its own, the number rule's edge values, lists from None to beyond 1000 entries, read ids that need quotes"""
    from adapted_amd import lib

    seed = 100 + 2 * lib.PRIMARY_CODE[primary] + fail
    modes = {"cand": 3, "open_pores": 3}  # (lists of every kind in every file; the other columns' states are drawn)
    if not fail:
        modes.update(PASS_MODES[primary])
    rows, ids = cases.random_file(seed, 257, primary, fail, modes=modes)
    if not fail:  # the float32 columns are in the state the case set names
        for c, mode in PASS_MODES[primary].items():
            assert bool((rows["present"] >> np.uint64(c) & np.uint64(1)).all()) == (mode == 0)
    assert (rows["n_open_pores"] > lib.MAX_OPEN_PORES).any() and (rows["n_open_pores"] == 0).any() and (rows["n_cand"] == 16).any()
    assert any("," in i for i in ids)
    want = lib.rows_csv_text(rows, ids, primary, fail)
    assert b'"[' in want and b" ... " in want  # (a list that wraps: numpy breaks the line and csv quotes the field; a summarised one)
    got, n_fallback = eng.format_csv_native(rows, ids, primary, fail)
    assert n_fallback == 0
    assert got == want
    before = (eng.csv_files, eng.csv_fallback_files)
    assert eng.format_csv(rows, ids, primary, fail) == want and (eng.csv_files, eng.csv_fallback_files) == (before[0] + 1, before[1])


def test_values_at_and_above_the_bounds_are_counted_and_the_file_goes_through_pandas(eng):
    from adapted_amd import lib

    rows, ids = cases.random_file(8, 300, "llr", False)
    hit = cases.planted(rows)
    assert len(hit) == 7
    want = lib.rows_csv_text(rows, ids, "llr", False)
    _, n_fallback = eng.format_csv_native(rows, ids, "llr", False)
    assert n_fallback == len(hit)
    before = (eng.csv_files, eng.csv_fallback_files)
    assert eng.format_csv(rows, ids, "llr", False) == want
    assert (eng.csv_files, eng.csv_fallback_files) == (before[0] + 1, before[1] + 1)
    # without the planted rows the same file is inside the bounds
    keep = np.asarray([i for i in range(rows.size) if i not in hit])
    got, n_fallback = eng.format_csv_native(rows[keep], [ids[i] for i in keep], "llr", False)
    assert n_fallback == 0 and got == lib.rows_csv_text(rows[keep], [ids[i] for i in keep], "llr", False)


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(eng, name):
    """every golden row case: the GPU's text equals the pandas writer's on the same rows and, where the golden carries the
    reference's CSV text, that text"""
    from adapted_amd import lib

    rows, ids, primary = cases.rows_from_golden(GOLD, name)
    for fail in (False, True):
        sel = np.flatnonzero((rows["success"] != 0) != fail)
        r, i = rows[sel], [ids[k] for k in sel]
        want = lib.rows_csv_text(r, i, primary, fail)
        ref = os.path.join(GOLD, name + (".fail.csv" if fail else ".pass.csv"))
        if os.path.exists(ref):
            with open(ref, "rb") as fh:
                assert fh.read() == want, (name, fail)
        got, n_fallback = eng.format_csv_native(r, i, primary, fail)
        assert n_fallback == 0 and got == want, (name, fail)


def test_some_golden_carries_the_references_text():
    assert len(GOLDENS) >= 50 and sum(os.path.exists(os.path.join(GOLD, n + ".pass.csv")) for n in GOLDENS) >= 9


def test_no_row_one_row_and_a_file_of_exception_rows(eng):
    from adapted_amd import lib

    for n in (0, 1):
        for fail in (False, True):
            rows, ids = cases.random_file(5 + n, n, "llr", fail)
            rows["fail_code"] = 3 if fail else 0
            got, n_fallback = eng.format_csv_native(rows, ids, "llr", fail)
            assert n_fallback == 0 and got == lib.rows_csv_text(rows, ids, "llr", fail)
            assert n == 1 or got == b"\n"
    rows, ids = cases.random_file(7, 40, "cnn", True)
    rows["fail_code"] = 9 + np.arange(40) % 6
    got, n_fallback = eng.format_csv_native(rows, ids, "cnn", True)
    assert n_fallback == 0 and got == lib.rows_csv_text(rows, ids, "cnn", True) and got.count(b"\n") == 41
    # a text longer than the first buffer: the second call takes the length the first one reported
    rows, ids = cases.random_file(9, 3, "llr", False, modes={"open_pores": 0})
    for k in range(3):
        rows["n_open_pores"][k] = 900
        rows["open_pores_more"][k] = lib.register_open_pores(np.arange(900, dtype=np.int64) * 1000003)
    got, n_fallback = eng.format_csv_native(rows, ids, "llr", False)
    assert len(got) > 640 * 3 + 2048 + sum(len(i) for i in ids) and n_fallback == 0 and got == lib.rows_csv_text(rows, ids, "llr", False)


def test_bad_arguments_are_refused_before_anything_is_launched(eng):
    from adapted_amd import lib

    rows, ids = cases.random_file(2, 5, "llr", True, modes={"open_pores": 2})
    for field, value in (("fail_code", 16), ("start_peak_type", 3), ("n_cand", 17), ("n_open_pores", 17)):
        bad = rows.copy()
        bad[field][2] = value
        bad["fail_code"][2] = value if field == "fail_code" else 3
        with pytest.raises(lib.HipLibraryError):
            if field == "n_open_pores":  # (a row that says it has more than it holds, and no list beside it)
                strings, off = lib.csv_string_table()
                zero = np.zeros(6, dtype=np.int64)
                eng._check(eng.lib.adp_format_rows(eng._h, bad, 5, 1, 0, np.zeros(1, dtype=np.uint8), zero, None, zero, strings, off, 69,
                                                   np.zeros(64, dtype=np.uint8), 64, np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int32)))
            else:
                eng.format_csv_native(bad, ids, "llr", True)
    got, _ = eng.format_csv_native(rows, ids, "llr", True)  # the handle stays usable
    assert got == lib.rows_csv_text(rows, ids, "llr", True)


# ---- `adapted detect --native_csv` against the same command without it

N = 150  # calls of 64 reads (-s 16, four minibatches a call) and files of 24: files straddle the calls


def _files(run_root):
    runs = [d for d in os.listdir(run_root) if d.startswith("adapted_")]
    assert len(runs) == 1, runs
    out = {}
    for d, _, names in os.walk(os.path.join(run_root, runs[0])):
        for f in names:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), os.path.join(run_root, runs[0]))] = fh.read()
    return out


def _same_run(plain, native):
    """every file of the two run directories: the data files and config.toml byte for byte, command.json up to the option itself
    and the output folder, an .npz file array for array (its zip container holds the time it was written); adapted.log holds
    times and rates and only has to be there in both or in neither"""
    import io

    assert plain.keys() == native.keys() and any(f.startswith("boundaries/") for f in plain) and any(f.startswith("failed_reads/") for f in plain)
    for f in plain:
        if f == "command.json":
            a, b = json.loads(plain[f]), json.loads(native[f])
            assert a.pop("native_csv") is False and b.pop("native_csv") is True
            a.pop("output"), b.pop("output")
            assert a == b
        elif f.endswith(".npz"):
            with np.load(io.BytesIO(plain[f])) as a, np.load(io.BytesIO(native[f])) as b:
                assert sorted(a.files) == sorted(b.files) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a.files), f
        elif f != "adapted.log":
            assert plain[f] == native[f], f


@pytest.fixture(scope="module")
def bundles(tmp_path_factory):
    from adapted_amd import synth
    from adapted_amd.config import get_chemistry_specific_config

    tmp = tmp_path_factory.mktemp("native_csv_cli")
    spc = get_chemistry_specific_config("RNA004")
    spc.update_primary_method()
    spc.update_sig_preload_size()
    m = spc.sig_preload_size
    lens = np.array([m + 300 if i % 3 == 0 else max(1012, synth.pareto_length(9, i, lo=2000, hi=2 * m)) for i in range(N)], dtype=np.int32)
    sig, lens = synth.synth_batch(71, 0, N, m, lens)
    for j in range(24):
        sig[4, 120 + 40 * j: 123 + 40 * j] = 260.0  # more open pores than a row holds
    ids = np.array(["read_%04d" % i for i in range(N)], dtype=object)
    ids[7] = "read,with,commas"
    np.savez(tmp / "reads_0.npz", signals=sig, full_lengths=lens, read_ids=ids)
    scale, offset = np.full(N, 0.18, dtype=np.float32), np.full(N, -12.0, dtype=np.float32)
    raw = np.clip(np.round(np.nan_to_num(sig) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
    np.savez(tmp / "raw_0.npz", raw=raw, scale=scale, offset=offset, full_lengths=lens, read_ids=ids)
    cfgs = {}
    for primary in ("llr", "start_peak"):
        p = get_chemistry_specific_config("RNA004")
        p.llr_boundaries.llr_detect = primary == "llr"
        p.cnn_boundaries.cnn_detect = False
        p.rna_start_peak.detect_rna_start_peak = primary == "start_peak"
        if primary == "start_peak":  # (the settings under which that primary passes reads: tests/golden_cases.py)
            p.mvs_polya.mvs_detect_check, p.med_shift.detect_med_shift = False, True
        p.update_primary_method()
        p.update_sig_preload_size()
        assert p.primary_method == primary
        cfgs[primary] = str(tmp / (primary + ".toml"))
        p.to_toml(cfgs[primary])
        if primary == "llr":
            assert p.sig_preload_size == m  # (the bundles' width)
        else:  # whole reads of that configuration's window
            full, full_lens = synth.synth_batch(18, 0, N, p.sig_preload_size)
            np.savez(tmp / "full_0.npz", signals=full, full_lengths=full_lens, read_ids=ids)
    return tmp, cfgs


CONFIGS = {
    "llr_resegment": ("reads_0.npz", "llr", ["--llr_resegment", "--start_peak"]),
    "cnn_second_opinion": ("reads_0.npz", None, ["--second_opinion", "llr", "--start_peak", "--flag_truncated"]),
    "start_peak": ("full_0.npz", "start_peak", []),
    "int16": ("raw_0.npz", "llr", ["--int16_ingest"]),
    "extensions": ("reads_0.npz", "llr", ["--polya_length", "events", "--fingerprints", "24"]),
}


def _argv(tmp, cfgs, name, out):
    bundle, cfg, extra = CONFIGS[name]
    return (["detect", "-i", str(tmp / bundle), "-o", str(out)] + (["--config", cfgs[cfg]] if cfg else ["-c", "RNA004"])
            + ["-s", "16", "-b", "24"] + extra)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cli_writes_the_same_run_directory(bundles, name, caplog):
    import logging

    from adapted_amd import main as cli

    tmp, cfgs = bundles
    cli.main(_argv(tmp, cfgs, name, tmp / (name + "_plain")))
    with caplog.at_level(logging.INFO):
        cli.main(_argv(tmp, cfgs, name, tmp / (name + "_native")) + ["--native_csv"])
    plain, native = _files(str(tmp / (name + "_plain"))), _files(str(tmp / (name + "_native")))
    _same_run(plain, native)
    n_files = sum(f.startswith(("boundaries/", "failed_reads/")) for f in native)
    assert n_files >= 7  # (150 reads in files of 24: at least seven, across three detect calls)
    assert "native CSV: %d files, 0 through pandas" % n_files in caplog.text
    if name == "extensions":
        assert any(f.startswith("polya_length/") for f in native) and any(f.startswith("fingerprints/") for f in native)


def test_cli_two_ranks_write_the_one_rank_files(bundles):
    """two ranks under torchrun (gloo rendezvous, both on this box's GPU) with --native_csv: rank 0 formats the gathered rows, and
    the files equal those of the one-rank run without the option"""
    from adapted_amd import main as cli

    tmp, cfgs = bundles
    plain_root = tmp / "llr_resegment_plain"
    if not plain_root.exists():
        cli.main(_argv(tmp, cfgs, "llr_resegment", plain_root))
    env = dict(os.environ, PYTHONPATH=ROOT, ADAPTED_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29743",
           "-m", "adapted_amd.main"] + _argv(tmp, cfgs, "llr_resegment", tmp / "two_ranks") + ["--native_csv"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    one, two = _files(str(plain_root)), _files(str(tmp / "two_ranks"))
    data = lambda files: {f: v for f, v in files.items() if f.startswith(("boundaries/", "failed_reads/"))}
    assert data(one) == data(two) and len(data(one)) >= 7
    assert "native CSV: %d files, 0 through pandas" % len(data(two)) in two["adapted.log"].decode()
