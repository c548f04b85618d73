"""The host side of the packed event calls and of `adapted events` (adp_segment_events_packed, adp_event_levels_packed,
adapted_amd/events_command.py), without a GPU: the new header against its prototype table and its flag against every other, the
command's refusals -- each before the library is loaded and with nothing created --, and the command's record path against
detect's builders."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["adp_event_levels_packed", "adp_segment_events_packed"]


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(os.path.join(ROOT, "include", "adapted_hip_events_packed.h"))
    assert sorted(declared) == sorted(lib.EVENT_PACKED_PROTOTYPES) == NAMES
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    at = [text.index('#include "adapted_hip_%s.h"' % h) for h in ("fingerprint", "events_packed", "adapter_front")]
    assert at == sorted(at) and text.index('extern "C"') < at[0]  # (behind adapted_hip_fingerprint.h, inside the extern "C" block)
    L = lib.load()
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.EVENT_PACKED_PROTOTYPES[name].split(":")
        assert got_ret.strip() == ret == "int" and got_params.split() == params, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for q, t in zip(params, fn.argtypes):
            if q in lib._SCALARS:
                assert t is lib._SCALARS[q], (name, q)
            elif q[:-1] in lib._ELEMENTS:
                assert isinstance(t, lib._Pointer) and t.element == q[:-1], (name, q)
            elif q == "adp_event_args*":
                assert t is ctypes.POINTER(lib.AdpEventArgs), (name, q)
            else:
                assert t is ctypes.c_void_p and q == "adp_handle*", (name, q)
    # the packed forms are the matrix forms with (packed, offsets, scale, offset) for (sig, len, n_reads, L, segs)
    for packed, matrix, table in (("adp_segment_events_packed", "adp_segment_events", lib.EVENT_PROTOTYPES),
                                  ("adp_event_levels_packed", "adp_event_levels", lib.FINGERPRINT_PROTOTYPES)):
        p, q = lib.EVENT_PACKED_PROTOTYPES[packed].split(":")[1].split(), table[matrix].split(":")[1].split()
        assert p[:5] == ["adp_handle*", "void*", "int64*", "float*", "float*"] and p[5:] == q[6:], packed


def test_the_new_table_is_disjoint_from_every_other():
    from adapted_amd import lib

    others = [getattr(lib, k) for k in dir(lib) if k.endswith("PROTOTYPES") and k != "EVENT_PACKED_PROTOTYPES"]
    assert len(others) >= 13 and lib.PROTOTYPES in others
    for table in others:
        assert not set(lib.EVENT_PACKED_PROTOTYPES) & set(table)
    assert not set(lib.EVENT_PACKED_PROTOTYPES) & set(lib.EXPORTS)


def _flags():
    """every ``#define ADP_NAME value`` of include/*.h whose value is a number or a shift -> {name: (header, value)}"""
    out = {}
    inc = os.path.join(ROOT, "include")
    for f in sorted(os.listdir(inc)):
        with open(os.path.join(inc, f)) as fh:
            for name, value in re.findall(r"^#define (ADP_\w+) +\(?((?:0x[0-9a-fA-F]+|\d+)u?(?: *<< *\d+)?)\)?", fh.read(), re.M):
                out[name] = (f, eval(value.replace("u", "")))  # noqa: S307 -- digits and a shift
    return out


def test_the_flag_bit_collides_with_no_other_flag():
    from adapted_amd import lib

    defs = _flags()
    assert defs["ADP_PACKED_I16"] == ("adapted_hip_events_packed.h", lib.ADP_PACKED_I16) and lib.ADP_PACKED_I16 == 1 << 24
    # the words a `flags` argument takes (the other numeric macros are sizes, statuses and row bits, not flags of a call)
    flags = ["ADP_IN_DEVICE", "ADP_OUT_DEVICE", "ADP_WITH_START_PEAK", "ADP_TOPK_NONE", "ADP_BOUNDS_HOST", "ADP_TAILS_NAN", "ADP_TRACE_FROM_SUMS",
             "ADP_CLLR_POLYA", "ADP_CLLR_F32", "ADP_LLR_INTERP", "ADP_LLR_GIVEN_PEAK", "ADP_MVS_F64", "ADP_SS_NANSKIP", "ADP_SS_WHOLE",
             "ADP_SS_CLIP", "ADP_SS_FORCE_GRID", "ADP_SS_FORCE_WAVE", "ADP_CNN_FALLBACK", "ADP_CNN_SECOND_LLR", "ADP_FLAG_TRUNCATED",
             "ADP_POLYA_TRUNCATED", "ADP_LLR_RESEGMENT", "ADP_KNN_NO_PRUNE", "ADP_CNN_SECOND_RESEGMENT"]
    used = 0
    for name in flags:
        v = defs[name][1]
        assert v & (v - 1) == 0 and not used & v, name  # (one bit each, no two alike)
        used |= v
    assert not used & lib.ADP_PACKED_I16
    assert used == (1 << 24) - 1  # (bits 0 .. 23 are taken: the new flag has the first free one)
    # and no numeric macro of any header is a shift to that bit or beyond
    for name, (f, v) in defs.items():
        assert name == "ADP_PACKED_I16" or v < (1 << 24), (name, f)
    # adapted_hip.h spells no call of the new names (tests/test_host_cpu.py takes every adp_name( there for a core export)
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert not re.search(r"adp_(segment_events|event_levels)_packed\s*\(", text)


def test_lds_arrays_of_the_event_kernels_stay_16_byte_aligned():
    for f in ("events_api.h", "fingerprint_api.h"):
        with open(os.path.join(ROOT, "adapted_amd", "csrc", f)) as fh:
            for line in fh:
                if "__shared__" in line:
                    assert "__attribute__((aligned(16)))" in line, (f, line)


def test_engine_signatures_and_the_empty_batch():
    from adapted_amd import fingerprint, lib, polya_length

    assert list(inspect.signature(lib.Engine.segment_events_packed).parameters) == ["self", "packed", "offsets", "args", "cap", "scale", "offset"]
    assert list(inspect.signature(lib.Engine.event_levels_packed).parameters) == ["self", "packed", "offsets", "args", "max_events", "scale", "offset",
                                                                                 "fp_ptr", "count_ptr"]
    eng = lib.Engine.__new__(lib.Engine)  # (no handle: the library is not entered)
    eng._h = lib._VoidP()
    a = lib.AdpEventArgs(16.0, 1e-3, 8, 8)
    pos, info, stats = eng.segment_events_packed(np.zeros(0, dtype=np.float32), [0], a, cap=3)
    assert pos.shape == (0, 3) and info.shape == (0, 2) and stats.shape == (0, 2) and pos.dtype == info.dtype == np.int64
    r = eng.event_levels_packed(np.zeros(4, dtype=np.int16), [2], a, 5, scale=[], offset=[])
    assert r["fingerprints"].shape == r["levels"].shape == (0, 5) and r["count"].shape == (0,) and r["lengths"].dtype == np.int32
    for bad, say in ((dict(packed=np.zeros(4, dtype=np.float64), offsets=[0, 4]), "float32 or int16"),
                     (dict(packed=np.zeros(4, dtype=np.int16), offsets=[0, 4]), "scale and an offset"),
                     (dict(packed=np.zeros(4, dtype=np.float32), offsets=[0, 5]), "offsets"),
                     (dict(packed=np.zeros(4, dtype=np.float32), offsets=[3, 2]), "offsets"),
                     (dict(packed=np.zeros(4, dtype=np.int16), offsets=[0, 4], scale=[1.0]), "go together"),
                     (dict(packed=np.zeros(4, dtype=np.int16), offsets=[0, 2, 4], scale=[1.0], offset=[0.0]), "one entry per read")):
        with pytest.raises(ValueError, match=say):
            eng.segment_events_packed(bad.pop("packed"), bad.pop("offsets"), a, **bad)
    assert callable(polya_length.segment_events_packed) and callable(fingerprint.event_levels_packed)
    assert polya_length.segment_events_packed(np.zeros(0, dtype=np.float32), [0])[0].shape == (0, 0)
    assert fingerprint.event_levels_packed(np.zeros(0, dtype=np.float32), [0], fingerprint.FingerprintParams(7)).fingerprints.shape == (0, 7)


def test_null_handle_and_wrong_types_never_enter_the_library():
    from adapted_amd import lib

    L = lib.load()
    a = lib.AdpEventArgs(16.0, 1e-3, 8, 8)
    off = np.zeros(2, dtype=np.int64)
    assert L.adp_segment_events_packed(None, None, off, None, None, 1, ctypes.byref(a), 0, 0, None, None, None) == -1  # ADP_ERR_INVALID
    assert b"bad argument" in L.adp_last_error()
    assert L.adp_event_levels_packed(None, None, off, None, None, 1, ctypes.byref(a), 0, 4, None, None, None, None, None, None, None, None) == -1
    with pytest.raises(ctypes.ArgumentError):  # int32 for int64 *offsets
        L.adp_segment_events_packed(None, None, np.zeros(2, dtype=np.int32), None, None, 1, ctypes.byref(a), 0, 0, None, None, None)
    with pytest.raises(ctypes.ArgumentError):  # float64 for float *scale
        L.adp_segment_events_packed(None, None, off, np.zeros(1), None, 1, ctypes.byref(a), 0, 0, None, None, None)


# ---- the command

def _rows():
    from adapted_amd.container_types import DetectResults

    return ["a", "b", "c"], [
        DetectResults(success=True, adapter_start=10, adapter_end=610, adapter_len=600, polya_end=1810, polya_len=1200, polya_truncated=True),
        DetectResults(success=True, adapter_start=None, adapter_end=300, adapter_len=300, polya_end=400, polya_len=100, polya_truncated=False),
        DetectResults(success=True, adapter_start=7, adapter_end=2007, adapter_len=2000, polya_end=2500, polya_len=493)]


def _run_dir(path, batch=2):
    """a run directory whose detected_boundaries_<k>.csv files _Writer wrote of _rows()"""
    from adapted_amd import main
    from adapted_amd.container_types import ReadResult

    ids, res = _rows()
    w = main._Writer(str(path), batch)
    w.add([ReadResult(read_id=i, success=True, detect_results=r) for i, r in zip(ids, res)])
    w.close()
    return str(path)


def test_the_subcommand_parses():
    from adapted_amd import main

    a = main.build_parser().parse_args(["events", "RUN", "-i", "x.npz", "y.npz", "-o", "OUT"])
    assert (a.mode, a.run_dir, a.input, a.output) == ("events", "RUN", ["x.npz", "y.npz"], "OUT")
    assert (a.polya_length, a.adapter_nt, a.fingerprints, a.barcode_templates, a.dtw_band, a.event_params) == (None,) * 6
    assert (a.int16_ingest, a.force, a.device) == (False, False, 0)
    a = main.build_parser().parse_args(["events", "RUN", "-i", "x", "-o", "OUT", "--polya_length", "adapter", "--adapter_nt", "60", "--fingerprints",
                                        "16", "--barcode_templates", "T.npz", "--dtw_band", "3", "--event_params", "4,4,9", "--int16_ingest",
                                        "--force", "--device", "1"])
    assert (a.polya_length, a.adapter_nt, a.fingerprints, a.barcode_templates, a.dtw_band, a.event_params, a.int16_ingest, a.force, a.device) == \
        ("adapter", 60.0, 16, "T.npz", 3, "4,4,9", True, True, 1)
    for bad in (["events", "-i", "x", "-o", "OUT"], ["events", "RUN", "-o", "OUT"], ["events", "RUN", "-i", "x"],
                ["events", "RUN", "-i", "x", "-o", "OUT", "--polya_length", "median"]):
        with pytest.raises(SystemExit):
            main.build_parser().parse_args(bad)


def _tree(path):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs) + sorted(os.path.join(d, s) for d, ss, _ in os.walk(path) for s in ss)


def test_every_refusal_has_its_message_loads_no_library_and_creates_nothing(tmp_path, monkeypatch):
    from adapted_amd import lib, main

    def no_library():
        pytest.fail("a refusal reached lib.load()")

    monkeypatch.setattr(lib, "load", no_library)
    monkeypatch.setattr(lib, "_LIB", None)
    run = _run_dir(tmp_path / "run")
    np.savez(tmp_path / "reads_0.npz", signals=np.zeros((3, 2600), dtype=np.float32), full_lengths=[2600] * 3, read_ids=np.array(["a", "b", "c"], dtype=object))
    np.savez(tmp_path / "not_templates.npz", x=np.zeros(3))
    reads, out = str(tmp_path / "reads_0.npz"), str(tmp_path / "out")
    (tmp_path / "no_run").mkdir()
    (tmp_path / "empty_run" / "boundaries").mkdir(parents=True)
    (tmp_path / "short_run" / "boundaries").mkdir(parents=True)
    with open(os.path.join(run, "boundaries", "detected_boundaries_0.csv")) as fh:
        lines = fh.read().splitlines()
    at = lines[0].split(",").index("polya_end")
    (tmp_path / "short_run" / "boundaries" / "detected_boundaries_0.csv").write_text(
        "\n".join(",".join(c for j, c in enumerate(ln.split(",")) if j != at) for ln in lines) + "\n")
    (tmp_path / "taken" / "polya_length").mkdir(parents=True)
    (tmp_path / "taken" / "polya_length" / "polya_length_1.csv").write_text("x\n")
    (tmp_path / "no_reads").mkdir()
    before = _tree(tmp_path)
    base = ["events", run, "-i", reads, "-o", out]
    pl = ["--polya_length", "events"]
    cases = [
        (base, "give --polya_length, --fingerprints or both"),
        (base + ["--adapter_nt", "60"], "give --polya_length, --fingerprints or both"),
        (base + ["--fingerprints", "16", "--adapter_nt", "60"], "go with --polya_length"),
        (base + ["--polya_length", "adapter"], "--adapter_nt"),
        (base + ["--polya_length", "adapter", "--adapter_nt", "0"], "--adapter_nt must be > 0"),
        (base + pl + ["--event_params", "1,8,16"], "window must lie in [2, 64]"),
        (base + pl + ["--barcode_templates", "T.npz"], "go with --fingerprints"),
        (base + pl + ["--dtw_band", "2"], "go with --fingerprints"),
        (base + ["--fingerprints", "1"], "must lie in [2, 512]"),
        (base + ["--fingerprints", "513"], "must lie in [2, 512]"),
        (base + ["--fingerprints", "16", "--dtw_band", "2"], "--dtw_band goes with --barcode_templates"),
        (base + ["--fingerprints", "16", "--event_params", "8,0,16"], "min_distance must be >= 1"),
        (base + ["--fingerprints", "16", "--barcode_templates", str(tmp_path / "not_templates.npz")], "not a template file"),
        (base + pl + ["--device", "-1"], "--device must be >= 0"),
        (["events", str(tmp_path / "no_run"), "-i", reads, "-o", out] + pl, "no boundaries/ directory"),
        (["events", str(tmp_path / "empty_run"), "-i", reads, "-o", out] + pl, "no detected_boundaries_<k>.csv"),
        (["events", str(tmp_path / "short_run"), "-i", reads, "-o", out] + pl, "has no column polya_end"),
        (["events", run, "-i", str(tmp_path / "no_reads"), "-o", out] + pl, "no valid input files"),
        (["events", run, "-i", reads, "-o", str(tmp_path / "taken")] + pl, "polya_length_1.csv exists"),
    ]
    for argv, say in cases:
        with pytest.raises(SystemExit) as e:
            main.main(argv)
        assert say in str(e.value), (argv, e.value)
        assert _tree(tmp_path) == before, argv
    # the two refusals of detect this command lifts are not made: --int16_ingest passes the option rules (and ends at the next one)
    with pytest.raises(SystemExit) as e:
        main.main(["events", str(tmp_path / "no_run"), "-i", reads, "-o", out, "--int16_ingest", "--fingerprints", "16"] + pl)
    assert "no boundaries/ directory" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        main.main(base + pl)
    assert "one GPU" in str(e.value) and "WORLD_SIZE is 2" in str(e.value)
    assert _tree(tmp_path) == before


def test_the_run_files_are_read_back_as_detect_held_them(tmp_path):
    from adapted_amd import events_command as ec

    run = _run_dir(tmp_path / "run")
    found = ec.find_run_files(run)
    assert [k for k, _ in found] == [0, 1]
    files = [ec.read_run_file(k, p) for k, p in found]
    ids, res = _rows()
    assert [rf.ids for rf in files] == [ids[:2], ids[2:]]
    got = [r for rf in files for r in rf.results]
    for g, w in zip(got, res):
        for col in ("adapter_start", "adapter_end", "adapter_len", "polya_end", "polya_len", "polya_truncated"):
            assert getattr(g, col) == getattr(w, col) and type(getattr(g, col)) is type(getattr(w, col)), col
    assert files[0].starts.tolist() == [10, 0] and files[0].ends.tolist() == [610, 300]  # (no adapter_start counts as 0)
    assert files[1].starts.tolist() == [7] and files[1].ends.tolist() == [2007]


def test_the_record_path_is_detects(tmp_path):
    """from the CSV files _Writer wrote and hand-made event arrays, the command's records are polya_length_records /
    fingerprint_records on the original values, and the files its writers make of them are _Writer's"""
    from adapted_amd import events_command as ec
    from adapted_amd import main, pipeline
    from adapted_amd.container_types import ReadResult

    ids, res = _rows()
    run = _run_dir(tmp_path / "run", batch=4)
    (rf,) = [ec.read_run_file(k, p) for k, p in ec.find_run_files(run)]
    E = 4
    ev = np.zeros(3, dtype=pipeline.EVENT_DTYPE)
    ev["n_bound"], ev["status"], ev["med"], ev["mad"] = [21, 1, 0], [0, 0, 2], [30.5, np.nan, np.nan], [4.25, np.nan, np.nan]
    fp = pipeline.AdapterFingerprints(3, E, True)
    fp.count[:], fp.status[:] = [4, 2, 0], [0, 4, 2]
    fp.lengths[:2] = [[100, 200, 150, 150], [100, 200, 0, 0]]
    fp.levels[0], fp.levels[1, :2] = [80.0, 95.5, 70.25, 101.0], [90.0, 90.0]
    fp.fingerprints[0] = [-0.5, 1.0, -1.25, 1.5]
    fp.best[:2], fp.bestdist[:2] = [[1, 0], [0, -1]], [[0.125, 2.5], [1 / 3, np.nan]]
    names = ["bc01", "bc02"]
    for method, nt in (("events", None), ("adapter", 60.0)):
        pl, fr = ec.file_records(rf, ev, fp, method, nt, names)
        assert _same(pl) == _same(main.polya_length_records(ids, res, ev, method, nt))
        want = main.fingerprint_records(ids, fp, names)
        assert len(fr) == len(want) == 3
        for g, w in zip(fr, want):
            assert list(g) == list(w) and _same(g["barcode"]) == _same(w["barcode"])
            for k in ("count", "status", "lengths", "levels", "fingerprints"):
                assert np.array_equal(g[k], w[k], equal_nan=True)
    only = ec.file_records(rf, ev, None, "events")
    assert _same(only[0]) == _same(main.polya_length_records(ids, res, ev, "events")) and only[1] is None
    assert ec.file_records(rf, ev, fp)[0] is None
    # the files: the command's writers are the blocks _Writer itself calls
    w = main._Writer(str(tmp_path / "direct"), 4, polya_length=True)
    w.enable_fingerprints(str(tmp_path / "direct"), E, barcodes=True)
    items = [ReadResult(read_id=i, success=True, detect_results=r) for i, r in zip(ids, res)]
    for it, a, b in zip(items, main.polya_length_records(ids, res, ev, "events"), main.fingerprint_records(ids, fp, names)):
        it.polya_length, it.fingerprint = a, b
    w.add(items)
    w.close()
    pl, fr = ec.file_records(rf, ev, fp, "events", None, names)
    for sub in ("polya_length", "fingerprints"):
        os.makedirs(tmp_path / "mine" / sub)
    main.write_polya_length_file(str(tmp_path / "mine" / "polya_length"), 0, pl)
    main.write_fingerprint_files(str(tmp_path / "mine" / "fingerprints"), 0, fr, E, True)
    for f in ("polya_length/polya_length_0.csv", "fingerprints/barcodes_0.csv"):
        assert (tmp_path / "mine" / f).read_bytes() == (tmp_path / "direct" / f).read_bytes(), f
    assert (tmp_path / "mine" / "polya_length" / "polya_length_0.csv").read_text().splitlines()[1] == "a,600,1200,20,30.5,4.25,30.5,39.344,True"
    with np.load(tmp_path / "mine" / "fingerprints" / "fingerprints_0.npz") as a, np.load(tmp_path / "direct" / "fingerprints" / "fingerprints_0.npz") as b:
        assert sorted(a.files) == sorted(b.files) == ["count", "fingerprints", "lengths", "levels", "read_id", "status"]
        for k in a.files:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    src = inspect.getsource(main._Writer._flush_extensions)
    assert "write_polya_length_file(" in src and "write_fingerprint_files(" in src and "to_csv" not in src and "savez" not in src


def _same(v):
    """records with NaN made comparable"""
    if isinstance(v, list):
        return [_same(x) for x in v]
    if isinstance(v, dict):
        return {k: _same(x) for k, x in v.items()}
    return "nan" if isinstance(v, float) and v != v else v
