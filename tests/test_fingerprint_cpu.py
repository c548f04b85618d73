"""The host side of the adapter event fingerprints and their DTW barcode assignment (adp_event_levels, adp_dtw_assign,
adapted_amd/fingerprint.py, `adapted detect --fingerprints`), without a GPU: the new header against its prototype table, the
refusals before launch, the oracle's own known answers worked by hand, the parameters, the template files, medoid_templates on a
fake distance function, the command line's refusals and the pipeline's method with a recording engine."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import events_oracle as eo
import fingerprint_oracle as fo
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adapted_hip_fingerprint.h")


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(HEADER)
    assert sorted(declared) == sorted(lib.FINGERPRINT_PROTOTYPES) == ["adp_dtw_assign", "adp_event_levels"]
    others = set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES) | set(lib.EVENT_PROTOTYPES) | set(lib.EXPORTS)
    assert not set(lib.FINGERPRINT_PROTOTYPES) & others
    assert sorted(lib.EVENT_PROTOTYPES) == ["adp_segment_events", "adp_sizeof_event_args"]
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_fingerprint.h"') == 1
    assert text.index('#include "adapted_hip_events.h"') < text.index('#include "adapted_hip_fingerprint.h"') < text.index("adp_set_profiling")
    assert len(_prototypes(os.path.join(ROOT, "include", "adapted_hip.h"))) == len(lib.PROTOTYPES) == 62
    L = lib.load()
    assert L.adp_abi_version() == 3
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.FINGERPRINT_PROTOTYPES[name].split(":")
        assert got_ret == ret and got_params.split() == params, name
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


def test_the_new_header_defines_no_numeric_macro_and_lib_restates_the_kernels_constants():
    from adapted_amd import lib

    with open(HEADER) as fh:
        defines = [ln.split()[1] for ln in fh if ln.startswith("#define")]
    assert defines == ["ADAPTED_HIP_FINGERPRINT_H"]
    with open(os.path.join(ROOT, "adapted_amd", "csrc", "fingerprint_api.h")) as fh:
        text = fh.read()
    assert int(re.search(r"#define FP_EMAX (\d+)", text).group(1)) == lib.FINGERPRINT_MAX_EVENTS == 512
    assert int(re.search(r"#define DTW_NT_MAX (\d+)", text).group(1)) == lib.DTW_MAX_TEMPLATES == 4096
    assert int(re.search(r"#define DTW_SCRATCH_MIB (\d+)", text).group(1)) == lib.DTW_SCRATCH_MIB == 512
    with open(os.path.join(ROOT, "adapted_amd", "csrc", "modules.hip")) as fh:
        entry = fh.read()
    # (the budget over the bytes of a row of the distance matrix: batch_rows states the division, adp_dtw_assign the row)
    assert 'getenv("ADP_DTW_SCRATCH_MIB")' in entry and "batch_rows(mib, nts * 8, nqs, nts)" in entry
    assert "size_t rows = ((size_t)mib << 20) / row_bytes;" in entry


def test_null_handle_is_refused_and_wrong_types_never_enter_the_library():
    from adapted_amd import lib

    L = lib.load()
    a = lib.AdpEventArgs(16.0, 1e-3, 8, 8)
    tail = (None,) * 8
    assert L.adp_event_levels(None, None, None, 1, 8, None, 1, ctypes.byref(a), 0, 16, *tail) == -1  # ADP_ERR_INVALID
    assert b"bad argument" in L.adp_last_error()
    assert L.adp_dtw_assign(None, None, None, 1, 8, None, None, 1, 8, 0, 0, None, None, None) == -1
    assert b"bad argument" in L.adp_last_error()
    segs = np.zeros(1, dtype=lib.SEG_DTYPE)
    with pytest.raises(ctypes.ArgumentError):  # int64 for int32 *count_out
        L.adp_event_levels(None, None, None, 1, 8, segs, 1, ctypes.byref(a), 0, 16, None, None, np.zeros(1, dtype=np.int64), None, None, None, None, None)
    with pytest.raises(ctypes.ArgumentError):  # float32 for double *fp_out
        L.adp_event_levels(None, None, None, 1, 8, segs, 1, ctypes.byref(a), 0, 16, None, None, None, None, None, None, np.zeros(16, dtype=np.float32), None)
    with pytest.raises(ctypes.ArgumentError):  # int64 for int32 *lengths_out
        L.adp_event_levels(None, None, None, 1, 8, segs, 1, ctypes.byref(a), 0, 16, None, None, None, None, np.zeros(16, dtype=np.int64), None, None, None)
    with pytest.raises(ctypes.ArgumentError):  # float32 queries
        L.adp_dtw_assign(None, np.zeros((1, 8), dtype=np.float32), None, 1, 8, None, None, 1, 8, 0, 0, None, None, None)
    with pytest.raises(ctypes.ArgumentError):  # int64 counts
        L.adp_dtw_assign(None, None, np.zeros(1, dtype=np.int64), 1, 8, None, None, 1, 8, 0, 0, None, None, None)
    with pytest.raises(ctypes.ArgumentError):  # int64 for int32 *best_out
        L.adp_dtw_assign(None, None, None, 1, 8, None, None, 1, 8, 0, 0, None, np.zeros(2, dtype=np.int64), None)


def test_empty_batches_have_empty_answers():
    from adapted_amd import fingerprint as fpm
    from adapted_amd import lib

    eng = lib.Engine.__new__(lib.Engine)  # (no handle: the library is not entered)
    eng._h = lib._VoidP()
    r = eng.event_levels(np.zeros((2, 8), dtype=np.float32), [8, 8], [], [], [], lib.AdpEventArgs(16.0, 1e-3, 8, 8), 16)
    assert r["info"].shape == (0, 2) and r["lengths"].shape == r["levels"].shape == r["fingerprints"].shape == (0, 16)
    assert r["count"].dtype == r["status"].dtype == r["lengths"].dtype == np.int32 and r["norm"].shape == (0, 2)
    dist, best, bd = eng.dtw_assign(np.zeros((0, 5)), [], np.zeros((3, 4)), [1, 2, 3])
    assert dist.shape == (0, 3) and best.shape == (0, 2) and bd.shape == (0, 2) and best.dtype == np.int32
    assert eng.dtw_assign(np.zeros((0, 5)), [], np.zeros((3, 4)), [1, 2, 3], want_dist=False)[0] is None
    e = fpm.event_levels_batch(np.zeros((2, 8), dtype=np.float32), [8, 8], ([], [], []), fpm.FingerprintParams(max_events=7))
    assert e.fingerprints.shape == (0, 7) and e.count.shape == (0,) and e.event_len_med.shape == (0,)
    assert fpm.dtw_distances(np.zeros((0, 5)), [], np.zeros((3, 4)), [1, 2, 3]).shape == (0, 3)
    a = fpm.assign_barcodes(np.zeros((0, 5)), [], fpm.Templates(["a"], np.zeros((1, 4)), np.asarray([2])))
    assert a.best.shape == a.margin.shape == (0,)
    assert list(inspect.signature(lib.Engine.event_levels).parameters)[:8] == ["self", "sig", "lens", "rows", "starts", "ends", "args", "max_events"]


def test_oracle_known_answers_worked_by_hand():
    # three plateaus: boundaries 40 and 80, levels 80, 120, 80; median 80, deviations 0, 40, 0: MAD 0 -> status 4
    x = np.repeat([80.0, 120.0, 80.0], 40)
    assert eo.segment(x)[0].tolist() == [40, 80]
    o = fo.levels(x, 16)
    assert (o["nk"], o["count"], o["status"]) == (2, 3, 4) and o["norm"] == (80.0, 0.0)
    assert o["levels"][:3].tolist() == [80.0, 120.0, 80.0] and np.isnan(o["levels"][3:]).all() and np.isnan(o["fp"]).all()
    assert o["lengths"].tolist() == [40, 40, 40] + [0] * 13
    # four plateaus 80, 120, 60, 100: median 90, deviations 10, 30, 30, 10: MAD 20 -> -0.5, 1.5, -1.5, 0.5
    y = np.repeat([80.0, 120.0, 60.0, 100.0], 40)
    o = fo.levels(y, 16)
    assert (o["count"], o["status"], o["norm"]) == (4, 0, (90.0, 20.0)) and o["fp"][:4].tolist() == [-0.5, 1.5, -1.5, 0.5]
    # E = 3 keeps the two highest of the three boundaries: the steps of 60 (80) and 40 (40, 120); E = 2 the step of 60
    sc = eo.scores(y, 8, 1e-3)
    assert sc[80] > sc[40] == sc[120]
    o = fo.levels(y, 3)
    assert o["nk"] == 3 and o["lengths"].tolist() == [80, 40, 40] and o["levels"].tolist() == [100.0, 60.0, 100.0]  # of equal scores the later index
    assert fo.levels(y, 2)["lengths"].tolist() == [80, 80]
    assert fo.select(np.asarray([5, 9, 20]), np.asarray([0.0] * 5 + [2.0] + [0.0] * 3 + [2.0] + [0.0] * 10 + [1.0]), 2).tolist() == [9]
    # status 1, 2 and a segment without a boundary (one event: MAD 0)
    assert fo.levels([1.0] * 30 + [np.nan], 8)["status"] == 1 and fo.levels([], 8)["status"] == 2 and fo.levels(np.arange(15.0), 8)["count"] == 0
    o = fo.levels(np.full(40, 7.0), 8)
    assert (o["count"], o["status"], o["lengths"][0], o["levels"][0]) == (1, 4, 40, 7.0)
    # DTW: [0, 1, 2] against [0, 2] -- 0 -> 0 (0), 1 -> 0 or 2 (1), 2 -> 2 (0)
    assert fo.dtw_pair([0, 1, 2], [0, 2]) == 1.0
    # one query value against three: every template value pairs with it -- 4 + 1 + 4
    assert fo.dtw_pair([3.0], [1.0, 2.0, 5.0]) == 9.0
    # a band of 1 with |n - m| = 4 is widened to 4: the end cell is reached (0 pairs with 0, the rest with 5: 25 + 16 + 9 + 4 + 1 + 0... )
    assert fo.dtw_pair([0, 1, 2, 3, 4, 5], [0, 5], 1) == 10.0 == fo.dtw_pair([0, 1, 2, 3, 4, 5], [0, 5], 0)
    # the band matters: [0, 0, 0, 9] against [0, 9, 9, 9] is 0 without one, and (0-9)^2 twice... with a band of 1
    assert fo.dtw_pair([0, 0, 0, 9], [0, 9, 9, 9]) == 0.0 and fo.dtw_pair([0, 0, 0, 9], [0, 9, 9, 9], 1) == 81.0
    q = np.asarray([[0, 1, 2, np.nan], [3.0, 0, 0, 0], [1, np.nan, 0, 0], [1, 1, 1, 1]])
    d = fo.dtw(q, [3, 1, 2, 5], np.asarray([[0, 2, 0.0], [1, 2, 5]]), [2, 3])
    assert d[0, 0] == 1.0 and d[1, 1] == 9.0 and np.isnan(d[2]).all() and np.isnan(d[3]).all()
    best, bd = fo.assign(np.asarray([[2.0, 1.0, 1.0], [np.nan] * 3, [5.0, 5.0, 7.0]]))
    assert best.tolist() == [[1, 2], [-1, -1], [0, 1]] and bd[0].tolist() == [1.0, 1.0] and np.isnan(bd[1]).all()
    assert fo.assign(np.asarray([[3.0]]))[0].tolist() == [[0, -1]]
    assert fo.same(np.asarray([np.nan, 1.0]), np.asarray([-np.nan, 1.0])) and not fo.same(np.asarray([0.0]), np.asarray([-0.0]))


def test_fingerprint_params_and_the_module():
    from adapted_amd import fingerprint as fpm
    from adapted_amd.polya_length import EventParams

    p = fpm.FingerprintParams()
    assert (p.max_events, p.band, p.events) == (110, 0, EventParams())
    p.check()
    for bad in (dict(max_events=1), dict(max_events=513), dict(band=-1), dict(events=EventParams(window=1))):
        with pytest.raises(ValueError):
            fpm.FingerprintParams(**bad).check()
    fpm.FingerprintParams(max_events=2).check()
    fpm.FingerprintParams(max_events=512, band=40).check()
    assert "untuned" in fpm.__doc__.lower() and "not claimed" in fpm.__doc__.lower()
    assert list(inspect.signature(fpm.event_levels).parameters) == ["signal", "params", "device"]
    assert list(inspect.signature(fpm.event_levels_batch).parameters)[:4] == ["signals", "lens", "segs", "params"]
    assert list(inspect.signature(fpm.dtw_distances).parameters)[:5] == ["q", "q_count", "t", "t_count", "band"]
    assert list(inspect.signature(fpm.assign_barcodes).parameters)[:4] == ["q", "q_count", "templates", "band"]
    assert list(inspect.signature(fpm.medoid_templates).parameters)[:4] == ["fingerprints", "counts", "labels", "band"]
    import adapted_amd.detect as detect

    assert not hasattr(detect, "fingerprint")  # (adapted_amd.detect mirrors the reference's package)
    for bad in (dict(q=np.zeros((2, 513))), dict(t=np.zeros((2, 0))), dict(tc=[0, 1]), dict(tc=[1, 5]), dict(band=-2),
                dict(t=np.asarray([[1.0, np.nan, 0, 0], [0, 0, 0, 0]]), tc=[2, 1])):
        kw = dict(q=np.zeros((2, 4)), qc=[1, 2], t=np.zeros((2, 4)), tc=[1, 2], band=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            fpm.dtw_distances(kw["q"], kw["qc"], kw["t"], kw["tc"], kw["band"])


def test_templates_round_trip_and_malformed_files(tmp_path):
    from adapted_amd import fingerprint as fpm

    t = fpm.Templates(["bc01", "bc02"], np.asarray([[1.0, -2.0, 7.0], [0.5, 0.25, 99.0]]), np.asarray([3, 2]))
    path = str(tmp_path / "t.npz")
    fpm.save_templates(path, t)
    u = fpm.load_templates(path)
    assert u.names == ["bc01", "bc02"] and u.counts.tolist() == [3, 2] and u.counts.dtype == np.int32
    assert fo.same(u.levels, np.asarray([[1.0, -2.0, 7.0], [0.5, 0.25, np.nan]]))  # NaN beyond each count
    with np.load(path) as z:
        assert sorted(z.files) == ["counts", "levels", "names"]
    lv, c = fpm.template_arrays(u)
    assert lv.tolist() == [[1.0, -2.0, 7.0], [0.5, 0.25, 0.0]] and c.tolist() == [3, 2]
    bad = {"missing": dict(names=["a"], levels=np.zeros((1, 2))),
           "shape": dict(names=["a"], levels=np.zeros(2), counts=np.asarray([1])),
           "names": dict(names=["a", "b"], levels=np.zeros((1, 2)), counts=np.asarray([1])),
           "count0": dict(names=["a"], levels=np.zeros((1, 2)), counts=np.asarray([0])),
           "count_big": dict(names=["a"], levels=np.zeros((1, 2)), counts=np.asarray([3])),
           "nan_inside": dict(names=["a"], levels=np.asarray([[np.nan, 1.0]]), counts=np.asarray([2])),
           "float_counts": dict(names=["a"], levels=np.zeros((1, 2)), counts=np.asarray([1.0])),
           "wide": dict(names=["a"], levels=np.zeros((1, 513)), counts=np.asarray([1]))}
    for name, arrays in bad.items():
        f = str(tmp_path / (name + ".npz"))
        np.savez(f, **arrays)
        with pytest.raises(ValueError, match="not a template file"):
            fpm.load_templates(f)
    with open(tmp_path / "text.npz", "w") as fh:
        fh.write("not an archive")
    for f in ("text.npz", "absent.npz"):
        with pytest.raises(ValueError, match="not a template file"):
            fpm.load_templates(str(tmp_path / f))


def test_medoid_templates_on_a_fake_distance_function():
    from adapted_amd import fingerprint as fpm

    calls = []

    def absdiff(q, qc, t, tc, band):
        """|first value of q - first value of t|: the medoid of a label is its median-most member"""
        calls.append((q.shape, list(qc), band))
        return np.abs(q[:, :1] - t[:, 0][None, :])

    fp = np.full((9, 4), np.nan)
    first = [10.0, 0.0, 11.0, 5.0, 14.0, 1.0, 5.0, np.inf, 2.0]
    labels = ["b", "a", "b", "c", "b", "a", "c", "a", "a"]
    counts = np.asarray([2, 3, 2, 1, 2, 3, 1, 2, 0], dtype=np.int32)
    for i, v in enumerate(first):
        fp[i, :max(counts[i], 1)] = v
    tm = fpm.medoid_templates(fp, counts, labels, band=3, distances=absdiff)
    # a: members 1 and 5 (7 holds an infinite value, 8 has no events): sums 1 and 1 -> the lower index; b: 10, 11, 14 -> 11; c: a tie -> 3
    assert tm.names == ["a", "b", "c"] and tm.counts.tolist() == [3, 2, 1] and tm.counts.dtype == np.int32
    assert fo.same(tm.levels, np.asarray([[0.0, 0.0, 0.0, np.nan], [11.0, 11.0, np.nan, np.nan], [5.0, np.nan, np.nan, np.nan]]))
    assert [c[0] for c in calls] == [(2, 4), (3, 4), (2, 4)] and all(c[2] == 3 for c in calls)
    with pytest.raises(ValueError, match="no usable"):
        fpm.medoid_templates(fp[[7, 8]], counts[[7, 8]], ["z", "z"], distances=absdiff)
    with pytest.raises(ValueError, match="one label"):
        fpm.medoid_templates(fp, counts, labels[:-1], distances=absdiff)
    assert fo.medoids(np.abs(np.subtract.outer(np.asarray(first[:7]), np.asarray(first[:7]))), labels[:7]) == [1, 2, 3]


def test_cli_options_and_refusals(tmp_path, monkeypatch):
    from adapted_amd import fingerprint as fpm
    from adapted_amd import main

    base = ["detect", "-i", str(tmp_path / "none.npz"), "-o", str(tmp_path / "out")]
    args = main.build_parser().parse_args(base + ["-c", "RNA004"])
    assert (args.fingerprints, args.barcode_templates, args.dtw_band) == (None, None, None)
    good = str(tmp_path / "good.npz")
    fpm.save_templates(good, fpm.Templates(["a"], np.asarray([[1.0, 2.0]]), np.asarray([2])))
    args = main.build_parser().parse_args(base + ["-c", "RNA004", "--fingerprints", "110", "--barcode_templates", good, "--dtw_band", "10"])
    assert (args.fingerprints, args.barcode_templates, args.dtw_band) == (110, good, 10)
    assert main._check_fingerprints(args).names == ["a"]
    args = main.build_parser().parse_args(base + ["-c", "RNA004", "--fingerprints", "16", "--event_params", "10,37,50", "--polya_length", "events"])
    main._check_polya_length(args)
    assert main._check_fingerprints(args) is None
    main._check_polya_length(main.build_parser().parse_args(base + ["-c", "RNA004", "--fingerprints", "16", "--event_params", "10,37,50"]))
    malformed = str(tmp_path / "malformed.npz")
    np.savez(malformed, names=["a"], levels=np.zeros((1, 2)))
    start_peak = str(tmp_path / "start_peak.toml")
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect = spc.cnn_boundaries.cnn_detect = False
    spc.rna_start_peak.detect_rna_start_peak = True
    spc.to_toml(start_peak)
    for extra, say in ((["-c", "RNA004", "--fingerprints", "16", "--int16_ingest"], "--int16_ingest"),
                       (["--config", start_peak, "--fingerprints", "16"], "primary is start_peak"),
                       (["-c", "RNA004", "--barcode_templates", good], "go with --fingerprints"),
                       (["-c", "RNA004", "--dtw_band", "3"], "go with --fingerprints"),
                       (["-c", "RNA004", "--fingerprints", "1"], "must lie in [2, 512]"),
                       (["-c", "RNA004", "--fingerprints", "513"], "must lie in [2, 512]"),
                       (["-c", "RNA004", "--fingerprints", "16", "--dtw_band", "3"], "--barcode_templates"),
                       (["-c", "RNA004", "--fingerprints", "16", "--barcode_templates", good, "--dtw_band", "-1"], ">= 0"),
                       (["-c", "RNA004", "--fingerprints", "16", "--event_params", "1,8,16"], "window must lie in [2, 64]"),
                       (["-c", "RNA004", "--fingerprints", "16", "--barcode_templates", str(tmp_path / "absent.npz")], "not a template file"),
                       (["-c", "RNA004", "--fingerprints", "16", "--barcode_templates", malformed], "not a template file"),
                       (["-c", "RNA004", "--event_params", "8,8,16"], "go with --polya_length")):
        with pytest.raises(SystemExit) as e:
            main.main(base + extra)
        assert say in str(e.value), (extra, e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        main.main(base + ["-c", "RNA004", "--fingerprints", "16"])
    assert "one GPU" in str(e.value)
    assert not os.path.exists(tmp_path / "out")  # nothing was created
    assert list(inspect.signature(main.run_detect).parameters)[-4:] == ["fingerprints", "polya_length", "adapter_nt", "event_params"]
    assert inspect.signature(main.run_detect).parameters["fingerprints"].default is None


def test_fingerprint_records_and_the_writer(tmp_path):
    from adapted_amd import main, pipeline
    from adapted_amd.container_types import DetectResults, ReadResult

    fp = pipeline.AdapterFingerprints(3, 4, True)
    fp.count[:], fp.status[:] = [3, -1, 2], [0, -1, 4]
    fp.lengths[0], fp.levels[0], fp.fingerprints[0] = [10, 20, 30, 0], [80.0, 90.0, 100.0, np.nan], [-1.0, 0.0, 1.0, np.nan]
    fp.lengths[2], fp.levels[2] = [5, 6, 0, 0], [70.0, 70.0, np.nan, np.nan]
    fp.best[0], fp.bestdist[0] = [1, 0], [0.125, 2.5]
    recs = main.fingerprint_records(["a", "b", "c"], fp, ["bc01", "bc02"])
    assert list(recs[0]["barcode"]) == main.BARCODE_COLUMNS
    assert recs[0]["barcode"] == {"read_id": "a", "n_events": 3, "barcode": "bc02", "dtw_dist": 0.125, "barcode_second": "bc01",
                                  "dtw_dist_second": 2.5, "dtw_margin": 2.375}
    assert recs[2]["barcode"]["barcode"] is None and np.isnan(recs[2]["barcode"]["dtw_margin"])
    assert "barcode" not in main.fingerprint_records(["a"], fp[:1])[0]
    half = fp[1:]
    assert len(half) == 2 and half.count.tolist() == [-1, 2] and half.best.shape == (2, 2)
    assert pipeline.AdapterFingerprints(2, 4, False)[0:1].best is None
    res = [DetectResults(success=True, adapter_start=0, adapter_end=60, adapter_len=60, polya_end=100, polya_len=40) for _ in range(2)]
    items = [ReadResult(read_id=i, success=True, detect_results=r) for i, r in zip("ac", res)]
    items[0].fingerprint, items[1].fingerprint = recs[0], recs[2]
    w = main._Writer(str(tmp_path), 2)
    w.enable_fingerprints(str(tmp_path), 4, barcodes=True)
    w.add(items)
    w.close()
    with np.load(tmp_path / "fingerprints" / "fingerprints_0.npz") as z:
        assert sorted(z.files) == ["count", "fingerprints", "lengths", "levels", "read_id", "status"]
        assert z["read_id"].tolist() == ["a", "c"] and z["count"].tolist() == [3, 2] and z["status"].tolist() == [0, 4]
        assert z["lengths"].tolist() == [[10, 20, 30, 0], [5, 6, 0, 0]] and z["lengths"].dtype == np.int32
        assert fo.same(z["fingerprints"], np.asarray([[-1.0, 0.0, 1.0, np.nan], [np.nan] * 4]))
    with open(tmp_path / "fingerprints" / "barcodes_0.csv") as fh:
        text = fh.read().splitlines()
    assert text == [",".join(main.BARCODE_COLUMNS), "a,3,bc02,0.125,bc01,2.5,2.375", "c,2,,,,,"]
    assert os.path.exists(tmp_path / "boundaries" / "detected_boundaries_0.csv")
    main._Writer(str(tmp_path / "plain"), 2).close()
    assert not os.path.exists(tmp_path / "plain" / "fingerprints")


class _Eng:
    """a recording engine: the segmentation's answers are numbered, so that what reaches on_rows can be told apart"""

    def __init__(self):
        self.calls, self.freed = [], []

    def segment_events(self, sig, lens, rows, starts, ends, args, cap=0, n=None, L=None, f64=False):
        self.calls.append(("segment_events", sig, lens.tolist(), rows.tolist(), starts.tolist(), ends.tolist(), cap, n, L))
        k = len(rows)
        return np.zeros((k, 0), dtype=np.int64), np.stack([np.arange(k) + 5, np.zeros(k, dtype=np.int64)], axis=1), \
            np.stack([np.arange(k) + 30.0, np.arange(k) + 1.0], axis=1)

    def event_levels(self, sig, lens, rows, starts, ends, args, max_events, n=None, L=None, f64=False, fp_ptr=None, count_ptr=None):
        self.calls.append(("event_levels", sig, lens.tolist(), rows.tolist(), starts.tolist(), ends.tolist(), max_events, n, L, fp_ptr, count_ptr))
        k, E = len(rows), max_events
        _, info, stats = _Eng.segment_events(_Eng(), sig, lens, rows, starts, ends, args)
        on_dev = fp_ptr is not None
        return {"info": info, "stats": stats, "count": None if on_dev else np.full(k, 2, dtype=np.int32), "status": np.zeros(k, dtype=np.int32),
                "lengths": np.full((k, E), 7, dtype=np.int32), "levels": np.full((k, E), 80.0),
                "fingerprints": None if on_dev else np.full((k, E), 0.5), "norm": np.zeros((k, 2))}

    def dtw_assign(self, q, q_count, t, t_count, band=0, nq=None, Eq=None, want_dist=True):
        self.calls.append(("dtw_assign", q, q_count, t.tolist(), t_count.tolist(), band, nq, Eq, want_dist))
        return None, np.tile(np.asarray([[1, 0]], dtype=np.int32), (nq, 1)), np.tile(np.asarray([[0.25, 4.0]]), (nq, 1))

    def dev_alloc(self, nbytes):
        self.calls.append(("dev_alloc", nbytes))
        return 7000 + nbytes

    def dev_free(self, ptr):
        self.freed.append(ptr)

    def d2h(self, arr, src):
        arr[...] = 0.75 if arr.dtype == np.float64 else 3


def _bare_pipeline(eng):
    from adapted_amd import lib, pipeline

    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.mb, p.m, p.N, p.eng, p._resident, p.native_i16, p.primary = 2, 100, 6, eng, 4096, False, "llr"
    p.slots = [{"lens": np.asarray([100, 250, 40, 100, 100, 100], dtype=np.int32)}]
    rows = lib.empty_rows(6)
    rows["success"] = [1, 0, 1, 1, 1, 1]
    rows["col"][:, 2], rows["col"][:, 3] = [3, 0, 0, 7, 9, 11], [50, 0, 30, 70, 90, 95]
    rows["present"] = [12, 0, 8, 12, 12, 12]
    return p, rows


def test_pipeline_method_one_segmentation_call_and_todays_arguments():
    from adapted_amd import fingerprint as fpm
    from adapted_amd import lib, pipeline
    from adapted_amd.polya_length import EventParams

    assert list(inspect.signature(pipeline.HostPipeline.__init__).parameters)[-1] == "second_opinion"
    assert list(inspect.signature(pipeline.HostPipeline.enable_fingerprints).parameters) == ["self", "params", "templates"]
    # refusals
    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.native_i16, p.primary = True, "llr"
    with pytest.raises(ValueError, match="int16"):
        p.enable_fingerprints()
    p.native_i16, p.primary = False, "start_peak"
    with pytest.raises(ValueError, match="LLR and CNN"):
        p.enable_fingerprints()
    p.primary = "cnn"
    with pytest.raises(ValueError, match="max_events"):
        p.enable_fingerprints(fpm.FingerprintParams(max_events=1))
    p.enable_polya_length(EventParams(10, 37, 50.0))
    with pytest.raises(ValueError, match="same event parameters"):
        p.enable_fingerprints(fpm.FingerprintParams(max_events=8))
    p.enable_fingerprints(fpm.FingerprintParams(max_events=8, events=EventParams(10, 37, 50.0)))
    assert p.fp_templates is None and p.fp_args.window == 10
    # enable_polya_length alone: what on_rows gets today -- one segment_events call, an EVENT_DTYPE array
    eng = _Eng()
    p, rows = _bare_pipeline(eng)
    p.enable_polya_length()
    mbs = np.asarray([0, lib.MB_MAD_ZERO, 0])
    ev0 = p._adapter_events(0, 5, rows, mbs)
    assert [c[0] for c in eng.calls] == ["segment_events"] and eng.calls[0][1:] == (4096, [100, 100, 40, 100, 100], [0, 4], [3, 9], [50, 90], 0, 5, 100)
    assert getattr(p, "fp_params", None) is None and ev0.dtype == pipeline.EVENT_DTYPE and ev0["n_bound"].tolist() == [5, -1, -1, -1, 6]
    # both options, with templates: one event_levels call, no segment_events call, then dtw_assign on the device pointers
    eng = _Eng()
    p, rows = _bare_pipeline(eng)
    p.enable_polya_length()
    tm = fpm.Templates(["x", "y"], np.asarray([[1.0, 2.0, np.nan], [0.0, 1.0, 2.0]]), np.asarray([2, 3]))
    p.enable_fingerprints(fpm.FingerprintParams(max_events=4, band=3), tm)
    ev, fp = p._adapter_fingerprints(0, 5, rows, mbs)
    names = [c[0] for c in eng.calls]
    assert names == ["dev_alloc", "dev_alloc", "event_levels", "dtw_assign"]
    fp_d, cnt_d = 7000 + 6 * 4 * 8, 7000 + 6 * 4
    assert eng.calls[2][1:] == (4096, [100, 100, 40, 100, 100], [0, 4], [3, 9], [50, 90], 4, 5, 100, fp_d, cnt_d)
    assert eng.calls[3][1:] == (fp_d, cnt_d, [[1.0, 2.0, 0.0], [0.0, 1.0, 2.0]], [2, 3], 3, 2, 4, False)
    assert ev.tobytes() == ev0.tobytes()  # its info / stats are what segment_events returns
    assert fp.count.tolist() == [3, -1, -1, -1, 3] and fp.status.tolist() == [0, -1, -1, -1, 0] and fp.best.tolist()[4] == [1, 0]
    assert fp.fingerprints[0].tolist() == [0.75] * 4 and np.isnan(fp.fingerprints[1]).all() and fp.lengths[4].tolist() == [7] * 4
    assert fp.bestdist[0].tolist() == [0.25, 4.0] and np.isnan(fp.bestdist[2]).all()
    p._adapter_fingerprints(0, 3, rows, None)
    assert [c[0] for c in eng.calls[4:]] == ["event_levels", "dtw_assign"] and eng.calls[4][3:6] == ([0, 2], [3, 0], [50, 30])  # (the buffers stay)
    # fingerprints alone, no templates: host arrays, no events
    eng = _Eng()
    p, rows = _bare_pipeline(eng)
    p.enable_fingerprints(fpm.FingerprintParams(max_events=4))
    ev, fp = p._adapter_fingerprints(0, 5, rows, mbs)
    assert ev is None and [c[0] for c in eng.calls] == ["event_levels"] and eng.calls[0][-2:] == (None, None)
    assert fp.best is None and fp.count.tolist() == [2, -1, -1, -1, 2] and fp.fingerprints[4].tolist() == [0.5] * 4
    rows["success"][:] = 0
    ev, fp = p._adapter_fingerprints(0, 5, rows, mbs)
    assert len(eng.calls) == 1 and (fp.count == -1).all()  # no passing read: no call
