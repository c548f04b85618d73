"""The host side of the event segmentation and the poly(A) length estimate (adp_segment_events, adapted_amd/polya_length.py,
`adapted detect --polya_length`), without a GPU: the new header against its prototype table, the refusals before launch, the
oracle's own known answers, estimate_polya_length, and the command line's refusals."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import events_oracle as eo
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(os.path.join(ROOT, "include", "adapted_hip_events.h"))
    assert sorted(declared) == sorted(lib.EVENT_PROTOTYPES) == ["adp_segment_events", "adp_sizeof_event_args"]
    assert not set(lib.EVENT_PROTOTYPES) & (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES))
    assert not set(lib.EVENT_PROTOTYPES) & set(lib.EXPORTS)
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        assert '#include "adapted_hip_events.h"' in fh.read()
    assert len(_prototypes(os.path.join(ROOT, "include", "adapted_hip.h"))) == len(lib.PROTOTYPES) == 62
    L = lib.load()
    assert L.adp_abi_version() == 3
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.EVENT_PROTOTYPES[name].split(":")
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
    assert L.adp_sizeof_event_args() == ctypes.sizeof(lib.AdpEventArgs) == 24
    assert [f[0] for f in lib.AdpEventArgs._fields_] == ["threshold", "var_floor", "window", "min_distance"]


def test_exported_kernel_constants_are_the_headers():
    """lib.EVENTS_TILE / EVENTS_SCRATCH_MIB / events_slot_bytes restate events_api.h and the entry point: the GPU tests place their
    tile-edge and batch-of-slots cases by them"""
    import re

    from adapted_amd import lib

    with open(os.path.join(ROOT, "adapted_amd", "csrc", "events_api.h")) as fh:
        text = fh.read()
    assert int(re.search(r"#define EV_TILE (\d+)", text).group(1)) == lib.EVENTS_TILE
    assert int(re.search(r"#define EV_SCRATCH_MIB (\d+)", text).group(1)) == lib.EVENTS_SCRATCH_MIB
    assert int(re.search(r"#define EV_WMAX (\d+)", text).group(1)) == 64
    with open(os.path.join(ROOT, "adapted_amd", "csrc", "modules.hip")) as fh:
        entry = fh.read()
    assert "stride = ((size_t)(lmax > 0 ? lmax : 1) + 1) & ~(size_t)1, half = stride / 2 + 1;" in entry
    assert "((size_t)mib << 20) / (stride * 8 + half * 8)" in entry and 'getenv("ADP_EVENTS_SCRATCH_MIB")' in entry
    assert lib.events_slot_bytes(40000) == 40000 * 8 + 20001 * 8 and lib.events_slot_bytes(0) == 2 * 8 + 2 * 8
    assert lib.events_slot_bytes(3501) == 3502 * 8 + 1752 * 8


def test_an_empty_batch_of_segments_has_an_empty_answer():
    from adapted_amd import lib

    eng = lib.Engine.__new__(lib.Engine)  # (no handle: the library is not entered)
    eng._h = lib._VoidP()
    pos, info, stats = eng.segment_events(np.zeros((2, 8), dtype=np.float32), [8, 8], [], [], [], lib.AdpEventArgs(16.0, 1e-3, 8, 8), cap=3)
    assert pos.shape == (0, 3) and info.shape == (0, 2) and stats.shape == (0, 2) and pos.dtype == info.dtype == np.int64


def test_the_new_header_defines_no_numeric_macro():
    with open(os.path.join(ROOT, "include", "adapted_hip_events.h")) as fh:
        defines = [ln.split()[1] for ln in fh if ln.startswith("#define")]
    assert defines == ["ADAPTED_HIP_EVENTS_H"]


def test_null_handle_is_refused_and_wrong_types_never_enter_the_library():
    from adapted_amd import lib

    L = lib.load()
    a = lib.AdpEventArgs(16.0, 1e-3, 8, 8)
    assert L.adp_segment_events(None, None, None, 1, 8, None, 1, ctypes.byref(a), 0, 0, None, None, None) == -1  # ADP_ERR_INVALID
    assert b"bad argument" in L.adp_last_error()
    segs = np.zeros(1, dtype=lib.SEG_DTYPE)
    with pytest.raises(ctypes.ArgumentError):  # int64 for int32 *len
        L.adp_segment_events(None, None, np.zeros(1, dtype=np.int64), 1, 8, segs, 1, ctypes.byref(a), 0, 0, None, None, None)
    with pytest.raises(ctypes.ArgumentError):  # int32 for int64 *pos_out
        L.adp_segment_events(None, None, None, 1, 8, segs, 1, ctypes.byref(a), 0, 4, np.zeros(4, dtype=np.int32), None, None)
    with pytest.raises(ctypes.ArgumentError):  # float32 for double *stats_out
        L.adp_segment_events(None, None, None, 1, 8, segs, 1, ctypes.byref(a), 0, 0, None, None, np.zeros(2, dtype=np.float32))
    with pytest.raises(ctypes.ArgumentError):  # plain int64 triples for adp_seg *segs
        L.adp_segment_events(None, None, None, 1, 8, np.zeros(3, dtype=np.int64), 1, ctypes.byref(a), 0, 0, None, None, None)


def test_oracle_known_answers():
    x = np.repeat([80, 95, 70, 100, 60, 90], [30, 12, 8, 25, 9, 40])
    b, status, med, mad = eo.segment(x, 8, 8, 16.0)
    assert b.tolist() == [30, 42, 50, 75, 84] and status == 0 and (med, mad) == (10.5, 2.0)
    y = [0] * 20 + [5] + [10] * 20
    sc = eo.scores(y, 8, 1e-3)
    assert sc[20] == sc[21] > sc[19] and sc[22] < sc[21]
    assert eo.segment(y)[0].tolist() == [20]  # one plateau, its midpoint rounded down
    for n, nonzero in ((15, 0), (16, 1), (17, 2)):
        assert int((eo.scores(np.arange(n, dtype=np.float64) ** 2, 8, 1e-3) != 0).sum()) == nonzero
    assert eo.segment(np.arange(15.0))[1] == 2 and eo.segment([1.0] * 30 + [np.nan])[1] == 1
    assert eo.segment([np.nan])[1] == 1 and eo.segment([])[1] == 2  # a NaN counts before the length
    z = np.repeat([0, 1, 3, 7, 15, 31], [10, 5, 5, 5, 5, 10]) + np.resize([0, .25, -.25, .125], 40)
    assert eo.candidates(z, 3, 1.0, 1e-3)[0].tolist() == [6, 10, 15, 20, 25, 30, 34]
    assert eo.segment(z, 3, 6, 1.0)[0].tolist() == [10, 20, 30]
    assert not eo.has_close_ties(z, 3, 6, 1.0, 1e-3) and eo.has_close_ties([0] * 9 + [1] * 3 + [0] * 9, 3, 9, 1.0, 1e-3)
    # the clipping of a segment: a Python slice of the read, an empty one for a negative start
    row = np.arange(10.0)
    assert eo.clip(row, 7, 2, 100).tolist() == [2, 3, 4, 5, 6] and eo.clip(row, 7, 8, 9).size == 0
    assert eo.clip(row, 7, -1, 5).size == 0 and eo.clip(row, 7, 5, 5).size == 0


def test_estimate_polya_length():
    from adapted_amd.polya_length import estimate_polya_length as est

    nt, spn = est([0, 10, 5], [600, 610, 305], [1800, 910, 400], method="events", event_len_med=[30.0, 12.5, 9.5])
    assert nt.tolist() == [40.0, 24.0, 10.0] and spn.tolist() == [30.0, 12.5, 9.5] and nt.dtype == np.float64
    nt, spn = est([0, 10], [600, 610], [1800, 910], method="adapter", adapter_nt=60)
    assert nt.tolist() == [120.0, 30.0] and spn.tolist() == [10.0, 10.0]
    nt, spn = est([100], [400], [1000], method="adapter", adapter_nt=[70])
    assert spn[0] == 300 / 70 and nt[0] == 600 / (300 / 70)
    # a missing input, a speed that is not > 0
    nt, spn = est([0, None, 0, 0, 0], [600, 610, None, 600, 600], [1800, 910, 900, None, 1800], method="events",
                  event_len_med=[None, 30.0, 30.0, 30.0, float("nan")])
    assert np.isnan(nt[[0, 2, 3, 4]]).all() and nt[1] == 10.0  # (the events method does not read adapter_start)
    assert np.isnan(spn[[0, 4]]).all() and spn[1:4].tolist() == [30.0] * 3
    nt, spn = est([0, 0, 600], [600, 600, 600], [1800, 1800, 1800], method="events", event_len_med=[0.0, -3.0, 30.0])
    assert np.isnan(nt[:2]).all() and np.isnan(spn[:2]).all() and nt[2] == 40.0
    nt, spn = est([600, 0, None], [600, 600, 600], [1800, 1800, 1800], method="adapter", adapter_nt=60)  # an adapter of no samples
    assert np.isnan(nt[0]) and np.isnan(spn[0]) and nt[1] == 120.0 and np.isnan(nt[2])
    assert np.isnan(est([0], [600], [1800], method="adapter", adapter_nt=0)[0][0])
    for bad in (dict(method="events"), dict(method="adapter"), dict(method="median", adapter_nt=60)):
        with pytest.raises(ValueError):
            est([0], [600], [1800], **bad)
    assert list(inspect.signature(est).parameters) == ["adapter_start", "adapter_end", "polya_end", "method", "event_len_med", "adapter_nt"]


def test_event_params_defaults_and_checks():
    from adapted_amd import polya_length as pl

    p = pl.EventParams()
    assert (p.window, p.min_distance, p.threshold, p.var_floor) == (8, 8, 16.0, 1e-3)
    a = p.args()
    assert (a.window, a.min_distance, a.threshold, a.var_floor) == (8, 8, 16.0, 1e-3)
    assert pl.EventParams.parse("10, 37,50") == pl.EventParams(10, 37, 50.0)
    for bad in ("8,8", "1,8,16", "65,8,16", "8,0,16", "8,8,0", "8,8,nan", "8,8,inf", "a,b,c"):
        with pytest.raises(ValueError):
            pl.EventParams.parse(bad)
    with pytest.raises(ValueError):
        pl.EventParams(var_floor=0.0).check()
    assert "untuned" in pl.__doc__.lower()
    assert list(inspect.signature(pl.segment_events).parameters) == ["signal", "params", "device"]
    assert list(inspect.signature(pl.segment_events_batch).parameters)[:6] == ["signals", "lens", "segs", "params", "cap", "device"]
    import adapted_amd.detect as detect

    assert not hasattr(detect, "polya_length")  # (adapted_amd.detect mirrors the reference's package)


def test_polya_length_records_and_the_writer(tmp_path):
    from adapted_amd import main, pipeline
    from adapted_amd.container_types import DetectResults, ReadResult

    res = [DetectResults(success=True, adapter_start=10, adapter_end=610, adapter_len=600, polya_end=1810, polya_len=1200, polya_truncated=True),
           DetectResults(success=True, adapter_start=0, adapter_end=300, adapter_len=300, polya_end=400, polya_len=100)]
    ev = np.zeros(2, dtype=pipeline.EVENT_DTYPE)
    ev["n_bound"], ev["status"], ev["med"], ev["mad"] = [21, 1], [0, 0], [30.5, np.nan], [4.25, np.nan]
    recs = main.polya_length_records(["a", "b"], res, ev, "events")
    assert list(recs[0]) == main.POLYA_LENGTH_COLUMNS
    assert recs[0] == {"read_id": "a", "adapter_len": 600, "polya_len": 1200, "n_events": 20, "event_len_med": 30.5, "event_len_mad": 4.25,
                       "samples_per_nt": 30.5, "polya_nt": 1200 / 30.5, "polya_truncated": True}
    assert recs[1]["n_events"] == 0 and np.isnan(recs[1]["polya_nt"]) and recs[1]["polya_truncated"] is None
    assert main.polya_length_records(["a", "b"], res, ev, "adapter", 60)[1]["polya_nt"] == 20.0
    w = main._Writer(str(tmp_path), 2, polya_length=True)
    items = [ReadResult(read_id=i, success=True, detect_results=r) for i, r in zip("ab", res)]
    for it, rec in zip(items, recs):
        it.polya_length = rec
    w.add(items)
    w.close()
    with open(tmp_path / "polya_length" / "polya_length_0.csv") as fh:
        text = fh.read().splitlines()
    assert text[0] == ",".join(main.POLYA_LENGTH_COLUMNS)
    assert text[1] == "a,600,1200,20,30.5,4.25,30.5,39.344,True" and text[2] == "b,300,100,0,,,,,"
    assert os.path.exists(tmp_path / "boundaries" / "detected_boundaries_0.csv")
    main._Writer(str(tmp_path / "plain"), 2).close()
    assert not os.path.exists(tmp_path / "plain" / "polya_length")


def test_cli_options_and_refusals(tmp_path, monkeypatch):
    from adapted_amd import main

    base = ["detect", "-i", str(tmp_path / "none.npz"), "-o", str(tmp_path)]
    args = main.build_parser().parse_args(base + ["-c", "RNA004"])
    assert (args.polya_length, args.adapter_nt, args.event_params) == (None, None, None)
    assert (args.flag_truncated, args.int16_ingest, args.second_opinion, args.start_peak, args.batch_size, args.minibatch_size) == \
        (False, False, None, False, 4000, 1000)
    args = main.build_parser().parse_args(base + ["-c", "RNA004", "--polya_length", "adapter", "--adapter_nt", "60", "--event_params", "10,37,50"])
    assert (args.polya_length, args.adapter_nt, args.event_params) == ("adapter", 60.0, "10,37,50")
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(base + ["-c", "RNA004", "--polya_length", "median"])
    # refused with a message before a GPU is touched (nothing is created either)
    start_peak = str(tmp_path / "start_peak.toml")
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect = spc.cnn_boundaries.cnn_detect = False
    spc.rna_start_peak.detect_rna_start_peak = True
    spc.to_toml(start_peak)
    for extra, say in ((["-c", "RNA004", "--polya_length", "events", "--int16_ingest"], "--int16_ingest"),
                       (["--config", start_peak, "--polya_length", "events"], "primary is start_peak"),
                       (["-c", "RNA004", "--polya_length", "adapter"], "--adapter_nt"),
                       (["-c", "RNA004", "--polya_length", "adapter", "--adapter_nt", "0"], "--adapter_nt must be > 0"),
                       (["-c", "RNA004", "--polya_length", "events", "--event_params", "1,8,16"], "window must lie in [2, 64]"),
                       (["-c", "RNA004", "--adapter_nt", "60"], "go with --polya_length")):
        with pytest.raises(SystemExit) as e:
            main.main(base + extra)
        assert say in str(e.value), (extra, e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        main.main(base + ["-c", "RNA004", "--polya_length", "events"])
    assert "one GPU" in str(e.value)
    assert not [d for d in os.listdir(tmp_path) if d.startswith("adapted_")]


def test_pipeline_refuses_what_it_cannot_do_and_leaves_its_constructor_alone():
    from adapted_amd import lib, main, pipeline

    assert list(inspect.signature(pipeline.HostPipeline.__init__).parameters)[-1] == "second_opinion"
    assert list(inspect.signature(main.run_detect).parameters)[-3:] == ["polya_length", "adapter_nt", "event_params"]
    assert list(inspect.signature(main._Writer.__init__).parameters)[-1] == "polya_length"
    assert list(inspect.signature(lib.Engine.segment_events).parameters) == ["self", "sig", "lens", "rows", "starts", "ends", "args", "cap", "n", "L", "f64"]
    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.native_i16, p.primary = True, "llr"
    with pytest.raises(ValueError, match="int16"):
        p.enable_polya_length()
    p.native_i16, p.primary = False, "start_peak"
    with pytest.raises(ValueError, match="LLR and CNN"):
        p.enable_polya_length()
    p.primary = "cnn"
    p.enable_polya_length()
    assert (p.event_args.window, p.event_args.threshold) == (8, 16.0)


def test_pipeline_segments_the_passing_reads_adapters_on_the_resident_matrix():
    """HostPipeline._adapter_events of a bare object with a recording engine: one call, the passing reads of undropped minibatches,
    their adapter bounds, lengths clipped to the window"""
    from adapted_amd import lib, pipeline

    calls = []

    class Eng:
        def segment_events(self, sig, lens, rows, starts, ends, args, cap=0, n=None, L=None, f64=False):
            calls.append((sig, lens.tolist(), rows.tolist(), starts.tolist(), ends.tolist(), cap, n, L))
            k = len(rows)
            return np.zeros((k, 0), dtype=np.int64), np.stack([np.arange(k) + 5, np.zeros(k, dtype=np.int64)], axis=1), \
                np.stack([np.arange(k) + 30.0, np.arange(k) + 1.0], axis=1)

    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.mb, p.m, p.eng, p._resident = 2, 100, Eng(), 4096
    p.event_args = pipeline.lib.AdpEventArgs(16.0, 1e-3, 8, 8)
    p.slots = [{"lens": np.asarray([100, 250, 40, 100, 100, 100], dtype=np.int32)}]
    rows = lib.empty_rows(6)
    rows["success"] = [1, 0, 1, 1, 1, 1]
    rows["col"][:, 2], rows["col"][:, 3] = [3, 0, 0, 7, 9, 11], [50, 0, 30, 70, 90, 95]
    rows["present"] = [12, 0, 8, 12, 12, 12]  # (read 2: no adapter_start in its row -> 0)
    ev = p._adapter_events(0, 5, rows, np.asarray([0, lib.MB_MAD_ZERO, 0]))
    assert calls == [(4096, [100, 100, 40, 100, 100], [0, 4], [3, 9], [50, 90], 0, 5, 100)]
    assert ev.dtype == pipeline.EVENT_DTYPE and ev["n_bound"].tolist() == [5, -1, -1, -1, 6]
    assert ev["med"][[0, 4]].tolist() == [30.0, 31.0] and np.isnan(ev["med"][1:4]).all() and ev["mad"][4] == 2.0
    ev = p._adapter_events(0, 3, rows, None)
    assert calls[-1][2:5] == ([0, 2], [3, 0], [50, 30])
