"""The host side of the adapter-front post-pass (adp_adapter_front / adp_adapter_front_i16, adapted_amd/adapter_front.py, `adapted
detect --adapter_front`), without a GPU: the new header against its prototype table, the refusals before launch, the parameters,
the command line's refusals, the pipeline's wiring, and the oracle's own known answers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import adapter_front_oracle as O
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["adp_adapter_front", "adp_adapter_front_i16", "adp_sizeof_adapter_front_args"]


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(os.path.join(ROOT, "include", "adapted_hip_adapter_front.h"))
    assert sorted(declared) == sorted(lib.ADAPTER_FRONT_PROTOTYPES) == NAMES
    others = (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES) | set(lib.EVENT_PROTOTYPES)
              | set(lib.FINGERPRINT_PROTOTYPES) | set(lib.EXPORTS))
    assert not set(lib.ADAPTER_FRONT_PROTOTYPES) & others
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_adapter_front.h"') == 1
    assert text.index('#include "adapted_hip_fingerprint.h"') < text.index('#include "adapted_hip_adapter_front.h"') < text.index("adp_set_profiling")
    assert re.search(r"^#define\s+ADP_ROW_ADAPTER_FRONT\s+8\s*$", text, re.M) and lib.ROW_ADAPTER_FRONT == O.ROW_ADAPTER_FRONT == 8
    assert re.search(r"^#define\s+ADP_ABI_VERSION\s+3\s*$", text, re.M)
    with open(os.path.join(ROOT, "include", "adapted_hip_adapter_front.h")) as fh:
        assert [ln.split()[1] for ln in fh if ln.startswith("#define")] == ["ADAPTED_HIP_ADAPTER_FRONT_H"]
    L = lib.load()
    assert L.adp_abi_version() == 3 and L.adp_sizeof_row() == lib.ROW_DTYPE.itemsize == 544
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.ADAPTER_FRONT_PROTOTYPES[name].split(":")
        assert got_ret == ret and got_params.split() == params, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for q, t in zip(params, fn.argtypes):
            if q in lib._SCALARS:
                assert t is lib._SCALARS[q], (name, q)
            elif q[:-1] in lib._ELEMENTS:
                assert isinstance(t, lib._Pointer) and t.element == q[:-1], (name, q)
            elif q == "adp_adapter_front_args*":
                assert t is ctypes.POINTER(lib.AdpAdapterFrontArgs), (name, q)
            else:
                assert t is ctypes.c_void_p and q == "adp_handle*", (name, q)
    # adp_adapter_start_args, then min_adapter_len
    assert L.adp_sizeof_adapter_front_args() == ctypes.sizeof(lib.AdpAdapterFrontArgs) == 32
    fields = [f[0] for f in lib.AdpAdapterFrontArgs._fields_]
    assert fields[:4] == [f[0] for f in lib.AdpAdapterStartArgs._fields_] and fields[4:] == ["min_adapter_len", "pad"]
    # the int16 form: the raw rows and their calibration as the detect twins take them, then the float32 form's tail
    f32, i16 = (lib.ADAPTER_FRONT_PROTOTYPES[k].split() for k in NAMES[:2])
    assert i16[:6] == lib.PROTOTYPES["adp_detect_llr_i16"].split()[:6] and i16[6:] == f32[4:]


def test_null_handle_is_refused_and_wrong_types_never_enter_the_library():
    from adapted_amd import lib

    L = lib.load()
    a = lib.AdpAdapterFrontArgs(20.0, 90.0, 100, 2500, 1000, 0)
    rows = lib.empty_rows(1)
    info, i64, f64 = np.zeros((1, 4), dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(1)
    sig = np.zeros((1, 8), dtype=np.float32)
    assert L.adp_adapter_front(None, sig, None, 1, 8, rows, ctypes.byref(a), 0, info, i64, i64, f64) == -1  # ADP_ERR_INVALID
    assert b"bad argument" in L.adp_last_error()
    assert L.adp_adapter_front_i16(None, None, None, None, None, 1, 8, rows, ctypes.byref(a), 1, info, i64, i64, f64) == -1
    with pytest.raises(ctypes.ArgumentError):  # float64 for float *sig
        L.adp_adapter_front(None, np.zeros((1, 8)), None, 1, 8, rows, ctypes.byref(a), 0, info, i64, i64, f64)
    with pytest.raises(ctypes.ArgumentError):  # plain bytes for adp_row *rows
        L.adp_adapter_front(None, sig, None, 1, 8, np.zeros(544, dtype=np.uint8), ctypes.byref(a), 0, info, i64, i64, f64)
    with pytest.raises(ctypes.ArgumentError):  # int32 for int64 *shift_out
        L.adp_adapter_front(None, sig, None, 1, 8, rows, ctypes.byref(a), 0, info, np.zeros(1, dtype=np.int32), i64, f64)
    with pytest.raises(ctypes.ArgumentError):  # float32 for int16 *raw
        L.adp_adapter_front_i16(None, sig, None, None, None, 1, 8, rows, ctypes.byref(a), 1, info, i64, i64, f64)
    with pytest.raises(ctypes.ArgumentError):  # the start module's arguments for adp_adapter_front_args *
        L.adp_adapter_front(None, sig, None, 1, 8, rows, ctypes.byref(lib.AdpAdapterStartArgs()), 0, info, i64, i64, f64)
    # the engine's own check of the rows: before the library
    eng = lib.Engine.__new__(lib.Engine)  # (no handle: the library is not entered)
    eng._h, eng.m, eng.lib = lib._VoidP(), 8, L
    frozen = lib.empty_rows(1)
    frozen.setflags(write=False)
    for bad in (np.zeros(2, dtype=lib.ROW_DTYPE), np.zeros(1, dtype=np.int64), frozen, lib.empty_rows(1).reshape(1, 1)):
        with pytest.raises(ValueError, match="rows"):
            eng.adapter_front(sig, None, bad, a)


def test_params_defaults_parse_and_check():
    from adapted_amd import adapter_front as af
    from adapted_amd.config.schema import MMAdapterStartConfig

    p, c = af.AdapterFrontParams(), MMAdapterStartConfig()
    assert (p.window, p.min_obs_adapter, p.min_shift, p.min_pA_current) == (c.window, c.min_obs_adapter, c.min_shift, c.min_pA_current) == \
        (100, 2500, 20.0, 90.0)
    assert p.min_adapter_len == 0
    a = af.AdapterFrontParams(16, 64, 5.0, 91.5, 32).args()
    assert (a.window, a.min_obs_adapter, a.min_shift, a.min_pA_current, a.min_adapter_len, a.pad) == (16, 64, 5.0, 91.5, 32, 0)
    assert af.AdapterFrontParams.parse(" 50, 1200,12.5 ,100", min_adapter_len=7) == af.AdapterFrontParams(50, 1200, 12.5, 100.0, 7)
    for bad in ("100,2500,20", "100,2500,20,90,1", "0,2500,20,90", "100,-1,20,90", "100,2500,nan,90", "100,2500,20,inf", "a,b,c,d",
                "1.5,2500,20,90", "4294967296,2500,20,90"):
        with pytest.raises(ValueError):
            af.AdapterFrontParams.parse(bad)
    with pytest.raises(ValueError, match="min_adapter_len"):
        af.AdapterFrontParams(min_adapter_len=-1).check()
    assert "untuned" in af.__doc__.lower() and "not repeated" in af.__doc__.lower()
    assert list(inspect.signature(af.adapter_front_rows).parameters)[:4] == ["signals", "lens", "rows", "params"]
    import adapted_amd.detect as detect

    assert not hasattr(detect, "adapter_front")  # (adapted_amd.detect mirrors the reference's package)
    # an empty batch has an empty answer, and the library is not entered
    rows, info, shift, cand, diff = af.adapter_front_rows(np.zeros((0, 8), dtype=np.float32), None, np.zeros(0, dtype=af.lib.ROW_DTYPE))
    assert rows.size == 0 and info.shape == (0, 4) and shift.dtype == cand.dtype == np.int64 and diff.dtype == np.float64


def test_cli_options_and_refusals(tmp_path):
    from adapted_amd import main
    from adapted_amd.config import get_chemistry_specific_config

    base = ["detect", "-i", str(tmp_path / "none.npz"), "-o", str(tmp_path)]
    args = main.build_parser().parse_args(base + ["-c", "RNA004"])
    assert (args.adapter_front, args.adapter_front_params) == (False, None)
    assert (args.flag_truncated, args.int16_ingest, args.second_opinion, args.start_peak, args.polya_length, args.fingerprints) == \
        (False, False, None, False, None, None)
    args = main.build_parser().parse_args(base + ["-c", "RNA004", "--adapter_front", "--adapter_front_params", "50,1200,12.5,100", "--int16_ingest"])
    assert (args.adapter_front, args.adapter_front_params, args.int16_ingest) == (True, "50,1200,12.5,100", True)
    assert main._check_adapter_front(args).window == 50 and main._check_adapter_front(main.build_parser().parse_args(base + ["-c", "RNA004"])) is None
    # refused with a message before a GPU is touched (nothing is created either)
    start_peak = str(tmp_path / "start_peak.toml")
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect = spc.cnn_boundaries.cnn_detect = False
    spc.rna_start_peak.detect_rna_start_peak = True
    spc.to_toml(start_peak)
    for extra, say in ((["--config", start_peak, "--adapter_front"], "primary is start_peak"),
                       (["-c", "RNA004", "--adapter_front_params", "100,2500,20,90"], "goes with --adapter_front"),
                       (["-c", "RNA004", "--adapter_front", "--adapter_front_params", "100,2500,20"], "WINDOW,MIN_OBS_ADAPTER,MIN_SHIFT,MIN_PA"),
                       (["-c", "RNA004", "--adapter_front", "--adapter_front_params", "0,2500,20,90"], "window must be >= 1"),
                       (["-c", "RNA004", "--adapter_front", "--adapter_front_params", "100,-5,20,90"], "min_obs_adapter must be >= 0"),
                       (["-c", "RNA004", "--adapter_front", "--adapter_front_params", "100,2500,nan,90"], "min_shift must be finite"),
                       (["-c", "RNA004", "--adapter_front", "--adapter_front_params", "x,2500,20,90"], "--adapter_front_params")):
        with pytest.raises(SystemExit) as e:
            main.main(base + extra)
        assert say in str(e.value), (extra, e.value)
    assert not [d for d in os.listdir(tmp_path) if d.startswith("adapted_")]


def test_signatures_keep_their_pinned_tails():
    from adapted_amd import lib, main, pipeline

    params = list(inspect.signature(main.run_detect).parameters)
    assert params[-4:] == ["fingerprints", "polya_length", "adapter_nt", "event_params"] and params[-5] == "adapter_front"
    assert inspect.signature(main.run_detect).parameters["adapter_front"].default is None
    assert list(inspect.signature(pipeline.HostPipeline.__init__).parameters)[-1] == "second_opinion"
    assert list(inspect.signature(lib.Engine.adapter_front).parameters) == ["self", "sig", "full_lens", "rows", "args", "n", "m"]
    assert list(inspect.signature(lib.Engine.adapter_front_i16).parameters) == ["self", "raw_dev", "len_dev", "scale_dev", "offset_dev", "rows",
                                                                               "args", "n", "m"]


def test_pipeline_runs_the_pass_on_what_the_detect_call_read():
    """HostPipeline.enable_adapter_front / _adapter_front of a bare object with a recording engine: the float32 matrix or the raw
    rows with their calibration, the call's rows patched in place, ahead of the event segmentation"""
    from adapted_amd import lib, pipeline
    from adapted_amd.adapter_front import AdapterFrontParams

    calls = []

    class Eng:
        def adapter_front(self, sig, full_lens, rows, args, n=None, m=None):
            calls.append(("f32", sig, full_lens, n, m, args.window, args.min_adapter_len))
            rows["col"][0, 2] = 77
            return np.asarray([[0, 0, 0, 1]] + [[-1, 0, 0, 0]] * (n - 1), dtype=np.int32), None, None, None

        def adapter_front_i16(self, raw, dlen, scale, offset, rows, args, n, m=None):
            calls.append(("i16", raw, dlen, scale, offset, n, m))
            return np.zeros((n, 4), dtype=np.int32), None, None, None

    p = pipeline.HostPipeline.__new__(pipeline.HostPipeline)
    p.primary = "start_peak"
    with pytest.raises(ValueError, match="LLR and CNN"):
        p.enable_adapter_front()
    p.primary = "llr"
    with pytest.raises(ValueError, match="window"):
        p.enable_adapter_front(AdapterFrontParams(window=0))
    assert getattr(p, "front_args", None) is None
    p.enable_adapter_front(AdapterFrontParams(min_adapter_len=1000))
    assert (p.front_args.window, p.front_args.min_obs_adapter, p.front_args.min_adapter_len, p.front_patched) == (100, 2500, 1000, 0)
    p.m, p.eng, p.native_i16, p._resident = 100, Eng(), False, 4096
    rows = lib.empty_rows(3)
    assert p._adapter_front(0, 3, rows) is rows and rows["col"][0, 2] == 77 and p.front_patched == 1
    p.native_i16, p._resident_i16 = True, (8192, 1, 2, 3)
    p._adapter_front(0, 2, rows[:2])
    assert calls == [("f32", 4096, None, 3, 100, 100, 1000), ("i16", 8192, 1, 2, 3, 2, 100)]
    src = inspect.getsource(pipeline.HostPipeline.run)
    assert src.index("self._adapter_front(j, n, rows)") < src.index("self._adapter_fingerprints(j, n, rows, mbs)") < src.index("self._adapter_events(j, n, rows, mbs)")


def _by_definition(x, w, min_obs):
    """moving_mean_adapter_start_detect's candidate written out in float64: the means of x[i:i + w) for i < N - w, the mean of
    those behind i less the mean of those up to i, the first minimum from position w on -> (cand, difference[cand])"""
    used = np.asarray(x[:len(x) - min_obs], dtype=np.float64)
    fwd = np.asarray([used[i:i + w].mean() for i in range(used.size - w)])
    diff = np.asarray([fwd[i:].mean() - fwd[:i + 1].mean() for i in range(fwd.size)])
    cand = w + int(np.argmin(diff[w:]))
    return cand, diff[cand]


def test_oracle_known_answers():
    """three hand-made reads: moved, not accepted, ValueError -- and the rows around them.  The samples are small integers, so the
    float32 chains are exact and the definition in float64 gives the same candidate"""
    x = np.full((4, 400), 80.0, dtype=np.float32)
    x[0, :100] = 150.0  # a lead the detector finds
    x[1, :100] = 150.0  # the same lead in a shorter adapter: too little of it would be left
    x[1, 200:] = 200.0  # (behind its adapter's end)
    x[3, :100] = 150.0  # a failing row
    rows = O.make_rows([(0, 300), (None, 200), (0, 59), (0, 300)], success=[1, 1, 1, 0])
    p = O.params(window=10, min_obs_adapter=50, min_shift=5.0, min_pA_current=90.0, min_adapter_len=150)
    out, info, shift, cand, diff = O.front(x, rows, p)
    c0, d0 = _by_definition(x[0, :300], 10, 50)
    c1, d1 = _by_definition(x[1, :200], 10, 50)
    assert 90 <= c0 <= 100 and 90 <= c1 <= 100 and d0 < -60.0 and d1 < -60.0  # (a step of 70 pA at sample 100)
    assert info.tolist() == [[0, 0, 0, 1], [0, 0, 0, 0], [2, 10, 9, 0], [-1, 0, 0, 0]]
    assert shift.tolist() == [c0 + 5, c1 + 5, 0, 0] and cand.tolist() == [c0, c1, -1, -1] and diff[2] == diff[3] == 0.0
    assert abs(diff[0] - d0) < 1e-4 and abs(diff[1] - d1) < 1e-4
    assert 200 - int(shift[1]) < 150 <= 300 - int(shift[0])
    assert out[1:].tobytes() == rows[1:].tobytes()  # not accepted, ValueError, failing: every byte stays
    s0 = int(shift[0])
    assert out["col"][0, [O.C_START, O.C_END, O.C_LEN]].tolist() == [s0, 300, 300 - s0]
    assert out["col"][0, O.C_MEAN:O.C_MEAN + 4].tolist() == [float(np.mean(x[0, s0:300])), float(np.std(x[0, s0:300])), 80.0, 0.0]
    assert out["reserved_"].tolist() == [8, 0, 0, 0] and int(out["present"][0]) == int(rows["present"][0])
    changed = [f for f in rows.dtype.names if out[0][f].tobytes() != rows[0][f].tobytes()]
    assert changed == ["col", "reserved_"] and np.flatnonzero(out["col"][0] != rows["col"][0]).tolist() == [2, 4, 5, 6, 7, 8]
    # an absent adapter_start counts as 0 and becomes present when the row is patched; the statistics end at the adapter's end
    p.min_adapter_len = 0
    out2, info2, *_ = O.front(x, rows, p)
    assert info2[1, 3] == 1 and int(out2["present"][1]) == int(rows["present"][1]) | 4 and out2["col"][1, O.C_START] == shift[1]
    assert out2["col"][1, O.C_MEAN] < 100.0 and out2["col"][1, O.C_LEN] == 200 - shift[1]
    # bounds outside the row: not looked at
    far = O.make_rows([(0, 401), (350, 300)])
    assert O.front(x[:2], far, p)[1][:, 0].tolist() == [-1, -1]
