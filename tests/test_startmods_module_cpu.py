"""The reference's start-peak and adapter-start modules (adapted/detect/start_peak.py, adapter_start.py): the CPU restatement
(tests/startmods_module_restated.py) against the vectors the REAL reference produced (tests/golden/startmods_module.npz,
tools/gen_startmods_module_golden.py) -- values, Python types, exception texts and None cells, exactly --, the drop-ins' names,
signatures and imports, MMAdapterStartConfig, and the arguments refused on the host."""
import os
import sys
import types
import warnings

import numpy as np
import pytest

import startmods_module_cases as M
import startmods_module_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "startmods_module.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _restated_frame(X, lens, spc):
    if (np.minimum(np.asarray(lens), X.shape[1]) // spc.rna_start_peak.downscale_factor == 0).any():
        raise ValueError("attempt to get argmax of an empty sequence")
    return R.start_peak_frame(X, lens, spc.rna_start_peak)


@pytest.mark.parametrize("dt", M.AS_DTYPES)
def test_restated_adapter_start_matches_reference(gold, dt):
    from adapted_amd.config.schema import MMAdapterStartConfig

    for case in M.AS_CASES:
        x = M.as_dtype(M.as_input(case), dt)
        assert M.as_call(R.adapter_start, x, M.as_params(MMAdapterStartConfig, case)) == str(gold["as.%s.%s" % (case["name"], dt)]), case["name"]


@pytest.mark.parametrize("name", [c["name"] for c in M.SP_CASES])
def test_restated_start_peak_matches_reference(gold, name):
    from adapted_amd.config.schema import RNAStartPeakConfig

    case = M.sp_by_name(name)
    sec = M.sp_section(RNAStartPeakConfig, case)
    X64, lens = M.sp_input(case, sec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dt in M.SP_DTYPES:
            got = M.sp_call(_restated_frame, M.sp_as_dtype(X64, dt), lens, types.SimpleNamespace(rna_start_peak=sec))
            assert M.frame_diff(got, M.sp_want(gold, name, dt), dtypes=M.same_pandas(gold)) == [], dt


def test_fixture_covers_every_branch(gold):
    vals = {k: str(gold[k]) for k in gold.files if k.startswith("as.")}
    assert str(gold["as.two_levels.f32"]) == "np.int64:1492" and str(gold["as.constant.f64"]) == "int:0"
    assert str(gold["as.low_current.f32"]) == "int:0" and str(gold["as.nan_used.f32"]) == "int:0"
    assert str(gold["as.nan_trimmed.f64"]) == str(gold["as.two_levels_noise.f64"]) != "int:0"
    assert str(gold["as.empty.f32"]).endswith("must between 1 and 0, inclusive")
    assert str(gold["as.just_short.f32"]) == "raise ValueError: Moving window (=100) must between 1 and 99, inclusive"
    assert str(gold["as.long_200k.f32"]) != str(gold["as.long_200k.f64"])  # (the type matters)
    for w, mo in M.AS_PARAMS:
        sweep = [vals["as.sweep.w%d.mo%d.L%d.f32" % (w, mo, ls)] for ls in M.as_diff_sizes(w)]
        assert sweep[0] == "int:0" and not any(v.startswith("raise") for v in sweep)
        assert w == 1 or any(v.startswith("np.int64:") for v in sweep), (w, mo)
    flags = set()
    for k in gold.files:
        if k.endswith(".flagged_type"):
            flags |= set(gold[k].tolist())
    assert flags == {"", "open pore in adapter", "potential concatemer adapter-only read"}
    assert gold["sp.rna004_2000.f32.start_peak_idx.none"].all() and "object" in str(gold["sp.rna004_2000.f32.dtypes"])
    assert np.isnan(gold["sp.rna004_17500.f32.start_peak_pa"][~gold["sp.rna004_17500.f32.start_peak_pa.none"]]).any()
    assert str(gold["sp.scan_raises.f32.raise"]) == "raise ValueError: attempt to get argmax of an empty sequence"


def test_modules_import_without_a_gpu_and_define_the_reference_names(gold):
    from adapted_amd.detect import adapter_start, start_peak

    for key, mod in (("start_peak", start_peak), ("adapter_start", adapter_start)):
        assert [str(s) for s in gold["names." + key]] == sorted(M.NAMES[key])
        assert M.signature_rows(mod, M.NAMES[key]) == [str(s) for s in gold["signatures." + key]]
    assert callable(start_peak.detect_rna_start_peak_batch) and callable(adapter_start.moving_mean_adapter_start_detect_batch)
    from adapted_amd.detect.adapter_start import MMAdapterStartConfig  # noqa: F401  (the reference module holds the name too)


def test_detect_package_defines_every_reference_module():
    import importlib

    for nm in ("_c_llr", "adapter_start", "anomalies", "cnn", "combined", "downscale", "llr", "mvs", "normalize", "real_range",
               "start_peak", "utils"):
        importlib.import_module("adapted_amd.detect." + nm)


def test_mm_adapter_start_config(gold):
    from adapted_amd.config import schema
    from adapted_amd.config.sig_proc import MMAdapterStartConfig, SigProcConfig

    c = MMAdapterStartConfig()
    assert sorted("%s=%r" % kv for kv in vars(c).items()) == [str(s) for s in gold["defaults.MMAdapterStartConfig"]]
    assert (c.detect_adapter_start, c.window, c.min_obs_adapter, c.min_shift, c.min_pA_current) == (False, 100, 2500, 20.0, 90.0)
    assert "mm_adapter_start" not in schema.SECTIONS and MMAdapterStartConfig not in schema.SECTION_CLASSES.values()
    assert not any(isinstance(getattr(SigProcConfig(llr_boundaries=schema.LLRBoundariesConfig(llr_detect=True),
                                                    cnn_boundaries=schema.CNNBoundariesConfig(cnn_detect=False)), f), MMAdapterStartConfig)
                   for f in ("core", "streaming", "rna_start_peak"))


def test_host_side_validation():
    from adapted_amd.config.schema import MMAdapterStartConfig, RNAStartPeakConfig
    from adapted_amd.detect import adapter_start as A
    from adapted_amd.detect import start_peak as S

    x = np.zeros((2, 50), dtype=np.float32)
    p, sec = MMAdapterStartConfig(), RNAStartPeakConfig()
    for lens in ([50], [50, 51], [50, -1]):
        with pytest.raises(ValueError):
            A.moving_mean_adapter_start_detect_batch(x, lens, p)
    with pytest.raises(ValueError):
        A.moving_mean_adapter_start_detect_batch(1 << 20, [50, 50], p)          # a pointer without n / L
    with pytest.raises(ValueError):
        A.moving_mean_adapter_start_detect_batch(1 << 20, [50, 50], p, n=2)
    with pytest.raises(TypeError):
        A.moving_mean_adapter_start_detect_batch(1 << 20, [50, 50], p, n=2, L=50, dtype=np.int32)
    with pytest.raises(TypeError):
        A.moving_mean_adapter_start_detect_batch(x.astype(np.complex64), [50, 50], p)
    bad = MMAdapterStartConfig(window=0)
    with pytest.raises(ValueError):
        A.moving_mean_adapter_start_detect_batch(x, [50, 50], bad)
    with pytest.raises(ValueError, match=r"Moving window \(=0\) must between 1 and 0, inclusive"):
        A.moving_mean_adapter_start_detect(x[0], bad)
    with pytest.raises(ValueError):
        A.moving_mean_adapter_start_detect_batch(x, [50, 50], MMAdapterStartConfig(min_obs_adapter=-1))
    for lens in ([50], [50, -1]):
        with pytest.raises(ValueError):
            S.detect_rna_start_peak_batch(x, lens, sec)
    with pytest.raises(ValueError):
        S.detect_rna_start_peak_batch(1 << 20, [50, 50], sec, n=2)              # a pointer without m
    with pytest.raises(TypeError):
        S.detect_rna_start_peak_batch(1 << 20, [50, 50], sec, n=2, m=50, dtype=np.int16)
    with pytest.raises(TypeError):
        S.detect_rna_start_peak_batch(x.astype(np.complex64), [50, 50], sec)
    with pytest.raises(ValueError):
        S.detect_rna_start_peak_batch(x, [50, 50], RNAStartPeakConfig(downscale_factor=0))
    with pytest.raises(ValueError):
        S.detect_rna_start_peak_batch(x, [50, 50], RNAStartPeakConfig(offset2=-1))
    with pytest.raises(ValueError, match="argmax of an empty sequence"):
        S.detect_rna_start_peak(x, [50, 5], types.SimpleNamespace(rna_start_peak=sec))
    assert S.detect_rna_start_peak_batch(np.zeros((0, 50), dtype=np.float32), [], sec).size == 0


def test_struct_sizes_and_chunk_match_the_sources():
    import ctypes
    import re

    from adapted_amd import lib

    L = lib.load()
    assert L.adp_sizeof_start_peak_args() == ctypes.sizeof(lib.AdpStartPeakArgs) == 24
    assert L.adp_sizeof_adapter_start_args() == ctypes.sizeof(lib.AdpAdapterStartArgs) == 24
    with open(os.path.join(ROOT, "adapted_amd", "csrc", "startmods_api.h")) as fh:
        assert int(re.search(r"#define ASC_CHUNK (\d+)", fh.read()).group(1)) == lib.ADAPTER_START_CHUNK


def test_module_prototype_table_matches_its_header():
    """lib.MODULE_PROTOTYPES restates every prototype of include/adapted_hip_startmods.h (name, return kind, per position the
    scalar kind or the pointer's element), load() binds them, and adapted_hip.h includes that header"""
    import ctypes
    import re

    from adapted_amd import lib

    with open(os.path.join(ROOT, "include", "adapted_hip_startmods.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        assert '#include "adapted_hip_startmods.h"' in fh.read()

    def kind(decl, named):
        m = re.fullmatch(r"(?:const\s+)?(\w+?)(?:_t)?\s*((?:\*\s*)*)" + (r"\w+" if named else ""), decl.strip())
        assert m, decl
        return m.group(1) + "*" * m.group(2).count("*")

    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\**)\s*(adp_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        declared[name] = (kind(ret, False), [] if params.strip() == "void" else [kind(q, True) for q in params.split(",")])
    assert sorted(declared) == sorted(lib.MODULE_PROTOTYPES) == ["adp_adapter_start", "adp_sizeof_adapter_start_args",
                                                                 "adp_sizeof_start_peak_args", "adp_start_peak"]
    assert not set(declared) & set(lib.PROTOTYPES)
    L = lib.load()
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.MODULE_PROTOTYPES[name].split(":")
        assert got_ret == ret and got_params.split() == params, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for q, t in zip(params, fn.argtypes):
            if q in lib._SCALARS:
                assert t is lib._SCALARS[q], (name, q)
            elif q[:-1] in lib._ELEMENTS:
                assert isinstance(t, lib._Pointer) and t.element == q[:-1], (name, q)
            else:
                assert t is (ctypes.c_void_p if q == "adp_handle*" else ctypes.POINTER(lib._POINTEES[q[:-1]])), (name, q)
    with pytest.raises(ctypes.ArgumentError):
        L.adp_adapter_start(None, None, np.zeros(2, dtype=np.int64), 2, 8, None, 0, None, None, None, None)  # int64 for int32 *len


def test_product_does_not_import_the_restatement():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "adapted_amd")):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(dirpath, f)) as fh:
                    text = fh.read()
                assert "startmods_module_restated" not in text and "startmods_module_cases" not in text, f
