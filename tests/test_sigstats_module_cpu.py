"""The reference's signal statistics modules (adapted/partition/signal_partitions.py, adapted/detect/normalize.py, downscale.py,
real_range.py, anomalies.py): the CPU restatement
(tests/sigstats_module_restated.py) against the vectors the REAL reference produced (tests/golden/sigstats_module.npz,
tools/gen_sigstats_module_golden.py) bit for bit, and the drop-in's names, signatures, imports and host-side checks."""
import os
import re
import sys
import types
import warnings

import numpy as np
import pytest

import sigstats_module_cases as M
import sigstats_module_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sigstats_module.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
RESTATED = types.SimpleNamespace(**{nm: getattr(R, nm) for names in M.DETECT_NAMES.values() for nm in names})


def _dropins():
    import importlib

    mods = {key: importlib.import_module("adapted_amd.detect." + key) for key in M.DETECT_NAMES}
    return mods, types.SimpleNamespace(**{nm: getattr(mods[key], nm) for key, names in M.DETECT_NAMES.items() for nm in names})


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES])
def test_restated_matches_reference(gold, name):
    from adapted_amd.container_types import Boundaries

    case = M.by_name(name)
    x64, names = M.inputs(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dt in M.DTYPES:
            x = M.as_dtype(x64, dt)
            for i, c in enumerate(case["calls"]):
                want = str(gold["%s.%s.%s" % (name, dt, M.call_key(i, c))])
                assert M.call(R, Boundaries, x, names, c) == want, (dt, i, c)


def test_fixture_covers_every_branch(gold):
    """the cases reach every sample count of M.COUNTS, the None results, the unclipped length, the NaN rules and MAD == 0"""
    stats = {k: str(gold[k]) for k in gold.files if k.endswith(".stats")}
    vals = {k: str(gold[k]) for k in gold.files if k.endswith(".vals")}
    for c in M.COUNTS:
        assert any(v.startswith("Partition(start=int:1000, len=int:%d, mean=float:0x" % c) for v in stats.values()), c
    none5 = "len=NoneType:None, mean=NoneType:None, std=NoneType:None, med=NoneType:None, mad=NoneType:None)"
    nan4 = "mean=float:nan, std=float:nan, med=float:nan, mad=float:nan)"
    # None positions, end <= start (equal and below), the all-None RNA partition of a truncated read
    assert any(v.startswith("Partition(start=NoneType:None, " + none5) for v in stats.values())
    assert any(v.startswith("Partition(start=int:10, " + none5) for v in stats.values())
    assert sum("rna=Partition(start=NoneType:None, " + none5 in v for v in vals.values()) >= 6
    assert "adapter=Partition(start=int:300, " + none5 in vals["end_before_start.f32.01.vals"]
    # end beyond the read: the full end - start with the clipped slice's statistics; start at / beyond the size: NaN x 4
    n = 6000
    assert str(gold["beyond.f32.06.stats"]).startswith("Partition(start=int:0, len=int:%d, mean=float:0x" % (n + 1))
    assert str(gold["beyond.f32.03.stats"]).startswith("Partition(start=int:%d, len=int:10, %s" % (n, nan4))
    assert str(gold["beyond.f32.05.stats"]).startswith("Partition(start=int:%d, len=int:1, %s" % (n + 5, nan4))
    assert str(gold["empty_read.f64.00.stats"]).startswith("Partition(start=int:0, len=int:5, " + nan4)
    # a NaN sample makes all four NaN, in each partition and in the last sample; integer input has none
    for case, part in (("nan_adapter", "adapter"), ("nan_polya", "polya"), ("nan_rna", "rna"), ("nan_tail", "rna")):
        for dt in ("f32", "f64"):
            v = vals["%s.%s.00.vals" % (case, dt)]
            assert "%s=Partition(start=int:" % part in v and v.split("%s=Partition(" % part)[1].split(")")[0].endswith(nan4[:-1]), (case, dt)
            assert v.count("mean=float:nan") == 1
        assert "nan" not in vals["%s.i32.00.vals" % case]
    assert str(gold["nan_adapter.f32.02.stats"]).startswith("Partition(start=int:500, len=int:1, " + nan4)
    assert "nan" not in str(gold["nan_adapter.f32.03.stats"])
    # MAD == 0 and std == 0 on a constant stretch; massive ties on the quantised read
    assert "std=float:0x0.0p+0, med=float:0x1.2c00000000000p+6, mad=float:0x0.0p+0" in vals["constant.f32.00.vals"]
    assert "nan" not in vals["quantised.f32.00.vals"]
    # every statistic is a Python float, every length an int; float32 values are float32 exactly (their last 29 bits are 0)
    v = str(gold["clean.f32.00.vals"])
    assert "np." not in v and v.count("float:0x") == 3 * 4 * 3
    f32 = [float.fromhex(h) for h in re.findall(r"float:(-?0x[0-9a-f.]+p[+-][0-9]+)", v)]
    f64 = [float.fromhex(h) for h in re.findall(r"float:(-?0x[0-9a-f.]+p[+-][0-9]+)", str(gold["clean.f64.00.vals"]))]
    assert len(f32) == len(f64) == 36 and all(h == float(np.float32(h)) for h in f32) and any(h != float(np.float32(h)) for h in f64)


@pytest.mark.parametrize("key", ["%s.%s" % (c["module"], c["name"]) for c in M.DETECT_CASES])
def test_restated_detect_modules_match_reference(gold, key):
    from adapted_amd.config.schema import RealRangeConfig

    case = M.detect_case(*key.split("."))
    x64 = M.detect_input(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for dt in case["dtypes"]:
            x = M.as_dtype(x64, dt)
            for i, c in enumerate(case["calls"]):
                assert M.detect_call(RESTATED, RealRangeConfig, x, c) == str(gold[M.detect_key(case, dt, i, c)]), (dt, i, c)


def test_fixture_covers_every_detect_branch(gold):
    g = {k: str(gold[k]) for k in gold.files}
    norm = {k: v for k, v in g.items() if k.startswith("normalize.")}
    # normalize: MAD 0 raises; NaN makes both NaN unless with_nan; float32 stays float32; the empty input gives float64 []
    assert sum(v == "raise ValueError: MAD normalization failed: scale is 0" for v in norm.values()) >= 12
    assert g["normalize.nan_read.f32.00.med_mad"] == "(float:nan, float:nan)" and "nan" not in g["normalize.nan_read.f32.01.med_mad"]
    assert g["normalize.minibatch_big.f64.00.med_mad"] == "(float:nan, float:nan)" and "nan" not in g["normalize.minibatch_big.f64.01.med_mad"]
    assert g["normalize.allnan.f32.01.med_mad"] == "(float:nan, float:nan)"
    assert g["normalize.read_odd.f32.02.normalize"].startswith("ndarray[float32](9001,) sha256:")
    assert g["normalize.read_300k.f64.02.normalize"].startswith("ndarray[float64](300001,) sha256:")
    assert g["normalize.minibatch_big.f32.03.normalize"].startswith("ndarray[float32](64, 6000) sha256:")
    assert g["normalize.rank3.f32.05.clip"].startswith("ndarray[float32](2, 3, 50) sha256:")
    assert g["normalize.empty.f32.02.normalize"] == "ndarray[float64](0,)[]" == g["normalize.empty2d.f32.02.normalize"]
    assert g["normalize.empty2d.f32.05.clip"] == "ndarray[float32](0, 5)[]"
    assert g["normalize.mostly_constant.f32.06.stretch"].startswith("raise ValueError: MAD")
    # downscale: every pool size on an exact and on a ragged width; the pool beyond the row; not 2-D
    for i, p in enumerate(M.POOLS):
        assert g["downscale.exact.f32.%02d.pool" % i].startswith("ndarray[float32](5, %d)" % (6720 // p))
        assert g["downscale.ragged.f64.%02d.pool" % i].startswith("ndarray[float64](4, %d)" % (-(-6719 // p)))
    assert g["downscale.ragged.f32.07.pool"].startswith("ndarray[float32](4, 1)")
    assert g["downscale.not_2d.f32.00.pool"] == "raise ValueError: Data must be a 2D array" == g["downscale.rank3.f64.00.pool"]
    # real_range: too short; each mean failing; the local range failing on both sides and passing; both window settings
    rr = {k: v for k, v in g.items() if k.startswith("real_range.") and ".f32." in k}
    assert rr["real_range.too_short.f32.01.rr"] == "(bool:False, NoneType:None, NoneType:None, NoneType:None)"
    assert rr["real_range.too_short.f32.00.rr"] == "bool:False" and rr["real_range.too_short.f32.02.rr"].startswith("(bool:True, np.float32:0x")
    for nm in ("start_low", "end_high", "nan_start"):
        assert rr["real_range.%s.f32.01.rr" % nm].startswith("(bool:False, np.float32:") and rr["real_range.%s.f32.01.rr" % nm].endswith("NoneType:None)")
    for nm in ("range_small", "range_large"):
        assert rr["real_range.%s.f32.01.rr" % nm].startswith("(bool:False, np.float32:0x") and "np.float64:0x" in rr["real_range.%s.f32.01.rr" % nm]
    assert rr["real_range.nan_tail.f32.01.rr"].endswith("np.float64:nan)")
    # (max_obs_local_range 5000 and 9000: both beyond the 4000 samples; 700: the tail alone, its range below the bound)
    assert rr["real_range.pass.f32.01.rr"] == rr["real_range.pass.f32.02.rr"] != rr["real_range.pass.f32.03.rr"]
    assert rr["real_range.pass.f32.01.rr"].startswith("(bool:True") and rr["real_range.pass_long.f32.01.rr"].startswith("(bool:True")
    assert "np.float64:" in g["real_range.pass.i32.01.rr"].split(", ")[1]
    # anomalies: every shape the reference returns
    assert g["anomalies.none.f32.00.op"] == "ndarray[int64](0, 1)[]" and g["anomalies.one.f32.00.op"] == "ndarray[int64](1, 1)[1500]"
    assert g["anomalies.one_run.f32.00.op"] == "ndarray[int64](1,)[708]" and g["anomalies.one_run.f32.01.op"].startswith("ndarray[int64](8, 1)[701, ")
    assert g["anomalies.two_close.f32.00.op"] == "ndarray[int64](1,)[704]" and g["anomalies.two_close.f32.01.op"] == "ndarray[int64](1, 1)[704]"
    assert g["anomalies.many.f32.00.op"].startswith("ndarray[int64](58, 1)[617, 917, ")
    assert g["anomalies.many.f32.02.op"] != g["anomalies.many.f32.00.op"] and g["anomalies.many.f32.02.op"].startswith("ndarray[int64](")
    assert g["anomalies.bound_not_float32.f32.00.op"] != g["anomalies.bound_not_float32.f64.00.op"]


def test_module_names_and_signatures(gold):
    import adapted_amd.partition.signal_partitions as sp
    from adapted_amd.partition import signal_partitions  # noqa: F401

    assert sorted(str(s) for s in gold["names"]) == sorted(M.NAMES)
    for nm in M.NAMES:
        assert callable(getattr(sp, nm))
    assert M.signature_rows(sp) == [str(s) for s in gold["signatures"]]
    assert M.signature_rows(R) == [str(s) for s in gold["signatures"]]
    for nm in ("calc_partition_stats_batch", "calc_partitions_from_vals_batch"):
        assert callable(getattr(sp, nm))
    mods, _ = _dropins()
    for key, names in M.DETECT_NAMES.items():
        assert sorted(str(v) for v in gold["names." + key]) == sorted(names)
        assert M.signature_rows(mods[key], names) == [str(v) for v in gold["signatures." + key]], key
        assert M.signature_rows(R, names) == [str(v) for v in gold["signatures." + key]], key
    for key, nm in (("normalize", "med_mad_batch"), ("normalize", "normalize_signal_batch"), ("downscale", "efficient_average_pooling_device"),
                    ("real_range", "real_range_check_batch"), ("anomalies", "find_open_pores_batch")):
        assert callable(getattr(mods[key], nm))


def test_dataclasses_without_the_gpu():
    import adapted_amd.partition.signal_partitions as sp

    p = sp.Partition(3, 4, 1.0, 2.0, 3.0, 4.0)
    none = sp.Partition(None, None, None, None, None, None)
    assert p.to_dict() == dict(start=3, len=4, mean=1.0, std=2.0, med=3.0, mad=4.0)
    assert list(p.to_dict("x")) == ["x_start", "x_len", "x_mean", "x_std", "x_med", "x_mad"]
    d = sp.Partitions(p, none, p).to_dict("r")
    assert list(d)[:2] == ["r_adapter_start", "r_adapter_len"] and len(d) == 18 and d["r_polya_mean"] is None and d["r_rna_mad"] == 4.0
    assert M.enc(sp.Partitions(p, none, p)) == M.enc(R.Partitions(R.Partition(3, 4, 1.0, 2.0, 3.0, 4.0), R.Partition(*[None] * 6),
                                                                  R.Partition(3, 4, 1.0, 2.0, 3.0, 4.0)))


def test_host_side_validation():
    import adapted_amd.partition.signal_partitions as sp

    x = np.zeros(100, np.float32)
    with pytest.raises(ValueError):
        sp.calc_partition_stats(x, -1, 50)
    with pytest.raises(ValueError):
        sp.calc_partition_stats(x, 0, -3)
    with pytest.raises(ValueError):
        sp.calc_partitions_from_vals(x, 0, -2, 50)
    with pytest.raises(TypeError):
        sp.calc_partition_stats(np.zeros(10, dtype=np.complex64), 0, 5)
    with pytest.raises(ValueError):
        sp.calc_partition_stats_batch(np.zeros((2, 10), np.float32), [10, 11], [0, 0], [5, 5])
    with pytest.raises(ValueError):
        sp.calc_partition_stats_batch(np.zeros((2, 10), np.float32), [10, 10], [0], [5, 5])
    with pytest.raises(ValueError):
        sp.calc_partitions_from_vals_batch(np.zeros((2, 10), np.float32), [10, 10], [0, 0], [5, -2], [7, 7])
    with pytest.raises(ValueError):
        sp.calc_partition_stats_batch(1 << 40, [10, 10], [0, 0], [5, 5])  # (a device pointer needs n and L)
    # nothing to compute: no library call
    length, stats = sp.calc_partition_stats_batch(np.zeros((2, 10), np.float64), [10, 10], [-1, 4], [5, 4])
    assert length.tolist() == [-1, -1] and np.isnan(stats).all() and stats.shape == (2, 4)
    assert sp.calc_partition_stats(x, None, 5) == sp.Partition(None, None, None, None, None, None)
    assert sp.calc_partition_stats(x, 7, 7) == sp.Partition(7, None, None, None, None, None)


def test_detect_modules_answer_without_the_gpu_where_nothing_is_computed():
    """host-side validation and the results that need no statistics"""
    from adapted_amd.config.schema import RealRangeConfig

    mods, d = _dropins()
    x = np.zeros(100, np.float32)
    assert d.normalize_signal(np.zeros(0, np.float32)).dtype == np.float64 and d.normalize_signal([]).shape == (0,)
    mm = d.med_mad(np.zeros((0, 4)))
    assert mm[0] != mm[0] and mm[1] != mm[1] and type(mm[0]) is float
    assert d.clip_signal(np.zeros((0, 5), np.float32), 5.0, 1.0, 1.0).shape == (0, 5)
    with pytest.raises(TypeError):
        d.med_mad(np.zeros(4, dtype=np.complex64))
    for bad in (np.zeros(8), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match="Data must be a 2D array"):
            d.efficient_average_pooling(bad, 2)
    with pytest.raises(ValueError):
        d.efficient_average_pooling(np.zeros((2, 8)), 0)
    assert d.efficient_average_pooling(np.zeros((0, 5), np.float32), 2).shape == (0, 3)
    assert d.downscale_signal(np.zeros((3, 0))).shape == (3, 0)
    assert d.real_range_check(x, RealRangeConfig()) is False
    assert d.real_range_check(x, RealRangeConfig(), True) == (False, None, None, None)
    bad = RealRangeConfig()
    bad.mean_window = 0
    with pytest.raises(ValueError):
        d.real_range_check(x, bad)
    with pytest.raises(ValueError):
        mods["real_range"].real_range_check_batch(np.zeros((2, 10), np.float32), [10, 10], [0, -1], [5, 5], RealRangeConfig())
    r = d.find_open_pores(np.zeros(0, np.float32))
    assert r.shape == (0, 1) and r.dtype == np.int64
    with pytest.raises(ValueError):
        d.find_open_pores(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        mods["anomalies"].find_open_pores_batch(np.zeros((2, 10), np.float32), [10, 10], [0, 0], [5])
    with pytest.raises(ValueError):
        mods["normalize"].med_mad_batch(np.zeros((2, 10), np.float32), [10, 11])
    assert mods["normalize"].med_mad_batch(np.zeros((0, 10), np.float32), []).shape == (0, 2)


def test_struct_sizes_match_library():
    """struct adp_seg and adp_real_range_args: the mirrors in adapted_amd/lib.py against the library's own sizes"""
    import ctypes

    from adapted_amd import lib

    L = lib.load()
    assert L.adp_sizeof_seg() == lib.SEG_DTYPE.itemsize == 24
    assert L.adp_sizeof_real_range_args() == ctypes.sizeof(lib.AdpRealRangeArgs) == 56
    for nm in ("adp_seg_stats", "adp_med_mad", "adp_normalize", "adp_pool_mean", "adp_real_range", "adp_open_pores"):
        assert nm in lib.EXPORTS and hasattr(L, nm)
