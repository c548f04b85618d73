"""The host side of the native CSV writer (adp_format_rows, Engine.format_csv, `detect --native_csv`), without a GPU: the option,
the pinned signatures, the new header against its prototype table, the string table, the number rule of
adapted_amd/csrc/csv_api.h against pandas below the bounds that header states, and the writer's file cutting on a stand-in engine."""
import ctypes
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest

import native_csv_cases as cases
from test_cnn_i16_cpu import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adapted_hip_csv.h")
KERNELS = os.path.join(ROOT, "adapted_amd", "csrc", "csv_api.h")


def test_the_parser_knows_the_option_and_it_is_off_by_default():
    from adapted_amd import main as cli

    p = cli.build_parser()
    assert p.parse_args(["detect", "-i", "x"]).native_csv is False
    assert p.parse_args(["detect", "-i", "x", "--native_csv"]).native_csv is True
    with pytest.raises(SystemExit):
        p.parse_args(["continue", "dir", "--native_csv"])  # (`continue` takes it from command.json)


def test_the_pinned_signature_tails_are_unchanged():
    from adapted_amd import main as cli

    params = inspect.signature(cli.run_detect).parameters
    assert list(params)[-4:] == ["fingerprints", "polya_length", "adapter_nt", "event_params"]
    assert list(params)[-5] == "adapter_front"  # (pinned by tests/test_adapter_front_cpu.py: the new parameter stands in front of it)
    assert list(params).index("native_csv") < list(params).index("fingerprints") and params["native_csv"].default is False
    assert list(inspect.signature(cli._Writer.__init__).parameters) == ["self", "run_dir", "batch", "bidx_pass", "bidx_fail", "polya_length"]
    assert list(inspect.signature(cli._Writer.enable_native_csv).parameters) == ["self", "engine", "primary"]


def test_prototype_table_matches_its_header():
    from adapted_amd import lib

    declared = _prototypes(HEADER)
    assert sorted(declared) == sorted(lib.CSV_PROTOTYPES) == ["adp_format_rows"]
    others = (set(lib.PROTOTYPES) | set(lib.MODULE_PROTOTYPES) | set(lib.I16_PROTOTYPES) | set(lib.EVENT_PROTOTYPES)
              | set(lib.FINGERPRINT_PROTOTYPES) | set(lib.ADAPTER_FRONT_PROTOTYPES) | set(lib.REVALIDATE_PROTOTYPES)
              | set(lib.TEMPLATE_PROTOTYPES) | set(lib.EXPORTS))
    assert not set(lib.CSV_PROTOTYPES) & others
    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = fh.read()
    assert text.count('#include "adapted_hip_csv.h"') == 1
    assert text.index('#include "adapted_hip_resegment.h"') < text.index('#include "adapted_hip_csv.h"') < text.index("adp_set_profiling")
    with open(HEADER) as fh:
        assert [ln.split()[1] for ln in fh if ln.startswith("#define")] == ["ADAPTED_HIP_CSV_H"]
    L = lib.load()
    for name, (ret, params) in declared.items():
        got_ret, got_params = lib.CSV_PROTOTYPES[name].split(":")
        assert got_ret == ret and got_params.split() == params, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        for q, t in zip(params, fn.argtypes):
            if q in lib._SCALARS:
                assert t is lib._SCALARS[q], (name, q)
            elif q[:-1] in lib._ELEMENTS:
                assert isinstance(t, lib._Pointer) and t.element == q[:-1], (name, q)
            else:
                assert t is ctypes.c_void_p and q == "adp_handle*", (name, q)
    # refused before the library is entered, and by the library without a handle
    size, bad = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int32)
    assert L.adp_format_rows(None, None, 0, 0, 0, None, None, None, None, None, None, 69, None, 0, size, bad) < 0
    with pytest.raises(ctypes.ArgumentError):
        L.adp_format_rows(None, np.zeros(1, dtype=np.float64), 1, 0, 0, None, None, None, None, None, None, 69, None, 0, size, bad)


def _defines(path):
    with open(path) as fh:
        return dict(re.findall(r"^#define (CSV_\w+) ([^\s/]+)", fh.read(), re.M))


def test_the_string_table_is_made_of_the_one_source_and_laid_out_as_the_kernels_index_it():
    from adapted_amd import lib
    from adapted_amd.output import CSV_COLUMNS

    d = _defines(KERNELS)
    raw, off = lib.csv_string_table()
    assert off.dtype == np.int32 and off.size == int(d["CSV_N_STR"]) + 1 == 70 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == raw.size
    text = [bytes(raw[off[k]:off[k + 1]]).decode() for k in range(69)]
    f, s, r, m, h = (int(d[k]) for k in ("CSV_S_FAIL", "CSV_S_SPT", "CSV_S_RESEG", "CSV_S_MVS", "CSV_S_HEAD"))
    assert (f, s, r, m, h) == (0, 16, 19, 35, 67)
    assert text[f:f + 16] == [lib.FAIL_REASONS[c] or "" for c in range(16)] and text[s:s + 3] == [lib.START_PEAK_TYPES[c] or "" for c in range(3)]
    assert text[r + 2] == "resegmented: first pass failed (adapter MAD check failed)" and text[r + 7].endswith("(MVS polya check failed)")
    row = lib.empty_rows(1)
    for mask in range(32):
        row["fail_code"], row["mvs_fail_mask"] = 7, mask
        assert text[f + 7] + text[m + mask] == lib.fail_reason_of(row[0])
    assert text[h] == ",".join(CSV_COLUMNS) + "\n" and text[h + 1] == ",".join(CSV_COLUMNS + ["fail_reason"]) + "\n"
    # the header lines are pandas' for such files
    for fail in (False, True):
        rows, ids = cases.random_file(3, 4, "llr", fail)
        assert lib.rows_csv_text(rows, ids, "llr", fail).decode().split("\n")[0] + "\n" == text[h + int(fail)]
    assert lib.rows_csv_text(rows[:0], [], "llr", True) == b"\n"
    assert float(d["CSV_F64_BOUND"]) == lib.CSV_F64_BOUND == 2.0 ** 43 and float(d["CSV_F32_BOUND"].rstrip("f")) == lib.CSV_F32_BOUND == 2.0 ** 14


def _rule(x, f32):
    """csv_f64 / csv_f32 of adapted_amd/csrc/csv_api.h in numpy: n = rint(|x| * 1000) in the column's precision, then n / 1000 as a
    decimal with trailing zeros trimmed to one, x's sign in front; inf and -inf; nothing for NaN"""
    t = np.float32 if f32 else np.float64
    x = np.asarray(x, dtype=t)
    a = np.abs(x)
    n = np.rint(a * t(1000)).astype(t)
    out = []
    for v, k in zip(x.tolist(), n.tolist()):
        if v != v:
            out.append("")
        elif abs(v) == float("inf"):
            out.append("-inf" if v < 0 else "inf")
        else:
            k = int(k)
            frac = ("%03d" % (k % 1000)).rstrip("0") or "0"
            out.append(("-" if np.signbit(v) else "") + "%d.%s" % (k // 1000, frac))
    return out


def _pandas(x):
    """the cells of a column as today's writer prints them (beside a second column: a lone empty cell would be quoted)"""
    lines = pd.DataFrame({"a": x, "b": 0}).round(3).to_csv(index=False, header=False).split("\n")[:-1]
    assert all(ln.endswith(",0") for ln in lines)
    return [ln[:-2] for ln in lines]


def _ties(t, top):
    k = np.arange(0, top * 1000, max(1, top * 1000 // 50000), dtype=np.float64)
    return np.concatenate([(k + 0.5) / 1000.0, k / 1000.0 + 0.0005, k / 1000.0 + 0.0015, -(k + 0.5) / 1000.0]).astype(t)


@pytest.mark.parametrize("f32", [False, True])
def test_the_trimmed_decimal_rule_is_pandas_text_below_the_bound(f32):
    """below |x| < 2^43 (float64) and |x| < 2^14 (float32) the decimal n / 1000 IS the shortest text that reads back as
    round(x, 3): half a unit in the last place stays below 0.0005 there and x * 1000 keeps integer precision.  A dense sample, not
    all values: log-uniform over the whole range below the bound, uniform over the top binade, the values next to the bound, ties at
    the third decimal (x.0005, x.0015, exact halves of a thousandth), zeros of both signs, |x| < 0.0005, NaN and the infinities."""
    from adapted_amd import lib

    t, bound = (np.float32, lib.CSV_F32_BOUND) if f32 else (np.float64, lib.CSV_F64_BOUND)
    rng = np.random.default_rng(17 + f32)
    sign = lambda n: rng.choice([-1.0, 1.0], n)
    parts = [sign(300000) * np.exp2(rng.uniform(-30, np.log2(bound), 300000)), sign(200000) * rng.uniform(bound / 2, bound, 200000),
             rng.normal(90.0, 40.0, 200000), _ties(t, 16000), sign(50000) * rng.uniform(0, 0.0006, 50000),
             np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, 0.0005, -0.0005, 0.0015, 1.0, -1.0, 0.001, 0.0004999])]
    top = np.nextafter(t(bound), t(0))
    parts.append(top - np.arange(100000) * (top - np.nextafter(top, t(0))))  # the 100000 values next below the bound
    x = np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]).astype(t)
    x = x[~(np.isfinite(x) & (np.abs(x) >= t(bound)))]
    assert x.dtype == t and x.size > 900000 and np.abs(x[np.isfinite(x)]).max() == top
    got, want = _rule(x, f32), _pandas(x)
    wrong = [(float(v), g, w) for v, g, w in zip(x, got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])


def test_beyond_the_float32_bound_the_rule_does_leave_pandas_text():
    """why the bound is there: above 2^14 a float32 times 1000 no longer has integer precision, and the shortest text of the
    rounded value is not always n / 1000 -- the rows the kernel counts instead of printing"""
    rng = np.random.default_rng(5)
    x = rng.uniform(2.0 ** 14, 2.0 ** 17, 200000).astype(np.float32)
    assert sum(g != w for g, w in zip(_rule(x, True), _pandas(x))) > 0


def test_a_file_with_a_none_prints_its_int_and_float32_columns_through_float64():
    """the dtype switches the kernels' column state stands for, on the pandas writer itself"""
    from adapted_amd import lib

    rows, ids = cases.random_file(1, 6, "llr", False, modes={**{c: 0 for c in range(lib.NCOL)}, "cand": 2, "open_pores": 2})
    rows["reserved_"] = 0
    rows["col"][:, 2], rows["col"][:, 23] = 4040, np.float32(23.5115)
    cols = lib.rows_csv_text(rows, ids, "llr").decode().split("\n")[0].split(",")
    cell = lambda text, name: text.split("\n")[1].split(",")[cols.index(name)]
    whole = lib.rows_csv_text(rows, ids, "llr").decode()
    assert cell(whole, "adapter_start") == "4040" and cell(whole, "start_peak_pa") == "23.512"
    rows["present"][3] &= ~np.uint64((1 << 2) | (1 << 23))
    mixed = lib.rows_csv_text(rows, ids, "llr").decode()
    assert cell(mixed, "adapter_start") == "4040.0" and cell(mixed, "start_peak_pa") == "23.511"


class _StandIn:
    """an engine whose format_csv is the pandas writer: what the writer's file cutting is held against"""
    csv_files = csv_fallback_files = 0

    def __init__(self):
        self.calls = []

    def format_csv(self, rows, read_ids, primary, fail=False, consume=False):
        from adapted_amd import lib

        assert rows.dtype == lib.ROW_DTYPE and len(read_ids) == len(rows) and consume
        self.calls.append((len(rows), fail))
        return lib.rows_csv_text(rows, read_ids, primary, fail, consume=consume)


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_the_writer_cuts_the_same_files_from_rows_as_from_results(tmp_path):
    """_Writer.add_rows against _Writer.add over three detect calls and files of 24: the files straddle the calls, the last ones are
    short, an exception row goes to the failed reads whatever its success says, and every file is formatted from ITS rows"""
    from adapted_amd import lib
    from adapted_amd import main as cli
    from adapted_amd.container_types import ReadResult

    calls = []
    for k, n in enumerate((64, 64, 22)):
        rows, ids = cases.random_file(40 + k, n, "cnn", True)
        exc = (rows["fail_code"] >= 9) & (rows["fail_code"] <= 14)
        rows["success"] = np.arange(n) % 3 != 0
        rows["fail_code"][(rows["success"] != 0) & ~exc] = 0
        calls.append((rows, ["c%d_%s" % (k, i) for i in ids]))
    old = cli._Writer(str(tmp_path / "old"), 24)
    new = cli._Writer(str(tmp_path / "new"), 24)
    eng = _StandIn()
    new.enable_native_csv(eng, "cnn")
    for rows, ids in calls:
        res = lib.rows_to_results(rows, "cnn")
        old.add([ReadResult(read_id=str(i), success=r.success, fail_reason=r.fail_reason, detect_results=r) for i, r in zip(ids, res)])
        new.add_rows(rows, np.asarray(ids, dtype=object))
    old.close()
    new.close()
    a, b = _tree(str(tmp_path / "old")), _tree(str(tmp_path / "new"))
    assert a.keys() == b.keys() and len(a) >= 6 and a == b
    assert old.n == new.n and old.bidx == new.bidx and sum(n for n, _ in eng.calls) == 150
    assert max(n for n, _ in eng.calls) == 24 and len([n for n, _ in eng.calls if n < 24]) <= 2
