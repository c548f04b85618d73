"""Rows for the native CSV writer's tests (Engine.format_csv, include/adapted_hip_csv.h): files of random adp_row records that drive
every switch of the pandas writer they are held against -- each column per FILE all-present, one-absent, all-absent or random (the
dtype of a pandas column is a property of the file), the row views of lib.rows_to_results (second opinion, truncated,
re-segmented, exception rows), the number rule's edge values and numpy's list printing (empty, one entry, wrapped lines, the
overflow registry, the summary beyond 1000 entries)."""
import numpy as np

from adapted_amd import lib


def _floats(rng, n, f32):
    """ordinary pA values, ties at the third decimal (x.0005, x.0015 and exact binary halves of a thousandth), -0.0, |x| < 0.0005 of
    both signs, NaN, +-inf and -- float64 only -- integers up to 2^31; everything inside the writer's bounds"""
    k = rng.integers(0, 200000, n)
    pool = [rng.normal(90.0, 40.0, n), k + 0.0005, k + 0.0015, -(k + 0.0005), (rng.integers(0, 16000, n) * 1000 + rng.integers(0, 1000, n) + 0.5) / 1000.0,
            np.full(n, -0.0), rng.uniform(-0.0005, 0.0005, n), rng.uniform(-0.0005, 0.0, n), np.full(n, np.nan), np.full(n, np.inf),
            np.full(n, -np.inf), rng.integers(0, 2 ** 31, n).astype(np.float64), -rng.integers(0, 2 ** 31, n).astype(np.float64),
            rng.integers(0, 100, n).astype(np.float64), rng.integers(0, 1000, n) / 10.0]
    w = np.asarray([8, 2, 2, 1, 2, 1, 1, 1, 1, 0.5, 0.5, 1, 0.5, 1, 1])
    v = np.stack(pool)[rng.choice(len(pool), n, p=w / w.sum()), np.arange(n)]
    if f32:
        big = np.isfinite(v) & (np.abs(v) >= 16000.0)  # (finite values stay below 2^14)
        v[big] = np.mod(v[big], 16000.0)
        v = v.astype(np.float32).astype(np.float64)
    return v


def _presence(rng, n, mode):
    if mode == 0:
        return np.ones(n, dtype=bool)
    if mode == 1:
        p = np.ones(n, dtype=bool)
        p[rng.integers(0, n)] = False
        return p
    if mode == 2:
        return np.zeros(n, dtype=bool)
    return rng.random(n) < 0.6


def random_file(seed, n, primary, fail, modes=None):
    """(rows, read ids) of one file: ``fail`` a failed_reads file (success 0, fail codes, exception rows), else a
    detected_boundaries file.  modes: {column or "cand" / "open_pores": 0 all-present, 1 one-absent, 2 all-absent, 3 random} for the
    columns the caller wants in a given state; the others are drawn"""
    rng = np.random.default_rng(seed)
    rows = lib.empty_rows(n)
    modes = dict(modes or {})
    present = np.zeros(n, dtype=np.uint64)
    for c in range(lib.NCOL):
        mode = modes.get(c, int(rng.integers(0, 4)))
        if n:
            present |= _presence(rng, n, mode).astype(np.uint64) << np.uint64(c)
        if c in lib._INT_COLS:
            rows["col"][:, c] = rng.choice([rng.integers(0, 200000, n), rng.integers(0, 2 ** 31, n), np.zeros(n, dtype=np.int64)], axis=0) if n else 0
        else:
            rows["col"][:, c] = _floats(rng, n, c in lib._F32_COLS)
    rows["present"] = present
    rows["success"] = 0 if fail else 1
    rows["start_peak_type"] = rng.integers(0, 3, n)
    rows["mvs_fail_mask"] = rng.integers(0, 32, n) | np.where(rng.random(n) < 0.2, 256, 0)
    if fail:
        rows["fail_code"] = rng.choice([1, 2, 3, 4, 5, 6, 7, 7, 8, 15, 9, 10, 11, 12, 13, 14], n)
    res = np.zeros(n, dtype=np.int32)
    res |= np.where(rng.random(n) < 0.5, lib.ROW_TRUNC_LOOKED, 0).astype(np.int32)
    res |= np.where(rng.random(n) < 0.15, lib.ROW_POLYA_TRUNCATED | lib.ROW_TRUNC_LOOKED, 0).astype(np.int32)
    if primary == "cnn":
        res |= np.where(rng.random(n) < 0.3, lib.ROW_FROM_SECOND_LLR, 0).astype(np.int32)
    if primary == "llr":
        first = rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 15], n).astype(np.int32)
        res |= np.where(rng.random(n) < 0.3, lib.ROW_RESEGMENTED | (first << lib.ROW_FIRST_FAIL_SHIFT), 0).astype(np.int32)
    rows["reserved_"] = res
    # the lists: None, empty, one entry, many (wide entries wrap the line), and open_pores beyond what a row holds
    pc = _presence(rng, n, modes.get("cand", int(rng.integers(0, 4)))) if n else np.zeros(0, dtype=bool)
    po = _presence(rng, n, modes.get("open_pores", int(rng.integers(0, 4)))) if n else np.zeros(0, dtype=bool)
    for i in range(n):
        if pc[i]:
            k = int(rng.choice([0, 1, 2, 5, 9, 10, 16]))
            rows["n_cand"][i] = k
            rows["cand"][i, :k] = rng.integers(0, int(rng.choice([10, 5000, 10 ** 7, 2 ** 31])), k)
        if po[i]:
            k = int(rng.choice([0, 1, 3, 16, 17, 40, 999, 1000, 1001], p=[.3, .2, .2, .1, .05, .05, .04, .03, .03]))
            vals = np.sort(rng.integers(0, int(rng.choice([100, 200000, 2 ** 31])), k)).astype(np.int64)
            rows["n_open_pores"][i] = k
            rows["open_pores"][i, :min(k, lib.MAX_OPEN_PORES)] = vals[:lib.MAX_OPEN_PORES]
            if k > lib.MAX_OPEN_PORES:
                rows["open_pores_more"][i] = lib.register_open_pores(vals)
    ids = ["%08x-read-%d" % (int(rng.integers(0, 2 ** 32)), i) for i in range(n)]
    if n > 2:
        ids[1] = 'with,comma'
        ids[2] = 'with "quotes" and, both'
    if n > 5:
        ids[5] = "línea"
    return rows, ids


def planted(rows):
    """plants finite values at and above each bound into a file WITHOUT exception rows -> the set of affected row indices.  The
    float32 bound applies where the column has no None in the file: columns 23 and 25 are made all-present, column 27 mixed"""
    assert rows.size >= 9 and not ((rows["fail_code"] >= 9) & (rows["fail_code"] <= 14)).any()
    ok = np.arange(rows.size)
    bit = lambda c: np.uint64(1) << np.uint64(c)
    rows["present"] |= bit(23) | bit(25)
    rows["present"][8] &= ~bit(27)
    hit = set()
    plan = [(5, 2.0 ** 43), (6, -(2.0 ** 43)), (12, 8.8e12 + 0.123), (30, 1e300), (23, 2.0 ** 14), (25, -20000.25), (23, 1e30)]
    for k, (c, v) in enumerate(plan):
        i = int(ok[k])
        rows["col"][i, c] = v
        rows["present"][i] |= bit(c)
        hit.add(i)
    # two in one row count once; a float32 value beyond 2^14 in the MIXED column is inside float64's bound and is no fallback
    i = int(ok[0])
    rows["col"][i, 7] = 9e15
    rows["present"][i] |= bit(7)
    j = int(ok[7])
    rows["col"][j, 27] = 123456.0
    rows["present"][j] |= bit(27)
    return hit


def rows_from_golden(gold_dir, name):
    """a golden case's rows (tests/golden/<name>.rows.json: the reference's DetectResults as dicts) as adp_row records and read
    ids read_0000, ... as tests/test_host_cpu.py names them -> (rows, ids, primary).  The inverse of lib.rows_to_results on what
    the reference produces; the caller holds the Python writer's text of these rows against the golden's CSV text where it has one."""
    import json
    import os

    with open(os.path.join(gold_dir, name + ".rows.json")) as fh:
        g = json.load(fh)
    primary = g["primary_method"]
    names = [c.format(primary=primary) for c in lib.COLS]
    code_of = {v: k for k, v in lib.FAIL_REASONS.items() if v is not None}
    type_of = {v: k for k, v in lib.START_PEAK_TYPES.items()}
    rows = lib.empty_rows(len(g["rows"]))
    for i, d in enumerate(g["rows"]):
        r = rows[i]
        r["success"] = int(bool(d["success"]))
        fr = d["fail_reason"]
        if primary == "start_peak" and fr is not None and "+" in fr:
            fr = fr.split("+")[0]
        if fr in code_of:
            r["fail_code"] = code_of[fr]
        elif fr is not None:  # (code 7: the names of the failed MVS tests behind the text)
            assert fr.startswith(lib.FAIL_REASONS[7]), (name, i, fr)
            r["fail_code"] = 7
            r["mvs_fail_mask"] = sum(1 << lib._MVS_NAMES.index(w) for w in fr[len(lib.FAIL_REASONS[7]):].split())
        if 9 <= int(r["fail_code"]) <= 14:
            assert all(v is None for k, v in d.items() if k not in ("success", "fail_reason")), (name, i)
            continue
        present = 0
        for c, field in enumerate(names):
            v = d[field]
            if v is None or (c in lib._INT_COLS and v != v):  # (open_pore_float_column's NaN: the CSV text is the same either way)
                continue
            present |= 1 << c
            r["col"][c] = v
        r["present"] = present
        for q in ("llr", "cnn", "start_peak"):
            assert q == primary or (d[q + "_adapter_end"] is None and d[q + "_polya_end"] is None), (name, i)
        assert d["llr_adapter_end_adjust"] is None and d["llr_polya_end_adjust"] is None and d["llr_trace_early_stop_pos"] is None
        assert d["polya_truncated"] is None and d["mvs_llr_polya_end_adjust_ignored"] is False, (name, i)
        if d["mvs_llr_polya_end_to_early_stop"]:
            r["mvs_fail_mask"] |= 256
        r["start_peak_type"] = type_of[d["start_peak_open_pore_type"]]
        if d["polya_candidates"] is not None:
            r["n_cand"] = len(d["polya_candidates"])
            r["cand"][:len(d["polya_candidates"])] = d["polya_candidates"]
        if d["open_pores"] is not None:
            op = np.asarray(d["open_pores"], dtype=np.int64)
            r["n_open_pores"] = op.size
            r["open_pores"][:min(op.size, lib.MAX_OPEN_PORES)] = op[:lib.MAX_OPEN_PORES]
            if op.size > lib.MAX_OPEN_PORES:
                r["open_pores_more"] = lib.register_open_pores(op)
    return rows, ["read_%04d" % i for i in range(len(rows))], primary
