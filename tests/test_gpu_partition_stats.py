"""k_partition_stats (adapted_amd/csrc/block_stats.h) branch by branch: the reads of tests/partition_stats_cases.py through
Engine.validate_rows on boundaries the test chooses, every field of every row identical to the oracle (which
tests/test_partition_stats_cases_cpu.py holds to plain numpy), and the kernel's own tallies as evidence that each group of cases
took the fallback it was built for -- a wrong fallback would otherwise be silent on all the data the rest of the suite uses."""
import numpy as np
import pytest

import partition_stats_cases as P
from util import row_diffs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from adapted_amd import lib

    e = lib.Engine(P.make_spc(), len(P.CASES), P.M, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def want(oracle_mod):
    sig, lens, bounds = P.batch(P.CASES)
    rows = oracle_mod.detect_cnn_from_preds(sig, lens, bounds, P.make_spc())
    assert not any(w.get("_exception") for w in rows)
    return {c["name"]: {k: v for k, v in w.items() if not k.startswith("_")} for c, w in zip(P.CASES, rows)}


def _diffs(rows, cases, want):
    from adapted_amd import lib

    got = lib.rows_to_results(rows, "cnn")
    return [(c["name"], d) for c, g in zip(cases, got) for d in [row_diffs(g, want[c["name"]], float_rel=0.0)] if d]


@pytest.mark.parametrize("group", P.GROUPS)
def test_group_equals_oracle_and_takes_its_branches(eng, want, group):
    """one call per group of cases: rows identical to the oracle's, no tolerance, and the tallies of the large segments
    (poly(A) / RNA, >= 8192 samples, no NaN) rise as the cases' tags say: slot 0 by their number, slots 2 (fallback_med),
    3 (not predicted), 4 (bracket overflow), g_dbg[20] (one-value bucket) and g_dbg[21] (dense bucket) by at least the cases
    built for them; predicted-but-unproven is slot 0 - 1 - 3 - 4; where every segment is a control, slot 1 equals slot 0."""
    cases = P.by_group(group)
    sig, lens, bounds = P.batch(cases)
    c0 = eng.debug_counters(22).astype(np.int64)
    rows = eng.validate_rows(sig, lens, len(cases), bounds)
    d = eng.debug_counters(22).astype(np.int64) - c0
    exp = P.expected_tallies(cases)
    print("tallies %-14s reads %2d  slots 0-4 %s  g_dbg[20] %d  g_dbg[21] %d  expected %s"
          % (group, len(cases), list(d[:5]), d[20], d[21], exp))
    bad = _diffs(rows, cases, want)
    assert not bad, bad[:5]
    assert d[0] == exp["segments"], (d[:5], exp)
    assert d[2] >= exp["fallback_med"] and d[3] >= exp["not_predicted"] and d[4] >= exp["bracket_overflow"], (d[:5], exp)
    assert d[0] - d[1] - d[3] - d[4] >= exp["unproven"], (d[:5], exp)
    assert d[1] == d[0] if exp["proven"] == exp["segments"] else d[1] >= exp["proven"], (d[:5], exp)
    assert d[20] >= exp["one_value_bucket"] and d[21] >= exp["dense_bucket"], (d[20], d[21], exp)
    if group == "control":
        assert d[0] > 0 and not d[2:5].any() and d[20] == 0 and d[21] == 0, d
    if group == "unproven":
        assert d[0] - d[1] - d[3] - d[4] > 0, d[:5]


def test_all_cases_in_one_call_twice_and_permuted(eng, want):
    """all reads in one call equal the oracle; a second call on the same engine gives the same bytes (no LDS or handle state
    leaks between branches); the reads in a permuted order give the permuted rows (neither the order of the workgroups nor
    what a workgroup's predecessor left behind matters)"""
    cases = P.CASES
    n = len(cases)
    sig, lens, bounds = P.batch(cases)
    rows = eng.validate_rows(sig, lens, n, bounds)
    bad = _diffs(rows, cases, want)
    assert not bad, bad[:5]
    again = eng.validate_rows(sig, lens, n, bounds)
    assert again.tobytes() == rows.tobytes()
    for perm in (np.arange(n)[::-1], np.random.default_rng(5).permutation(n)):
        rows_p = eng.validate_rows(np.ascontiguousarray(sig[perm]), lens[perm], n, bounds[perm])
        differ = [cases[i]["name"] for j, i in enumerate(perm) if rows_p[j].tobytes() != rows[i].tobytes()]
        assert not differ, differ
