"""The cases of tests/partition_stats_cases.py on the CPU: the oracle's twelve partition statistics equal plain numpy on the
float32 slices, no case is an exception row, and every case's data take the branch of k_partition_stats they were built for
(by the numpy restatement of the kernel's branch arithmetic).  This pins the checker and the data; tests/test_gpu_partition_stats.py
holds the device to both."""
import math

import numpy as np
import pytest

import partition_stats_cases as P

NAMES = [c["name"] for c in P.CASES]


@pytest.fixture(scope="module")
def oracle_rows(oracle_mod):
    sig, lens, bounds = P.batch(P.CASES)
    return dict(zip(NAMES, oracle_mod.detect_cnn_from_preds(sig, lens, bounds, P.make_spc())))


def test_the_cases_are_the_ones_the_kernel_needs():
    """every distribution, size and edge is there, one read each, and no read outgrows the row"""
    kinds = set(P.DIST_TAGS)
    assert kinds == set(c["rna"][0] for c in P.CASES if c["rna"][1] in (20000, 20001)) and len(kinds) == 18
    assert sorted(c["rna"][1] for c in P.CASES if c["name"].startswith("rna_len")) == [3073, 8191, 8192, 8193, 16384, 16385, 24703, 24705]
    assert sorted(c["polya"][1] for c in P.CASES if c["name"].startswith("polya_len")) == [1, 2, 7, 8, 9, 127, 128, 129, 3071, 3072, 3073]
    assert sorted(c["adapter"][1] for c in P.CASES if c["name"].startswith("adapter_len")) == [7423, 7424, 7425, 8193]
    starts = set((P.build(c)[2] % 4, P.build(c)[3] % 4) for c in P.CASES if c["name"].startswith("start_mod4"))
    assert len(starts) == 16
    for kind in P.REPEATED:
        assert sorted(c["polya"][1] for c in P.CASES if c["polya"][0] == kind) == [3000, 3073]
        assert [c["adapter"][1] for c in P.CASES if c["adapter"][0] == kind] == [9000]
    assert set(c["group"] for c in P.CASES) == set(P.GROUPS)
    assert len(set(c["seed"] for c in P.CASES)) == len(P.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_numpy(oracle_rows, name):
    case = next(c for c in P.CASES if c["name"] == name)
    row = oracle_rows[name]
    assert not row.get("_exception"), row
    _, S, a_e, p_e = P.build(case)
    assert (row["adapter_start"], row["adapter_end"], row["polya_end"], row["rna_preloaded_start"]) == (0, a_e, p_e, p_e)
    assert (row["adapter_len"], row["polya_len"], row["rna_preloaded_len"], row["preloaded"]) == (a_e, p_e - a_e, S - p_e, S)
    want = P.numpy_stats(case)
    bad = [(k, row[k], want[k]) for k in P.FIELDS if not (row[k] == want[k] or (math.isnan(row[k]) and math.isnan(want[k])))]
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_case_takes_its_branch(name):
    """the partition under test carries exactly the tags it was built for, the other large partition the control's.  (rk0_even
    is the one tag that plain data meet by chance -- one even count in ten: it is demanded where a case names it and allowed elsewhere)"""
    case = next(c for c in P.CASES if c["name"] == name)
    which = P.under_test(case)
    for part, x in P.segments(case).items():
        if part == "adapter":  # (k_validate's wave_median supplies its median and MAD: none of the branches)
            continue
        got = P.tags(x)
        want = case["expect"] if part == which else (P.CONTROL if x.size > P.BS_BINS else frozenset(["lds"]))
        assert want <= got and got - want <= {"rk0_even"}, (part, sorted(got), sorted(want))


def test_every_branch_has_a_case():
    """each predicate holds for a tallied segment (>= 8192 samples) of some case; the one-value and the several-value
    bucket, the C/D miss and both C/D overflows among them"""
    seen = set()
    for c in P.CASES:
        if c["expect"] and c[P.under_test(c)][1] >= P.TALLY_MIN:
            seen |= c["expect"]
    assert seen >= set(P.PREDICATES) | {"nan", "nan_mean"}, sorted(set(P.PREDICATES) - seen)


def test_groups_name_every_tally():
    """the cases' tags reach every tally the kernel keeps, so that no assertion of the GPU test on them is vacuous"""
    total = P.expected_tallies(P.CASES)
    assert all(v > 0 for v in total.values()), total
    control = P.expected_tallies(P.by_group("control"))
    assert control["segments"] == control["proven"] > 0
    assert P.expected_tallies(P.by_group("unproven"))["unproven"] > 0


def test_key_order_and_window_restatement():
    """the restated key is order preserving over signs, zeros, denormals and infinities, and key2f inverts it"""
    x = np.array([-np.inf, -3e38, -100.0, -1e-30, -1e-45, 0.0, 1e-45, 1e-30, 77.25, 100.0, 3e38, np.inf], dtype=np.float32)
    k = P.f2key(x)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert P.key2f(k).tobytes() == x.tobytes()
    assert int(P.f2key(np.float32(77.25))) & 0xFFF == 0  # (the constant case sits on a bucket's first key)
