"""The LLR second opinion of the CNN operator inside adp_detect_cnn (ADP_CNN_SECOND_LLR; adapted_amd/csrc/cnn_second_opinion.h):
a read the CNN path fails gets the row combined_detect_llr2 returns for it on its minibatch, where that row passes.

Yardsticks: for the CNN side the same engine's call WITHOUT the flag on the same batch, byte for byte (predictions may differ
from the golden ones inside exact ties, so golden CNN rows are not used); for the LLR side ``oracle.detect_llr`` per minibatch
with the LLR-switched copy of the configuration, at the tolerance of test_gpu_llr.py (integers exact, floats 1e-5).  Every
precondition is asserted, so that a batch that stops exercising a branch fails loudly."""
import copy

import numpy as np
import pytest

from test_gpu_cnn_fallback import _case, _engine
from util import row_diffs

pytestmark = pytest.mark.gpu

FLOAT_REL = 1e-5  # test_gpu_llr.py::test_llr_rows_vs_golden_and_oracle
EMPTY_TRACE = "attempt to get argmin of an empty sequence"


def _llr_spc(spc):
    s = copy.deepcopy(spc)
    s.llr_boundaries.llr_detect, s.cnn_boundaries.cnn_detect = True, False
    s.update_primary_method()
    s.update_sig_preload_size()
    assert s.primary_method == "llr" and s.sig_preload_size == spc.sig_preload_size
    return s


_ORACLE = {}


def _oracle_llr(oracle_mod, key, sig, lens, spc, mb):
    """oracle.detect_llr minibatch by minibatch -> (per-read dict, or None where the minibatch raised; the messages of the
    minibatches that raised, by minibatch).  key: cached under it (the inputs of one key never change)"""
    if key is not None and (key, mb) in _ORACLE:
        return _ORACLE[(key, mb)]
    s = _llr_spc(spc)
    n = sig.shape[0]
    want, raised = [], {}
    for a in range(0, n, mb):
        b = min(n, a + mb)
        try:
            want += oracle_mod.detect_llr(sig[a:b], lens[a:b], s)
        except ValueError as e:
            want += [None] * (b - a)
            raised[a // mb] = str(e)
    if key is not None:
        _ORACLE[(key, mb)] = (want, raised)
    return want, raised


def _per_row(rows):
    """-> (bytes of every row with the registry token blanked, {read: overflow open-pore list})"""
    from adapted_amd import lib

    lists = {int(i): lib._OPEN_PORES_MORE[int(rows[i]["open_pores_more"])].tolist() for i in np.flatnonzero(rows["n_open_pores"] > lib.MAX_OPEN_PORES)}
    r = rows.copy()
    r["open_pores_more"] = 0
    return [r[i].tobytes() for i in range(r.size)], lists


def _both(eng, sig, lens, mb):
    """the call without and with the flag on one engine -> (plain rows, second-opinion rows, counts)"""
    n = sig.shape[0]
    plain, b0 = eng.detect_cnn_rows(sig, lens, n, mb, fallback=True)
    assert eng.debug_cnn_second_opinion() == (0, 0, 0, 0)
    got, b1 = eng.detect_cnn_rows(sig, lens, n, mb, fallback=True, second_opinion=True)
    assert np.array_equal(b0, b1), "bounds_out stays what cnn_detect returned"
    return plain, got, eng.debug_cnn_second_opinion()


def _check(plain, got, counts, want, raised, mb, what):
    """every read against its yardstick -> the reads of the three kinds (pass, rescued, fail both ways)"""
    from adapted_amd import lib

    n = plain.size
    assert (plain["reserved_"] == 0).all()
    pb, pl = _per_row(plain)
    gb, gl = _per_row(got)
    kinds = {"pass": [], "rescued": [], "both": []}
    still = 0
    for i in range(n):
        if plain[i]["success"] == 1:
            kinds["pass"].append(i)
        elif want[i] is not None and want[i]["success"]:
            kinds["rescued"].append(i)
        else:
            kinds["both"].append(i)
            still += want[i] is not None
    print("%s: pass / rescued / fail both ways %d / %d / %d, counts %s, minibatches without %s" % (
        what, len(kinds["pass"]), len(kinds["rescued"]), len(kinds["both"]), counts, raised))
    print("%s: rescued %s, fail both ways %s" % (what, kinds["rescued"], kinds["both"]))
    for i in kinds["pass"] + kinds["both"]:
        assert gb[i] == pb[i] and gl.get(i) == pl.get(i), (what, "read %d must keep the plain call's row" % i, int(got[i]["success"]), int(got[i]["reserved_"]))
        assert got[i]["reserved_"] == 0
    for i in kinds["rescued"]:
        assert got[i]["reserved_"] == 1 and got[i]["success"] == 1, (what, i, int(got[i]["reserved_"]), int(got[i]["success"]), int(got[i]["fail_code"]))
        res = lib.rows_to_results(got[i:i + 1], "cnn")[0]
        pub = {k: v for k, v in want[i].items() if not k.startswith("_")}
        d = row_diffs(res, pub, float_rel=FLOAT_REL)
        assert not d, (what, i, d[:6])
        assert res.llr_detect_log == "" and res.cnn_adapter_end is None and res.cnn_polya_end is None
        assert len(res.open_pores) == want[i]["_n_open_pores"]
    no_opinion = sum(1 for k in raised if any(plain[i]["success"] == 0 for i in range(k * mb, min(n, (k + 1) * mb))))
    implied = (len(kinds["rescued"]) + len(kinds["both"]), len(kinds["rescued"]), still, no_opinion)
    assert counts == implied, (what, counts, implied)
    return kinds


@pytest.mark.parametrize("name", ["rna004_cnn_default", "rna004_cnn_200k", "rna004_cnn_k3", "rna004_cnn_nan_holes"])
def test_failed_reads_get_the_llr_row_where_it_passes(name, oracle_mod):
    """(on the CPU, with golden CNN rows, the kinds split 11 / 11 / 26, 4 / 3 / 5, 5 / 8 / 19 and 2 / 10 / 12 rescued / both / pass)"""
    spc, sig, lens, _ = _case(name)
    n, m = sig.shape
    eng = _engine(spc, n, m)
    plain, got, counts = _both(eng, sig, lens, n)
    want, raised = _oracle_llr(oracle_mod, name, sig, lens, spc, n)
    assert not raised
    kinds = _check(plain, got, counts, want, raised, n, name)
    assert all(len(v) >= 1 for v in kinds.values()), ("precondition: reads of all three kinds", {k: len(v) for k, v in kinds.items()})
    if name == "rna004_cnn_default":
        assert any(9 <= plain[i]["fail_code"] <= 14 for i in kinds["both"]), "precondition: an exception row among the reads that fail both ways"
    eng.close()


@pytest.mark.parametrize("minibatch", [16, 20])
def test_minibatches_and_lanes(minibatch, oracle_mod, monkeypatch):
    """the second opinion is normalised over the read's minibatch: read 15 passes the LLR path in a minibatch of 16 and fails it
    in the batch of 48 (on the CPU the per-chunk rescues at 16 are {5,12,14,15}, {17,19,22,24}, {33,38,46,47})"""
    name = "rna004_cnn_default"
    spc, sig, lens, _ = _case(name)
    n, m = sig.shape
    want, raised = _oracle_llr(oracle_mod, name, sig, lens, spc, minibatch)
    assert not raised
    if minibatch == 16:
        whole, _ = _oracle_llr(oracle_mod, name, sig, lens, spc, n)
        assert want[15]["success"] and not whole[15]["success"], "precondition: read 15 passes in its minibatch only"
    out = {}
    for lanes in (False, True):
        monkeypatch.delenv("ADP_CNN_GROUPS", raising=False)
        monkeypatch.delenv("ADP_CNN_LANES", raising=False)
        if lanes:
            monkeypatch.setenv("ADP_CNN_GROUPS", "3")
            monkeypatch.setenv("ADP_CNN_LANES", "2")
        eng = _engine(spc, n, m)
        plain, got, counts = _both(eng, sig, lens, minibatch)
        kinds = _check(plain, got, counts, want, raised, minibatch, "minibatch %d, lanes %s" % (minibatch, lanes))
        # preconditions, from the two yardsticks alone.  The CNN path's own outcome depends on the minibatch (its find_peaks runs
        # over the flattened minibatch), so which reads are left to rescue differs between 16 and 20: at 16 every minibatch
        # holds a rescue; at 20 the first two do and the CNN path passes every read of the last, partial one [40, 48), which
        # the second opinion therefore has to skip
        chunks = list(range(0, n, minibatch))
        with_rescue = [a for a in chunks if any(a <= i < a + minibatch for i in kinds["rescued"])]
        with_selected = [a for a in chunks if any(a <= i < a + minibatch for i in kinds["rescued"] + kinds["both"])]
        if minibatch == 16:
            assert with_rescue == chunks, ("precondition: a rescue in every minibatch", kinds["rescued"])
            assert 15 in kinds["rescued"], ("precondition: the CNN path fails read 15", kinds)
        else:
            assert len(with_rescue) >= 2, ("precondition: rescues in more than one minibatch", kinds["rescued"])
            assert with_selected != chunks, ("precondition: a minibatch without a failed read", kinds)
        out[lanes] = (_per_row(got), counts)
        eng.close()
    assert out[True] == out[False], "lanes against one stream"


def test_a_minibatch_the_llr_primary_drops_keeps_its_rows(oracle_mod):
    name = "rna004_cnn_default"
    spc, sig0, lens0, _ = _case(name)
    n, m = sig0.shape
    mb, cut = 16, 21
    sig, lens = sig0.copy(), lens0.copy()
    sig[cut, 1004:] = np.nan
    lens[cut] = 1004
    want, raised = _oracle_llr(oracle_mod, None, sig, lens, spc, mb)
    assert raised == {1: EMPTY_TRACE}, raised
    eng = _engine(spc, n, m)
    plain, got, counts = _both(eng, sig, lens, mb)
    assert (plain[mb:2 * mb]["success"] == 0).any(), "precondition: the dropped minibatch holds a failed read"
    kinds = _check(plain, got, counts, want, raised, mb, "dropped middle minibatch")
    assert _per_row(got)[0][mb:2 * mb] == _per_row(plain)[0][mb:2 * mb]
    assert any(i < mb for i in kinds["rescued"]) and any(i >= 2 * mb for i in kinds["rescued"]), ("the outer minibatches get their second opinions", kinds["rescued"])
    assert counts[3] == 1
    eng.close()


# reads of rna004_cnn_default, on the LLR side in every pattern: 12 and 5 pass, 0 passes, 6 fails ("No adapter detected").  On the
# CNN side 0 passes and 6 fails in every pattern.  Read 12 fails the CNN path in the batch of 48 only through its neighbours
# (cnn_predict's candidates are grouped over the flattened minibatch, and a read without a candidate shifts the groups of the
# reads behind it): alone or among its own copies the CNN path passes it, so in these batches it is never selected.  Read 5 fails
# the CNN path on its own ("MVS polya check failed: mean var") and the LLR path passes it: with it in read 12's place the
# patterns do select 1, 64, 65, every other, the last and no read.  Both sets run.  pattern -> reads (R: read 12 or read 5)
_PATTERNS = {
    "one_selected": ["R"],
    "64_all_selected": ["R"] * 64,
    "65_all_selected": ["R"] * 65,
    "130_alternating": ["R", 0, 6, 0] * 32 + ["R", 0],
    "130_last_selected": [0] * 129 + ["R"],
    "130_none_selected": [0] * 130,
}
_CNN_FAILS_IT = {0: False, 6: True, 12: False, 5: True}  # in these batches; asserted against the plain call


@pytest.mark.parametrize("pattern", list(_PATTERNS))
@pytest.mark.parametrize("R", [12, 5])
def test_compaction_edges(R, pattern, oracle_mod):
    spc, sig, lens, _ = _case("rna004_cnn_default")
    pick = [R if r == "R" else r for r in _PATTERNS[pattern]]
    bs, bl = np.ascontiguousarray(sig[pick]), np.ascontiguousarray(lens[pick])
    n = len(pick)
    want, raised = _oracle_llr(oracle_mod, None, bs, bl, spc, n)
    assert not raised
    for i, r in enumerate(pick):  # precondition, LLR side: pass / pass / "No adapter detected"
        assert want[i]["success"] == (r != 6) and (r != 6 or want[i]["fail_reason"] == "No adapter detected (primary)"), (i, r, want[i]["success"], want[i]["fail_reason"])
    eng = _engine(spc, n, sig.shape[1])
    plain, got, counts = _both(eng, bs, bl, n)
    assert [int(s) for s in plain["success"]] == [int(not _CNN_FAILS_IT[r]) for r in pick], "precondition, CNN side"
    kinds = _check(plain, got, counts, want, raised, n, "read %d, %s" % (R, pattern))
    rescued = [i for i, r in enumerate(pick) if r == 5]
    assert kinds["rescued"] == rescued
    assert counts == (len(rescued) + sum(r == 6 for r in pick), len(rescued), sum(r == 6 for r in pick), 0)
    eng.close()


def test_compaction_carries_its_total_across_a_1024_read_step(oracle_mod):
    """k_cnn_so_select walks the rows 1024 at a time and carries the reads taken so far from step to step: 1090 = 1024 + 64 + 2 copies of
    the reads of _PATTERNS in one minibatch (5: selected and rescued, 6: selected and failing both ways, 0: never selected).  Reads
    1023 and 1024 are selected (the step's border), the last read is, and the second wave of the first step (reads 64..127) holds
    none; of the second step's waves only two hold reads at all."""
    spc, sig, lens, _ = _case("rna004_cnn_default")
    n = 1090
    pick = [(5, 0, 6, 0)[i % 4] for i in range(n)]
    pick[64:128] = [0] * 64
    pick[1023] = 6
    pick[n - 1] = 5
    selected = [_CNN_FAILS_IT[r] for r in pick]
    assert selected[1023] and selected[1024] and selected[n - 1] and not any(selected[64:128])
    assert sum(selected) == 515 and sum(selected[:1024]) == 481
    bs, bl = np.ascontiguousarray(sig[pick]), np.ascontiguousarray(lens[pick])
    want, raised = _oracle_llr(oracle_mod, None, bs, bl, spc, n)
    assert not raised
    for i, r in enumerate(pick):  # precondition, LLR side (as in test_compaction_edges)
        assert want[i]["success"] == (r != 6), (i, r, want[i]["fail_reason"])
    eng = _engine(spc, n, sig.shape[1])
    plain, got, counts = _both(eng, bs, bl, n)
    assert [int(s) for s in plain["success"]] == [int(not s) for s in selected], "precondition, CNN side"
    kinds = _check(plain, got, counts, want, raised, n, "1090 reads")
    rescued = [i for i, r in enumerate(pick) if r == 5]
    assert kinds["rescued"] == rescued
    assert counts == (sum(selected), len(rescued), sum(r == 6 for r in pick), 0)
    eng.close()


def test_resident_input_and_device_rows_give_the_same_bytes(oracle_mod):
    import torch

    from adapted_amd import lib
    from adapted_amd.detect import cnn

    name = "rna004_cnn_default"
    spc, sig, lens, _ = _case(name)
    n, m = sig.shape
    mb = 16
    want, raised = _oracle_llr(oracle_mod, name, sig, lens, spc, mb)
    eng = _engine(spc, n, m)
    plain, staged, counts = _both(eng, sig, lens, mb)
    kinds = _check(plain, staged, counts, want, raised, mb, "staged")
    assert kinds["rescued"]
    dsig = torch.from_numpy(np.ascontiguousarray(sig)).cuda()
    dlen = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    res = cnn.detect_rows_device_second_opinion(eng, dsig.data_ptr(), dlen.data_ptr(), n, lens, None, spc, mb)
    assert eng.debug_cnn_second_opinion() == counts
    assert _per_row(res) == _per_row(staged), "resident against staged"
    drows = eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
    none, _ = eng.detect_cnn_rows(dsig.data_ptr(), dlen.data_ptr(), n, mb, device_ptrs=True, rows_dev=drows, want_bounds=False, fallback=True,
                                  second_opinion=True)
    assert none is None and eng.debug_cnn_second_opinion() == counts
    back = np.zeros(n, dtype=lib.ROW_DTYPE)
    eng.d2h(back, drows)
    eng.dev_free(drows)
    assert _per_row(eng.attach_open_pores(back)) == _per_row(staged), "rows on the device"
    # the flag leaves nothing behind: the plain call on the same engine afterwards
    again = cnn.detect_rows_device(eng, dsig.data_ptr(), dlen.data_ptr(), n, lens, None, spc, mb)
    assert eng.debug_cnn_second_opinion() == (0, 0, 0, 0)
    assert _per_row(again) == _per_row(plain)
    # the operator: always a list, the rescued reads named by the LLR path's columns
    out = cnn.combined_detect_cnn_llr(sig[:mb], lens[:mb], None, spc)
    assert isinstance(out, list) and len(out) == mb
    for i in (k for k in kinds["rescued"] if k < mb):
        assert out[i].success and out[i].llr_adapter_end == want[i]["llr_adapter_end"] and out[i].cnn_adapter_end is None
    assert isinstance(cnn.combined_detect_cnn_llr(sig[:1], lens[:1], None, spc), list)
    eng.close()


def _open_pore_read(read=12, stop=2800):
    """a read of rna004_cnn_default with 250-pA samples in its adapter, 10 apart from 300 up to stop -> (spc, [1, m] signal, [1] length)"""
    spc, sig, lens, _ = _case("rna004_cnn_default")
    s = np.array(sig[read:read + 1])
    s[0, 300:stop:10] = 250.0
    return spc, s, np.ascontiguousarray(lens[read:read + 1])


# case -> (the batch's reads, position of the read with the open pores, its last pore's bound, open pores, CNN path fails it).
# Read 12 alone passes the CNN path (see _PATTERNS), so its row stays the CNN's, list and all; among reads 7..15, in its own
# place, the CNN path fails it ("MVS polya check failed: mean var") and the LLR row with the 249 open pores replaces it.  Read 5
# fails the CNN path alone; the LLR path passes it with pores up to 2300 only (beyond: "Open pore too close to boundary")
_PORE_CASES = {
    "read12_alone": ([12], 0, 2800, 249, False),
    "read12_among_8_others": (list(range(7, 16)), 5, 2800, 249, True),
    "read5_alone": ([5], 0, 2300, 199, True),
}


@pytest.mark.parametrize("case", list(_PORE_CASES))
def test_open_pore_list_of_a_replaced_row_is_whole(case, oracle_mod):
    pick, at, stop, pores, cnn_fails = _PORE_CASES[case]
    spc, s, _ = _open_pore_read(pick[at], stop)
    _, sig, lens, _ = _case("rna004_cnn_default")
    bs, bl = np.ascontiguousarray(sig[pick]), np.ascontiguousarray(lens[pick])
    bs[at] = s[0]
    n = bs.shape[0]
    want, raised = _oracle_llr(oracle_mod, None, bs, bl, spc, n)
    assert not raised and want[at]["success"] and want[at]["_n_open_pores"] == pores, "precondition: the LLR row passes with all the open pores"
    eng = _engine(spc, n, bs.shape[1])
    plain, got, counts = _both(eng, bs, bl, n)
    assert plain[at]["success"] == (not cnn_fails), "precondition: what the CNN path makes of the read"
    kinds = _check(plain, got, counts, want, raised, n, case)
    assert at in kinds["rescued" if cnn_fails else "pass"] and got[at]["n_open_pores"] == pores
    assert _per_row(got)[1][at] == want[at]["open_pores"]
    eng.close()


@pytest.mark.parametrize("read,stop,pores,n", [(12, 2800, 249, 140), (5, 2300, 199, 190)])
def test_arena_overflow_in_the_second_opinion_repeats_the_call(read, stop, pores, n, oracle_mod):
    """copies of one read on a fresh engine (its arena holds 65 536 entries).  140 copies of read 12: the CNN path passes them all
    (see _PATTERNS), nothing is selected, the 140 lists fit.  190 copies of read 5: the first rows and the second opinion's rows
    together need 2 * 190 * 199 entries, the call repeats on a larger arena, and no list is cut"""
    spc, s, l = _open_pore_read(read, stop)
    bs, bl = np.ascontiguousarray(np.repeat(s, n, axis=0)), np.ascontiguousarray(np.repeat(l, n))
    want, raised = _oracle_llr(oracle_mod, None, bs, bl, spc, n)
    assert not raised and all(w["success"] and w["_n_open_pores"] == pores for w in want)
    eng = _engine(spc, n, s.shape[1])  # (fresh: its arena is the initial one)
    got, _ = eng.detect_cnn_rows(bs, bl, n, n, fallback=True, second_opinion=True)
    counts = eng.debug_cnn_second_opinion()
    used = np.zeros(1, dtype=np.uint64)
    eng._check(eng.lib.adp_open_pores_arena(eng._h, None, 0, used))
    print("read %d: arena entries in use: %d, counts %s" % (read, int(used[0]), counts))
    plain, _ = eng.detect_cnn_rows(bs, bl, n, n, fallback=True)
    selected = read == 5
    assert (plain["success"] == (not selected)).all(), "precondition: what the CNN path makes of the copies"
    if selected:
        assert int(used[0]) > 65536, ("precondition: more than the initial arena in use", int(used[0]))
    assert counts == ((n, n, 0, 0) if selected else (0, 0, 0, 0))
    assert (got["reserved_"] == int(selected)).all() and (got["success"] == 1).all() and (got["n_open_pores"] == pores).all()
    lists = _per_row(got)[1]
    assert len(lists) == n and all(v == want[0]["open_pores"] for v in lists.values())
    eng.close()
