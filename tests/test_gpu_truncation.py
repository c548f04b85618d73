"""ADP_FLAG_TRUNCATED on the GPU (adapted_amd/csrc/polya_truncated.h): every row of a flagged call against the rule restated
from the checkers (tests/truncation_restated.py: first rows from the CPU oracle, T1 from tests/mvs_module_restated.check, T2 from
oracle.detect_cnn_from_preds on the one read), every field without tolerance, ``polya_truncated`` and the marks in
``reserved_`` included.  Inputs: tests/truncation_cases.py; tests/test_truncation_cpu.py asserts that they hold every outcome."""
import numpy as np
import pytest

import truncation_cases as tc
import truncation_restated as tr
from util import row_diffs

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -4


def _canon(rows):
    """(bytes of every row with the registry token blanked, {read: overflow open-pore list})"""
    from adapted_amd import lib

    lists = {int(i): lib._OPEN_PORES_MORE[int(rows[i]["open_pores_more"])].tolist() for i in np.flatnonzero(rows["n_open_pores"] > lib.MAX_OPEN_PORES)}
    r = rows.copy()
    r["open_pores_more"] = 0
    return [r[i].tobytes() for i in range(r.size)], lists


def _compare(rows, exp, primary, what):
    from adapted_amd import lib

    res = lib.rows_to_results(rows, primary)
    bad = []
    for i, (g, e) in enumerate(zip(res, exp)):
        d = row_diffs(g, tr.public(e))
        if g.polya_truncated is not e["polya_truncated"]:
            d.append(("polya_truncated", g.polya_truncated, e["polya_truncated"]))
        if int(rows[i]["reserved_"]) != e["_reserved"]:
            d.append(("reserved_", int(rows[i]["reserved_"]), e["_reserved"]))
        if d:
            bad.append((i, d[:6]))
    assert not bad, (what, bad[:6])


def _llr_expected(oracle_mod, m_trace, n, mb, with_start_peak=False):
    spc = tc.spc_of("llr", m_trace)
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, n)
    first = tr.llr_first_rows(oracle_mod, sig, lens, spc, mb, with_start_peak, key=("gpu", m, n))
    exp, counts, kinds = tr.look(oracle_mod, sig, lens, first, spc, "llr")
    return spc, sig, lens, exp, counts, kinds


@pytest.mark.parametrize("with_start_peak", [False, True])
def test_llr_rows_equal_the_restated_rule(oracle_mod, with_start_peak):
    """two minibatches of 24, host and device inputs / outputs; flag off: today's rows; flag on: unflagged reads keep them apart from bit 2"""
    import torch

    from adapted_amd import lib

    spc, sig, lens, exp, counts, kinds = _llr_expected(oracle_mod, None, 48, 24, with_start_peak)
    n, m = sig.shape
    assert counts[2] >= 3 and counts[1] - counts[2] >= 3 and counts[0] - counts[1] >= 3, counts
    if with_start_peak:
        assert any(exp[r]["start_peak_idx"] is not None for r in range(n) if kinds[r] == "flagged"), "precondition: a flagged read with a start peak"
    eng = lib.Engine(spc, n, m, device=0)
    plain, mbs0 = eng.detect_llr_rows(sig, lens, n, 24, with_start_peak=with_start_peak)
    assert eng.debug_truncated() == (0, 0, 0) and (plain["reserved_"] == 0).all()
    _compare(plain, _plain_expected(oracle_mod, spc, sig, lens, 24, with_start_peak), "llr", "flag off")
    got, mbs = eng.detect_llr_rows(sig, lens, n, 24, with_start_peak=with_start_peak, flag_truncated=True)
    assert eng.debug_truncated() == counts, (eng.debug_truncated(), counts)
    assert (mbs == mbs0).all() and (mbs == lib.MB_OK).all()
    _compare(got, exp, "llr", "flag on")
    pb, gb = _canon(plain), _canon(got)
    for r in range(n):
        if kinds[r] != "flagged":
            unmarked = got[r:r + 1].copy()
            unmarked["reserved_"] &= ~lib.ROW_TRUNC_LOOKED
            assert _canon(unmarked)[0][0] == pb[0][r] and gb[1].get(r) == pb[1].get(r), "read %d keeps its row apart from bit 2" % r
    # device inputs, host rows; device inputs, device rows
    dsig = torch.from_numpy(np.array(sig)).cuda()
    dlen = torch.from_numpy(np.array(lens)).cuda()
    torch.cuda.synchronize()
    res, _ = eng.detect_llr_rows(dsig.data_ptr(), dlen.data_ptr(), n, 24, with_start_peak=with_start_peak, device_ptrs=True, flag_truncated=True)
    assert eng.debug_truncated() == counts and _canon(res) == gb, "resident input"
    drows = eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
    none, _ = eng.detect_llr_rows(dsig.data_ptr(), dlen.data_ptr(), n, 24, with_start_peak=with_start_peak, device_ptrs=True, rows_dev=drows,
                                  flag_truncated=True)
    back = np.zeros(n, dtype=lib.ROW_DTYPE)
    eng.d2h(back, drows)
    eng.dev_free(drows)
    assert none is None and eng.debug_truncated() == counts and _canon(eng.attach_open_pores(back)) == gb, "rows on the device"
    # the flag leaves nothing behind
    again, _ = eng.detect_llr_rows(sig, lens, n, 24, with_start_peak=with_start_peak)
    assert _canon(again) == pb and eng.debug_truncated() == (0, 0, 0)
    eng.close()


def _plain_expected(oracle_mod, spc, sig, lens, mb, with_start_peak):
    first = tr.llr_first_rows(oracle_mod, sig, lens, spc, mb, with_start_peak, key=("gpu", sig.shape[1], sig.shape[0]))
    return [dict(r, polya_truncated=None, _reserved=0) for r in first]


def test_groups_and_lanes_give_the_same_rows(oracle_mod, monkeypatch):
    """four minibatches of 12: one group against ADP_GROUPS=2 over two lanes"""
    from adapted_amd import lib

    spc, sig, lens, exp, counts, kinds = _llr_expected(oracle_mod, None, 48, 12)
    n, m = sig.shape
    assert counts[2] >= 3
    out = {}
    for groups in (None, "2"):
        monkeypatch.delenv("ADP_GROUPS", raising=False)
        monkeypatch.delenv("ADP_LANES", raising=False)
        if groups:
            monkeypatch.setenv("ADP_GROUPS", groups)
            monkeypatch.setenv("ADP_LANES", "2")
        eng = lib.Engine(spc, n, m, device=0)
        got, _ = eng.detect_llr_rows(sig, lens, n, 12, flag_truncated=True)
        assert eng.debug_truncated() == counts
        _compare(got, exp, "llr", "ADP_GROUPS=%s" % groups)
        out[groups] = _canon(got)
        eng.close()
    assert out[None] == out["2"]


def test_selection_carries_its_total_across_a_1024_read_step(oracle_mod):
    """k_pt_select walks the verdicts 1024 at a time and carries the reads taken so far from step to step: 1090 = 1024 + 64 + 2 reads in
    one minibatch, copies of a flagged, a T1-failing and a T2-failing read of the file's batch and of an ineligible one (full_len == m).
    Reads 1023 and 1024 pass T1 (the step's border), the last read does, and the second wave of the first step (reads 64..127) holds
    none that does; of the second step's waves only two hold reads at all.  Kinds and counts come from the restated rule on this batch."""
    from adapted_amd import lib

    spc = tc.spc_of("llr")
    m = spc.sig_preload_size
    long_sig, long_len = tc.batch(m, 48)
    short_sig, short_len = tc.batch(m, 24, full_len=m)
    src = [(long_sig[3], long_len[3]), (long_sig[0], long_len[0]), (short_sig[3], short_len[3]), (long_sig[1], long_len[1])]
    n = 1090
    pick = [i % 4 for i in range(n)]
    pick[64:128] = [1, 2] * 32
    pick[n - 1] = 0
    sig = np.stack([src[p][0] for p in pick])
    lens = np.array([src[p][1] for p in pick], dtype=np.int32)
    first = tr.llr_first_rows(oracle_mod, sig, lens, spc, n)
    exp, counts, kinds = tr.look(oracle_mod, sig, lens, first, spc, "llr")
    passed = [k in ("t2_failed", "flagged") for k in kinds]
    print("1090 reads: counts %s, kinds %s" % (counts, {k: kinds.count(k) for k in set(kinds)}))
    assert passed[1023] and passed[1024] and passed[n - 1] and not any(passed[64:128]), "precondition: the step's border, the last read, an empty wave"
    assert set(kinds) == {"ineligible", "t1_failed", "t2_failed", "flagged"}, "precondition: reads of every outcome"
    assert counts[1] == sum(passed) and sum(passed[:1024]) >= 3 and sum(passed[1024:]) >= 3
    eng = lib.Engine(spc, n, m, device=0)
    got, _ = eng.detect_llr_rows(sig, lens, n, n, flag_truncated=True)
    assert eng.debug_truncated() == counts, (eng.debug_truncated(), counts)
    _compare(got, exp, "llr", "1090 reads")
    eng.close()


@pytest.mark.parametrize("short_by", [0, 700])
def test_a_read_that_ends_inside_its_polya_is_never_flagged(oracle_mod, short_by):
    """full_len == m and full_len < m: the poly(A) of a quarter of the reads reaches their end, the tail window of another quarter
    looks like poly(A), and no read is eligible -- every row keeps the plain call's bytes apart from bit 2"""
    from adapted_amd import lib

    spc = tc.spc_of("llr")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 24, full_len=m - short_by)
    first = tr.llr_first_rows(oracle_mod, sig, lens, spc, 24, key=("gpu-short", short_by))
    exp, counts, kinds = tr.look(oracle_mod, sig, lens, first, spc, "llr")
    assert counts == (0, 0, 0) and set(kinds) == {"ineligible"}
    # (what the guard keeps out: with one sample more behind the window the same signals are flagged)
    if short_by == 0:
        longer = np.full(24, m + 1, dtype=np.int32)
        assert tr.look(oracle_mod, sig, longer, oracle_mod.detect_llr(sig, longer, spc), spc, "llr")[1][2] >= 3
    eng = lib.Engine(spc, 24, m, device=0)
    plain, _ = eng.detect_llr_rows(sig, lens, 24, 24)
    got, _ = eng.detect_llr_rows(sig, lens, 24, 24, flag_truncated=True)
    assert eng.debug_truncated() == (0, 0, 0)
    _compare(got, exp, "llr", "full_len = m - %d" % short_by)
    assert (got["reserved_"] == lib.ROW_TRUNC_LOOKED).all()
    unmarked = got.copy()
    unmarked["reserved_"] = 0
    assert _canon(unmarked) == _canon(plain)
    eng.close()


def test_large_window_takes_the_large_segment_path(oracle_mod):
    """max_obs_trace = 40 000: T2's poly(A) partition is tens of thousands of samples long (k_partition_stats' large-segment path)"""
    from adapted_amd import lib

    spc, sig, lens, exp, counts, kinds = _llr_expected(oracle_mod, 40000, 24, 24)
    n, m = sig.shape
    flagged = [r for r in range(n) if kinds[r] == "flagged"]
    assert len(flagged) >= 3 and all(exp[r]["polya_len"] > 30000 for r in flagged) and "ineligible" in kinds
    eng = lib.Engine(spc, n, m, device=0)
    got, _ = eng.detect_llr_rows(sig, lens, n, 24, flag_truncated=True)
    assert eng.debug_truncated() == counts
    _compare(got, exp, "llr", "max_obs_trace 40000")
    eng.close()


@pytest.mark.parametrize("first0,second", [(0, False), (0, True), (192, True)])
def test_cnn_rows_equal_the_restated_rule(oracle_mod, first0, second):
    """adp_detect_cnn with the shipped weights, plain and with ADP_CNN_FALLBACK | ADP_CNN_SECOND_LLR; expected rows from the call's
    own bounds_out through the oracle.  From read 192 on the batch holds a read that fails the CNN path, passes the LLR path and is
    flagged: its row keeps bit 0"""
    from adapted_amd import lib
    from adapted_amd.detect import cnn

    spc = tc.spc_of("cnn")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 48, first=first0)
    n = 48
    eng = lib.Engine(spc, n, m, device=0)
    cnn.ensure_weights(eng, None, spc)
    plain, b0 = eng.detect_cnn_rows(sig, lens, n, n, fallback=second, second_opinion=second)
    assert eng.debug_truncated() == (0, 0, 0)
    got, bounds = eng.detect_cnn_rows(sig, lens, n, n, fallback=second, second_opinion=second, flag_truncated=True)
    assert np.array_equal(b0, bounds)
    first = oracle_mod.detect_cnn_from_preds(sig, lens, bounds, spc)
    if second:
        first = tr.second_llr(first, oracle_mod.detect_llr(sig, lens, tc.llr_copy(spc)))
    exp, counts, kinds = tr.look(oracle_mod, sig, lens, first, spc, "cnn")
    print("reads from %d on, second opinion %s: counts %s" % (first0, second, counts))
    assert sum(k == "flagged" for k in kinds) >= 3 and sum(k != "flagged" for k in kinds) >= 3
    assert eng.debug_truncated() == counts, (eng.debug_truncated(), counts)
    _compare(got, exp, "cnn", "cnn")
    if first0 == 192:
        assert any(e["_reserved"] == 7 for e in exp), "precondition: a flagged second-opinion row"
    pb, gb = _canon(plain), _canon(got)
    for r in range(n):
        if kinds[r] != "flagged":
            unmarked = got[r:r + 1].copy()
            unmarked["reserved_"] &= ~lib.ROW_TRUNC_LOOKED
            assert _canon(unmarked)[0][0] == pb[0][r] and gb[1].get(r) == pb[1].get(r), r
    # the operators
    out = cnn.combined_detect_cnn_llr(sig, lens, None, spc, flag_truncated=True) if second else cnn.combined_detect_cnn(sig, lens, None, spc, flag_truncated=True)
    assert [o.polya_truncated for o in out] == [e["polya_truncated"] for e in exp]
    eng.close()


def test_cnn_groups_and_lanes_give_the_same_rows(monkeypatch):
    """the look behind cnn_grouped: three minibatches of 16 in one chunk against ADP_CNN_GROUPS=3 over two lanes, with the second
    opinion, on the batch that holds a flagged second-opinion row"""
    from adapted_amd import lib
    from adapted_amd.detect import cnn

    spc = tc.spc_of("cnn")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 48, first=192)
    out = {}
    for groups in (None, "3"):
        monkeypatch.delenv("ADP_CNN_GROUPS", raising=False)
        monkeypatch.delenv("ADP_CNN_LANES", raising=False)
        if groups:
            monkeypatch.setenv("ADP_CNN_GROUPS", groups)
            monkeypatch.setenv("ADP_CNN_LANES", "2")
        eng = lib.Engine(spc, 48, m, device=0)
        cnn.ensure_weights(eng, None, spc)
        got, bounds = eng.detect_cnn_rows(sig, lens, 48, 16, fallback=True, second_opinion=True, flag_truncated=True)
        out[groups] = (_canon(got), bounds.tobytes(), eng.debug_truncated())
        eng.close()
    counts = out[None][2]
    assert counts[0] >= counts[1] >= counts[2] >= 3, counts
    assert out[None] == out["3"]


def test_validate_candidates_with_polya_truncated(oracle_mod):
    from adapted_amd import lib
    from adapted_amd.container_types import Boundaries
    from adapted_amd.detect import combined

    spc = tc.spc_of("llr")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 48)
    pick = [0, 1, 3, 7, 11]
    first = oracle_mod.detect_llr(sig[:24], lens[:24], spc)
    b = np.array([[first[r]["llr_adapter_end"], m if r % 4 == 3 else first[r]["llr_polya_end"]] for r in pick], dtype=np.int64)
    assert (b > 0).all()
    s, l = np.ascontiguousarray(sig[pick]), np.ascontiguousarray(lens[pick])
    want = oracle_mod.detect_cnn_from_preds(s, l, b, spc)
    assert sum(w["success"] for w in want) >= 3 and any(w["rna_preloaded_len"] is not None for w in want)
    eng = lib.Engine(spc, len(pick), m, device=0)
    plain = lib.rows_to_results(eng.validate_rows(s, l, len(pick), b), "cnn")
    got_rows = eng.validate_rows(s, l, len(pick), b, polya_truncated=True)
    got = lib.rows_to_results(got_rows, "cnn")
    for i, (g, p, w) in enumerate(zip(got, plain, want)):
        assert not row_diffs(p, tr.public(w)), (i, row_diffs(p, tr.public(w))[:5])
        blank = dict(tr.public(w), **{k: None for k in tr.RNA_FIELDS})
        assert not row_diffs(g, blank), (i, row_diffs(g, blank)[:5])
        assert g.polya_truncated is None
    assert (got_rows["reserved_"] == 0).all()
    eng.close()
    # the public validator honours Boundaries.polya_truncated
    r = pick[2]
    bd = Boundaries(adapter_start=0, adapter_end=int(b[2, 0]), polya_end=int(b[2, 1]), polya_end_topk=np.array([int(b[2, 1])]), polya_truncated=True)
    res = combined.validate_boundaries(sig[r, :m], bd, spc, int(lens[r]))
    blank = dict(tr.public(want[2]), **{k: None for k in tr.RNA_FIELDS})
    blank = {k.replace("cnn_", "llr_"): v for k, v in blank.items()}
    assert not row_diffs(res, blank) and res.polya_truncated is None and res.success


def test_unsupported_combinations_return_the_error_before_anything_runs():
    from adapted_amd import lib

    spc = tc.spc_of("llr")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 48)
    s, l = np.ascontiguousarray(sig[:4]), np.ascontiguousarray(lens[:4])
    rows = np.zeros(4, dtype=lib.ROW_DTYPE)
    mbs = np.zeros(4, dtype=np.int32)
    F = lib.ADP_FLAG_TRUNCATED

    def llr(eng, mb=4):
        return eng.lib.adp_detect_llr(eng._h, s, l, 4, m, mb, F, rows, mbs)

    no_check, overwrite = tc.spc_of("llr"), tc.spc_of("llr")
    no_check.mvs_polya.mvs_detect_check = False
    overwrite.mvs_polya.mvs_detect_overwrite = True
    for cfg, says in ((no_check, "mvs_detect_check"), (overwrite, "mvs_detect_overwrite")):
        eng = lib.Engine(cfg, 4, m, device=0)
        assert llr(eng) == ERR_UNSUPPORTED and says in eng.lib.adp_last_error().decode()
        assert eng.lib.adp_detect_llr(eng._h, s, l, 4, m, 4, 0, rows, mbs) == 0  # (the same call without the flag runs)
        eng.close()
    eng = lib.Engine(spc, 4, m, device=0, single_read_layout=True)
    assert llr(eng, 1) == ERR_UNSUPPORTED
    eng.close()
    eng = lib.Engine(spc, 4, m, device=0)
    assert eng.lib.adp_detect_start_peak(eng._h, s, l, 4, m, 4, F, rows) == ERR_UNSUPPORTED
    d_raw, d_len, d_cal = eng.dev_alloc(4 * m * 2), eng.dev_alloc(16), eng.dev_alloc(32)
    assert eng.lib.adp_detect_llr_i16(eng._h, d_raw, d_len, d_cal, d_cal + 16, 4, m, 4, lib.ADP_IN_DEVICE | F, rows, mbs) == ERR_UNSUPPORTED
    for p in (d_raw, d_len, d_cal):
        eng.dev_free(p)
    assert (rows["reserved_"] == 0).all() and llr(eng) == 0 and (rows["reserved_"] & lib.ROW_TRUNC_LOOKED).all()
    eng.close()


@pytest.mark.parametrize("int16", [False, True])
def test_host_pipeline_equals_the_direct_call(int16):
    from adapted_amd import lib
    from adapted_amd.pipeline import HostPipeline

    spc = tc.spc_of("llr")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 48)
    n, mb = 48, 24
    if int16:
        rng = np.random.default_rng(8)
        scale = rng.uniform(0.14, 0.2, n).astype(np.float32)
        offset = rng.uniform(-20.0, 20.0, n).astype(np.float32)
        raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
        pa = (scale[:, None] * (raw.astype(np.float32) + offset[:, None])).astype(np.float32)
    else:
        pa = sig
    eng = lib.Engine(spc, n, m, device=0)
    direct, _ = eng.detect_llr_rows(pa, lens, n, mb, flag_truncated=True)
    counts = eng.debug_truncated()
    eng.close()
    assert counts[2] >= 3 and (direct["reserved_"] & lib.ROW_POLYA_TRUNCATED != 0).sum() == counts[2]
    pipe = HostPipeline(spc, mb, m, device=0, primary="llr", int16_input=int16, group=2, flag_truncated=True)
    assert not pipe.native_i16
    out = {}

    def fill(get_buffers):
        bufs = get_buffers()
        if int16:
            bufs[0][:n], bufs[1][:n], bufs[2][:n], bufs[3][:n] = raw, lens, scale, offset
        else:
            bufs[0][:n], bufs[1][:n] = pa, lens
        yield n, 0

    pipe.run(fill, lambda k, rows: out.__setitem__(k, rows.copy()))
    pipe.close()
    assert _canon(out[0]) == _canon(direct)
