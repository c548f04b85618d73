"""ADP_CNN_SECOND_RESEGMENT on the GPU (adapted_amd/csrc/cnn_second_resegment.h, include/adapted_hip_second_resegment.h): a read the
CNN primary fails and whose LLR second opinion fails behind a first change point gets the row of the re-segmentation.

Yardsticks, both behaviour of calls that existed before the flag and that other tests pin -- never the code under test:
  A   adp_detect_cnn with ADP_CNN_SECOND_LLR alone (tests/test_gpu_cnn_second_opinion.py),
  B   adp_detect_llr with ADP_LLR_RESEGMENT on the same signals and minibatch size, with the LLR-switched copy of the configuration
      (_llr_spc of the second-opinion tests); tests/test_gpu_resegment.py holds B to the real reference's stored results.
THE RULE for every read: A's row byte for byte where it passes; else B's row with reserved_ |= 1 where B's row carries
ADP_ROW_RESEGMENTED; else A's row byte for byte.  Rows are compared with the registry token blanked and the overflow open-pore lists
resolved.  The three counts of adp_debug_fetch(26) follow from the yardsticks and the stored second segmentation (the reference's
eligible / p2 per read, tests/golden/resegment_*.npz, which B's own counts are held to): over the reads A leaves failing.

What an MI355X gave for ``main`` (48 reads), the same at minibatch 48 and 24: the CNN path fails 19 reads, the second opinion rescues 1
of them itself and leaves 18 failing (adp_debug_fetch(11): 19, 1, 18, 0); all 18 are eligible and get a p2, 15 are replaced by
re-segmented rows (reads 3, 4, 9, 10, 13, 15, 16, 27, 28, 33, 39, 40, 43, 45, 46) and 3 fail the second validation as well
(adp_debug_fetch(26): 18, 18, 15) -- the CPU oracle's 15 / 3 / 1 of 19.  ``extra``: (3, 0, 0): the CNN path passes the two stalled reads B
re-segments, the three eligible reads it leaves failing have no p2.  The 1104 tiled reads: (414, 414, 345)."""
import csv
import io
import json
import os

import numpy as np
import pytest

import resegment_cases as R
from test_gpu_cnn_fallback import _engine
from test_gpu_cnn_second_opinion import _llr_spc, _per_row

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
SO = "llr_resegment"
_YARD = {}


def _spc():
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.update_primary_method()
    spc.update_sig_preload_size()
    assert spc.primary_method == "cnn" and spc.sig_preload_size == R.M
    return spc


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _yardsticks(sig, lens, mb, sp=False, key=None):
    """A and B over one batch -> dict(A rows, B rows, B0 = B's call without its flag, mbs of the LLR call); cached under key"""
    from adapted_amd import lib

    if key is not None and (key, mb, sp) in _YARD:
        return _YARD[(key, mb, sp)]
    spc = _spc()
    n, m = sig.shape
    eng = _engine(spc, n, m)
    A, _ = eng.detect_cnn_rows(sig, lens, n, mb, fallback=True, second_opinion=True, with_start_peak=sp)
    assert eng.debug_second_resegment() == (0, 0, 0)
    so = eng.debug_cnn_second_opinion()
    eng.close()
    leng = lib.Engine(_llr_spc(spc), n, m, device=0)
    B0, mbs = leng.detect_llr_rows(sig, lens, n, mb, with_start_peak=sp)
    B, _ = leng.detect_llr_rows(sig, lens, n, mb, with_start_peak=sp, resegment=True)
    leng.close()
    _freeze(A, B, B0, mbs)
    out = dict(A=A, B=B, B0=B0, mbs=mbs, so=so)
    if key is not None:
        _YARD[(key, mb, sp)] = out
    return out


def _row_eligible(row, mb_status):
    """the rule's test on a failing LLR row (include/adapted_hip_resegment.h)"""
    from adapted_amd import lib

    a, p = lib.COLS.index("{primary}_adapter_end"), lib.COLS.index("{primary}_polya_end")
    if mb_status != lib.MB_OK or row["success"] != 0 or 9 <= row["fail_code"] <= 14:
        return False
    if not (int(row["present"]) >> a & 1 and int(row["present"]) >> p & 1):
        return False
    return row["col"][a] > 0 and row["col"][p] > row["col"][a]


def _rule(y, mb, g=None, times=1):
    """-> (expected canon, kinds per read: "A passes" / "replaced" / "second fails" / "no p2" / "not eligible", implied counts or None)"""
    from adapted_amd import lib

    A, B, B0, mbs = y["A"], y["B"], y["B0"], y["mbs"]
    n = A.size
    Bm = B.copy()
    Bm["reserved_"] |= lib.ROW_FROM_SECOND_LLR
    ca, cb = _per_row(A), _per_row(Bm)
    rows, lists, kinds = [], {}, []
    for i in range(n):
        take_b = A[i]["success"] != 1 and (int(B[i]["reserved_"]) & lib.ROW_RESEGMENTED) != 0
        src = cb if take_b else ca
        rows.append(src[0][i])
        if i in src[1]:
            lists[i] = src[1][i]
        if A[i]["success"] == 1:
            kinds.append("A passes")
        elif take_b:
            kinds.append("replaced")
        elif not _row_eligible(B0[i], mbs[i // mb]):
            kinds.append("not eligible")
        elif g is not None and g["p2"][i % len(g["p2"])] == 0:
            kinds.append("no p2")
        else:
            kinds.append("second fails")
    counts = None
    if g is not None:
        per = len(g["p2"])
        failing = [i for i in range(n) if A[i]["success"] != 1]
        # (the stored eligibility is the rule's on B's own first rows)
        assert [bool(g["eligible"][i % per]) for i in range(n)] == [bool(_row_eligible(B0[i], mbs[i // mb])) for i in range(n)]
        counts = (sum(bool(g["eligible"][i % per]) for i in failing), sum(int(g["p2"][i % per]) > 0 for i in failing), kinds.count("replaced"))
        assert n == per * times
    return (rows, lists), kinds, counts


def _flagged(eng, sig, lens, mb, sp=False):
    n = sig.shape[0]
    got, _ = eng.detect_cnn_rows(sig, lens, n, mb, fallback=True, second_opinion=SO, with_start_peak=sp)
    return got, eng.debug_second_resegment()


def _assert_rule(got, exp, kinds, what):
    from adapted_amd import lib

    gb, gl = _per_row(got)
    bad = [i for i in range(got.size) if gb[i] != exp[0][i] or gl.get(i) != exp[1].get(i)]
    assert not bad, (what, "rows that do not follow the rule", [(i, kinds[i], int(got[i]["success"]), int(got[i]["reserved_"])) for i in bad[:8]])
    marked = [i for i in range(got.size) if int(got[i]["reserved_"]) & lib.ROW_RESEGMENTED]
    assert marked == [i for i, k in enumerate(kinds) if k == "replaced"]
    for i in marked:
        assert int(got[i]["reserved_"]) & (lib.ROW_FROM_SECOND_LLR | lib.ROW_RESEGMENTED) == 33 and got[i]["success"] == 1


# ---- 1. the 48 reads
@pytest.mark.parametrize("mb", [48, 24])
def test_main_rows_follow_the_rule(mb):
    """(counts on the GPU: see the module's docstring)"""
    sig, lens = R.batch("main")
    y = _yardsticks(sig, lens, mb, key="main")
    exp, kinds, counts = _rule(y, mb, R.load("main", mb))
    eng = _engine(_spc(), *sig.shape)
    got, got_counts = _flagged(eng, sig, lens, mb)
    so_counts = eng.debug_cnn_second_opinion()
    eng.close()
    tally = {k: kinds.count(k) for k in sorted(set(kinds))}
    print("main, minibatch %d: %s, counts %s (implied %s), second opinion %s" % (mb, tally, got_counts, counts, so_counts))
    print("main, minibatch %d: replaced %s" % (mb, [i for i, k in enumerate(kinds) if k == "replaced"]))
    if mb == 48:
        # the three kinds among the reads the CNN path fails: replaced; second validation fails as well; never eligible.  The third
        # kind is read 44 of the stored results, "ineligible" because its LLR row PASSES: here that is a read the second opinion
        # rescues itself (A carries its row with reserved_ bit 0), or one whose failing LLR row is not eligible.  On the GPU the
        # precondition is met by the one rescued read alone: no failing LLR row of ``main`` is ineligible.  An eligible read without
        # a p2 belongs to none of the three and is not counted.
        rescued = int(((y["A"]["reserved_"] & 1) != 0).sum())
        assert rescued == y["so"][1] and y["so"][0] == rescued + y["so"][2] == rescued + sum(tally.get(k, 0) for k in tally if k != "A passes")
        third = rescued + tally.get("not eligible", 0)
        print("main, minibatch 48: of the %d reads the CNN path fails: %d replaced / %d fail the second validation / %d never eligible "
              "(%d rescued by the second opinion, %d not eligible); %d eligible without a p2"
              % (y["so"][0], tally.get("replaced", 0), tally.get("second fails", 0), third, rescued, tally.get("not eligible", 0), tally.get("no p2", 0)))
        assert tally.get("replaced", 0) >= 10, tally
        assert tally.get("second fails", 0) >= 1, tally
        assert third >= 1, (tally, rescued)
        assert tally.get("A passes", 0) >= 1, tally
    else:
        assert tally.get("replaced", 0) >= 1 and tally.get("A passes", 0) >= 1, tally
    _assert_rule(got, exp, kinds, "main %d" % mb)
    assert got_counts == counts
    assert so_counts == y["so"], "adp_debug_fetch(11) keeps its meaning: the second opinion's own counts, those of A"


# ---- 2. the hand-made reads beside a dropped minibatch
def test_extra_rows_follow_the_rule():
    from adapted_amd import lib

    sig, lens = R.batch("extra")
    mb = R.X_MB
    y = _yardsticks(sig, lens, mb, key="extra")
    g = R.load("extra", mb)
    exp, kinds, counts = _rule(y, mb, g)
    assert y["mbs"].tolist() == [lib.MB_MAD_ZERO, lib.MB_OK]
    eng = _engine(_spc(), *sig.shape)
    got, got_counts = _flagged(eng, sig, lens, mb)
    eng.close()
    print("extra: %s, counts %s (implied %s)" % (dict(zip(R.X_NAMES, kinds)), got_counts, counts))
    # what the batch exercises, from the yardsticks and the stored second segmentation
    failing = [i for i, k in enumerate(kinds) if k != "A passes"]
    assert any(i < mb for i in failing) and any(g["eligible"][i] for i in failing), "a dropped minibatch beside one with eligible reads"
    assert "no p2" in kinds and "not eligible" in kinds[mb:], "reads without an adapter or a poly(A) end, and p2 == 0"
    # (the CNN path passes the two stalled reads that B re-segments: on this batch the phase selects and replaces nothing else)
    assert any(g["eligible"][i] and lens[i] < R.M for i in failing), "an eligible read that ends inside the window"
    _assert_rule(got, exp, kinds, "extra")
    assert got_counts == counts


# ---- 3. flag off
def test_flag_off_keeps_the_bytes_and_calls_alternate():
    sig, lens = R.batch("main")
    n, mb = sig.shape[0], 24
    y = _yardsticks(sig, lens, mb, key="main")
    exp, kinds, counts = _rule(y, mb, R.load("main", mb))
    eng = _engine(_spc(), *sig.shape)
    for turn in range(2):
        got, got_counts = _flagged(eng, sig, lens, mb)
        _assert_rule(got, exp, kinds, "flagged, turn %d" % turn)
        assert got_counts == counts
        for value in (True, "llr"):
            plain, _ = eng.detect_cnn_rows(sig, lens, n, mb, fallback=True, second_opinion=value)
            assert eng.debug_second_resegment() == (0, 0, 0)
            assert _per_row(plain) == _per_row(y["A"]), "the plain second-opinion call on an engine that ran the flagged one"
    eng.close()


# ---- 4. start peak
def test_start_peak_columns_are_the_cnn_calls():
    from adapted_amd import lib

    sig, lens = R.batch("main")
    n, mb = sig.shape[0], 24
    y = _yardsticks(sig, lens, mb, sp=True, key="main")
    exp, kinds, counts = _rule(y, mb, R.load("main", mb))
    eng = _engine(_spc(), *sig.shape)
    got, got_counts = _flagged(eng, sig, lens, mb, sp=True)
    cnn_only, _ = eng.detect_cnn_rows(sig, lens, n, mb, fallback=True, with_start_peak=True)
    eng.close()
    sp = slice(lib.COLS.index("start_peak_idx"), lib.COLS.index("start_peak_open_pore_idx") + 1)
    mask = np.uint64(31 << sp.start)
    replaced = [i for i, k in enumerate(kinds) if k == "replaced"]
    assert sum(bool(cnn_only["present"][i] & mask) for i in replaced) >= 3, "precondition: replaced reads with start-peak columns"
    for i in replaced:
        assert got["col"][i, sp].tobytes() == cnn_only["col"][i, sp].tobytes() and got["start_peak_type"][i] == cnn_only["start_peak_type"][i]
        assert got["present"][i] & mask == cnn_only["present"][i] & mask
    _assert_rule(got, exp, kinds, "with_start_peak")
    assert got_counts == counts


# ---- 5. resident input, device rows, grouped execution
def test_resident_input_device_rows_and_lanes_give_the_same_bytes(monkeypatch):
    import torch

    from adapted_amd import lib
    from adapted_amd.detect import cnn

    sig, lens = R.batch("main")
    n, mb = sig.shape[0], 24
    spc = _spc()
    y = _yardsticks(sig, lens, mb, key="main")
    exp, kinds, counts = _rule(y, mb, R.load("main", mb))
    eng = _engine(spc, *sig.shape)
    dsig = torch.from_numpy(np.array(sig)).cuda()
    dlen = torch.from_numpy(np.array(lens)).cuda()
    torch.cuda.synchronize()
    res = cnn.detect_rows_device_second_opinion(eng, dsig.data_ptr(), dlen.data_ptr(), n, np.array(lens), None, spc, mb, second_opinion=SO)
    assert eng.debug_second_resegment() == counts
    _assert_rule(res, exp, kinds, "resident input")
    drows = eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
    none, _ = eng.detect_cnn_rows(dsig.data_ptr(), dlen.data_ptr(), n, mb, device_ptrs=True, rows_dev=drows, want_bounds=False, fallback=True,
                                  second_opinion=SO)
    back = np.zeros(n, dtype=lib.ROW_DTYPE)
    eng.d2h(back, drows)
    eng.dev_free(drows)
    assert none is None and eng.debug_second_resegment() == counts
    _assert_rule(eng.attach_open_pores(back), exp, kinds, "rows on the device")
    eng.close()
    for env in ({"ADP_GROUPS": "0", "ADP_LANES": "2"}, {"ADP_CNN_GROUPS": "0", "ADP_CNN_LANES": "2", "ADP_GROUPS": "0", "ADP_LANES": "2"},
                {"ADP_G2_WINDOW": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = _engine(spc, *sig.shape)
        got, got_counts = _flagged(eng, sig, lens, mb)
        eng.close()
        for k in env:
            monkeypatch.delenv(k)
        _assert_rule(got, exp, kinds, env)
        assert got_counts == counts, env


# ---- 6. both selections across their 1024-read step
def test_selections_carry_their_totals_past_1024_reads():
    sig, lens = R.tiled("main", 23)
    n, mb = sig.shape[0], 48
    assert n == 1104
    y = _yardsticks(sig, lens, mb)
    exp, kinds, counts = _rule(y, mb, R.load("main", mb), times=23)
    eng = _engine(_spc(), n, sig.shape[1])
    got, got_counts = _flagged(eng, sig, lens, mb)
    so = eng.debug_cnn_second_opinion()
    eng.close()
    replaced = [i for i, k in enumerate(kinds) if k == "replaced"]
    print("1104 reads: second opinion %s, counts %s, %d replaced" % (so, got_counts, len(replaced)))
    assert sum(i < 1024 for i in replaced) >= 3 and sum(i >= 1024 for i in replaced) >= 3
    _assert_rule(got, exp, kinds, "1104 reads")
    assert got_counts == counts


# ---- 7. int16
def test_int16_rows_equal_the_float32_calls():
    from test_gpu_cnn_i16 import _Dev, _assert_same

    sig, lens = R.batch("main")
    n, mb = sig.shape[0], 24
    rng = np.random.default_rng(8)
    scale = rng.uniform(0.14, 0.2, n).astype(np.float32)
    offset = rng.uniform(-20.0, 20.0, n).astype(np.float32)
    raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
    dev = _Dev(_spc(), raw, scale, offset, np.array(lens))
    e = dev.eng
    e.calibrate_i16(dev.d_raw, dev.d_len, dev.d_cal, dev.d_cal + n * 4, n, dev.d_f32)
    rows, bounds = e.detect_cnn_rows(dev.d_f32, dev.d_len, n, mb, device_ptrs=True, fallback=True, second_opinion=SO)
    want = dict(dev._result(rows, bounds), sr=e.debug_second_resegment())
    rows, bounds = e.detect_cnn_rows_i16(dev.d_raw, dev.d_len, dev.d_cal, dev.d_cal + n * 4, n, mb, fallback=True, second_opinion=SO)
    got = dict(dev._result(rows, bounds), sr=e.debug_second_resegment())
    dev.close()
    print("int16: counts %s" % (want["sr"],))
    assert want["sr"][2] >= 3, "precondition: re-segmented rows in the quantised batch"
    _assert_same(got, want, "int16 against calibrate + float32")
    assert got["sr"] == want["sr"]


# ---- 8. open pores: no case.  No edit of a ``main`` read that was tried gives B a re-segmented row with an open-pore list: 250-pA
# samples inside the true adapter of reads 1, 3, 4, 7, 9, 10, 13 and 15 -- every 10th to every 50th sample, 4 to 115 of them, 100 to
# 400 samples behind the front stretch and 300 to 800 in front of the adapter's end -- make B's second validation fail for every
# read and every spacing (the re-segmented row only returns with no sample edited).  The lists of the second rows go through
# k_validate's arena code as every other phase's do.  No case makes an attempt fall short of the arena in this phase either (the
# fourth attempt of cnn_attempts; the case below overflows in the second opinion's phase with the flag on): no test makes the replaced
# rows write into the arena (says so too).


def test_arena_overflow_with_the_flag_repeats_the_call():
    """test_arena_overflow_in_the_second_opinion_repeats_the_call's 190 copies of read 5 with the flag on: the call runs under the
    flag's attempt bound (cnn_attempts) and repeats on a larger arena; the attempt falls short in the SECOND OPINION's phase, whose
    rows all pass, so the new phase selects nothing and every row equals the plain second-opinion call's on a fresh engine"""
    from test_gpu_cnn_second_opinion import _open_pore_read

    spc, s, l = _open_pore_read(5, 2300)
    n, pores = 190, 199
    bs, bl = np.ascontiguousarray(np.repeat(s, n, axis=0)), np.ascontiguousarray(np.repeat(l, n))
    out = {}
    for choice in (True, SO):
        eng = _engine(spc, n, s.shape[1])  # (fresh: its arena is the initial one, 65 536 entries)
        rows, _ = eng.detect_cnn_rows(bs, bl, n, n, fallback=True, second_opinion=choice)
        used = np.zeros(1, dtype=np.uint64)
        eng._check(eng.lib.adp_open_pores_arena(eng._h, None, 0, used))
        out[choice] = (rows, int(used[0]), eng.debug_cnn_second_opinion(), eng.debug_second_resegment())
        eng.close()
    (want, used_a, so_a, sr_a), (got, used, so, sr) = out[True], out[SO]
    print("190 copies of read 5: arena entries in use %d (plain %d), second opinion %s, re-segmentation %s" % (used, used_a, so, sr))
    assert used_a > 65536 and used > 65536, "precondition: more than the initial arena in use"
    assert so_a == so == (n, n, 0, 0) and sr_a == sr == (0, 0, 0)
    assert (got["reserved_"] == 1).all() and (got["success"] == 1).all() and (got["n_open_pores"] == pores).all()
    gb, gl = _per_row(got)
    assert (gb, gl) == _per_row(want) and len(gl) == n


# ---- the refusals
def test_refusals_leave_the_handle_usable():
    from adapted_amd import lib

    sig, lens = R.batch("main")
    m = R.M
    s, l = np.ascontiguousarray(sig[:4]), np.ascontiguousarray(lens[:4])
    rows = np.zeros(4, dtype=lib.ROW_DTYPE)
    spc = _spc()
    # (bounds_out takes int64 [n, 1 + max(k, 1)] from every call that runs: the preset's k is 10)
    bounds = np.zeros((4, 1 + max(1, int(spc.cnn_boundaries.polya_cand_k))), dtype=np.int64)
    mbs = np.zeros(4, dtype=np.int32)
    F, L2 = lib.ADP_CNN_SECOND_RESEGMENT, lib.ADP_CNN_SECOND_LLR

    def cnn(eng, flags, out=rows):
        return eng.lib.adp_detect_cnn(eng._h, s, l, 4, m, 4, flags, out, bounds)

    def cnn_i16(eng, bufs, flags):
        """adp_detect_cnn_i16 runs the same check: the refusals come before anything reads the (unwritten) device buffers"""
        d_raw, d_len, d_cal = bufs
        return eng.lib.adp_detect_cnn_i16(eng._h, d_raw, d_len, d_cal, d_cal + 16, 4, m, 4, lib.ADP_IN_DEVICE | flags, rows, bounds)

    def refused(rc, eng, says, code=ERR_UNSUPPORTED):
        assert rc == code and says in eng.lib.adp_last_error().decode() and not rows.tobytes().strip(b"\0"), (says, rc)

    def bufs_of(eng):
        return eng.dev_alloc(4 * m * 2), eng.dev_alloc(16), eng.dev_alloc(32)

    def free(eng, bufs):
        for p in bufs:
            eng.dev_free(p)

    eng = _engine(spc, 4, m)
    bufs = bufs_of(eng)
    refused(cnn(eng, F), eng, "ADP_CNN_SECOND_LLR", ERR_INVALID)
    refused(cnn(eng, F | L2, None), eng, "rows_out", ERR_INVALID)
    refused(cnn(eng, F | L2 | lib.ADP_FLAG_TRUNCATED), eng, "ADP_FLAG_TRUNCATED")
    refused(cnn_i16(eng, bufs, F), eng, "ADP_CNN_SECOND_LLR", ERR_INVALID)
    refused(cnn_i16(eng, bufs, F | L2 | lib.ADP_FLAG_TRUNCATED), eng, "ADP_FLAG_TRUNCATED")
    refused(eng.lib.adp_detect_llr(eng._h, s, l, 4, m, 4, F, rows, mbs), eng, "ADP_CNN_SECOND_RESEGMENT")
    refused(eng.lib.adp_detect_start_peak(eng._h, s, l, 4, m, 4, F, rows), eng, "ADP_CNN_SECOND_RESEGMENT")
    d_raw, d_len, d_cal = bufs
    refused(eng.lib.adp_detect_llr_i16(eng._h, d_raw, d_len, d_cal, d_cal + 16, 4, m, 4, lib.ADP_IN_DEVICE | F, rows, mbs), eng, "ADP_CNN_SECOND_RESEGMENT")
    free(eng, bufs)
    assert eng.debug_second_resegment() == (0, 0, 0)
    assert cnn(eng, L2) == 0 and cnn(eng, F | L2) == 0
    rows[:] = 0
    eng.close()
    over = _spc()
    over.mvs_polya.mvs_detect_overwrite = True
    eng = _engine(over, 4, m)
    bufs = bufs_of(eng)
    refused(cnn(eng, F | L2), eng, "mvs_detect_overwrite")
    refused(cnn_i16(eng, bufs, F | L2), eng, "mvs_detect_overwrite")
    free(eng, bufs)
    eng.close()
    eng = lib.Engine(spc, 4, m, device=0, single_read_layout=True)
    bufs = bufs_of(eng)
    refused(cnn(eng, F | L2), eng, "single-read")
    refused(cnn_i16(eng, bufs, F | L2), eng, "single-read")
    free(eng, bufs)
    eng.close()


# ---- 9. the command line
def _cli(tmp_path, name, bundle, *options):
    from adapted_amd import main as cli

    out = tmp_path / name
    cli.main(["detect", "-i", str(bundle), "-o", str(out), "-c", "RNA004", "-s", "24", "-b", "4000"] + list(options))
    (run,) = [d for d in os.listdir(out) if d.startswith("adapted_")]
    files = {}
    for sub, f in (("boundaries", "detected_boundaries_0.csv"), ("failed_reads", "failed_reads_0.csv")):
        files[f] = (out / run / sub / f).read_bytes()
    with open(out / run / "command.json") as fh:
        files["command"] = json.load(fh)
    return files


def _table(data):
    lines = list(csv.reader(io.StringIO(data.decode())))
    at = lines[0].index("read_id")
    return lines[0], {ln[at]: ln for ln in lines[1:]}


def test_cli_writes_the_resegmented_reads_with_their_llr_columns(tmp_path):
    """`adapted detect -c RNA004 --second_opinion llr_resegment` on a bundle of the ``main`` reads (as an int16 bundle calibrates
    them, so that the raw bundle holds the same reads)"""
    from adapted_amd import lib
    from test_gpu_cnn_i16 import _calibrated

    sig, lens = R.batch("main")
    n, mb = sig.shape[0], 24
    rng = np.random.default_rng(8)
    scale = rng.uniform(0.14, 0.2, n).astype(np.float32)
    offset = rng.uniform(-20.0, 20.0, n).astype(np.float32)
    raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
    pa = _calibrated(raw, scale, offset, np.array(lens))
    y = _yardsticks(pa, lens, mb)
    exp, kinds, _ = _rule(y, mb)
    replaced = [i for i, k in enumerate(kinds) if k == "replaced"]
    assert len(replaced) >= 3, "precondition: re-segmented reads in the calibrated batch"
    ids = np.array(["read_%04d" % i for i in range(n)], dtype=object)
    np.savez(tmp_path / "reads_0.npz", signals=pa, full_lengths=np.array(lens), read_ids=ids)
    np.savez(tmp_path / "raw_0.npz", raw=raw, scale=scale, offset=offset, full_lengths=np.array(lens), read_ids=ids)
    got = _cli(tmp_path, "flagged", tmp_path / "reads_0.npz", "--second_opinion", "llr_resegment")
    assert got["command"]["second_opinion"] == "llr_resegment"  # (`adapted continue` repeats it)
    plain = _cli(tmp_path, "plain", tmp_path / "reads_0.npz", "--second_opinion", "llr")
    head, passed = _table(got["detected_boundaries_0.csv"])
    _, failed = _table(got["failed_reads_0.csv"])
    _, plain_passed = _table(plain["detected_boundaries_0.csv"])
    _, plain_failed = _table(plain["failed_reads_0.csv"])
    col = {name: head.index(name) for name in ("adapter_start", "llr_adapter_end", "llr_polya_end", "cnn_adapter_end", "llr_detect_log", "adapter_end")}
    a_end, p_end = lib.COLS.index("{primary}_adapter_end"), lib.COLS.index("{primary}_polya_end")
    for i in range(n):
        rid = ids[i]
        if i in replaced:
            ln, b = passed[rid], y["B"][i]
            code = (int(b["reserved_"]) & lib.ROW_FIRST_FAIL_MASK) >> lib.ROW_FIRST_FAIL_SHIFT
            assert rid in plain_failed and rid not in failed
            # (pandas prints a column that is empty on some lines as floats)
            assert float(ln[col["adapter_start"]]) == y["B0"][i]["col"][a_end], "adapter_start = a1, the second opinion's adapter end"
            assert (float(ln[col["llr_adapter_end"]]), float(ln[col["llr_polya_end"]]), ln[col["cnn_adapter_end"]]) == (b["col"][a_end], b["col"][p_end], "")
            assert ln[col["llr_detect_log"]] == lib.resegmented_row_log(code)
        else:
            assert passed.get(rid) == plain_passed.get(rid) and failed.get(rid) == plain_failed.get(rid), (i, kinds[i])
    native = _cli(tmp_path, "native", tmp_path / "reads_0.npz", "--second_opinion", "llr_resegment", "--native_csv")
    i16 = _cli(tmp_path, "i16", tmp_path / "raw_0.npz", "--second_opinion", "llr_resegment", "--int16_ingest")
    for f in ("detected_boundaries_0.csv", "failed_reads_0.csv"):
        assert native[f] == got[f], ("--native_csv", f)
        assert i16[f] == got[f], ("--int16_ingest", f)
