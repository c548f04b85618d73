"""ADP_LLR_RESEGMENT on the GPU (adapted_amd/csrc/llr_resegment.h): every row of a flagged call against what the real reference
stored for the rule (tests/golden/resegment_*.npz through tests/resegment_cases.py: the first row, the second segmentation, the
validation from the first adapter end), every field without tolerance, the marks in ``reserved_`` and the counts included; every
row the phase does not replace against the bytes of the same call without the flag."""
import numpy as np
import pytest

import resegment_cases as R
from util import row_diffs

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -4
_ROWS = {}


def _canon(rows):
    """(bytes of every row with the registry token blanked, {read: overflow open-pore list})"""
    from adapted_amd import lib

    lists = {int(i): lib._OPEN_PORES_MORE[int(rows[i]["open_pores_more"])].tolist() for i in np.flatnonzero(rows["n_open_pores"] > lib.MAX_OPEN_PORES)}
    r = rows.copy()
    r["open_pores_more"] = 0
    return [r[i].tobytes() for i in range(r.size)], lists


def _public(d):
    return {k: v for k, v in d.items() if not k.startswith("_")}


def _compare(rows, exp, what):
    """every field of every row that exists in the reference (a dropped minibatch's reads: nothing present, no verdict)"""
    from adapted_amd import lib

    res = lib.rows_to_results(rows, "llr")
    bad = []
    for i, (g, e) in enumerate(zip(res, exp)):
        if e is None:
            empty = (int(rows[i]["present"]), int(rows[i]["success"]), int(rows[i]["fail_code"]), int(rows[i]["reserved_"]))
            d = [] if empty == (0, 0, 0, 0) else [("row of a dropped minibatch: present, success, fail_code, reserved_", empty, (0, 0, 0, 0))]
        else:
            d = row_diffs(g, _public(e))
            if g.llr_detect_log != e["llr_detect_log"]:
                d.append(("llr_detect_log", g.llr_detect_log, e["llr_detect_log"]))
            if int(rows[i]["reserved_"]) != e["_reserved"]:
                d.append(("reserved_", int(rows[i]["reserved_"]), e["_reserved"]))
        if d:
            bad.append((i, d[:6]))
    assert not bad, (what, bad[:6])


def _unreplaced_rows_keep_their_bytes(got, plain, kinds):
    pb, gb = _canon(plain), _canon(got)
    for r, kind in enumerate(kinds):
        if kind != "kept":
            assert gb[0][r] == pb[0][r] and gb[1].get(r) == pb[1].get(r), "read %d (%s) keeps the bytes of the call without the flag" % (r, kind)
        else:
            assert gb[0][r] != pb[0][r]


def _run(name, mb, **options):
    """(plain rows, flagged rows, counts) of one engine, cached for the tests that start from test 1's rows"""
    from adapted_amd import lib

    key = (name, mb, tuple(sorted(options.items())))
    if key not in _ROWS:
        sig, lens = R.batch(name)
        n, m = sig.shape
        eng = lib.Engine(R.spc_of(), n, m, device=0)
        plain, mbs0 = eng.detect_llr_rows(sig, lens, n, mb, **options)
        assert eng.debug_resegment() == (0, 0, 0) and (plain["reserved_"] == 0).all()
        got, mbs = eng.detect_llr_rows(sig, lens, n, mb, resegment=True, **options)
        counts = eng.debug_resegment()
        assert (mbs == mbs0).all()
        again, _ = eng.detect_llr_rows(sig, lens, n, mb, **options)  # the flag leaves nothing behind
        assert _canon(again) == _canon(plain) and eng.debug_resegment() == (0, 0, 0)
        eng.close()
        for a in (plain, got):
            a.setflags(write=False)
        _ROWS[key] = (plain, got, counts, mbs)
    return _ROWS[key]


@pytest.mark.parametrize("name,mb", R.RUNS)
def test_rows_equal_the_reference(name, mb):
    """host pointers; the 48 reads with minibatch 24 and 48, and the hand-made reads beside a minibatch the primary drops"""
    from adapted_amd import lib

    g = R.load(name, mb)
    exp, counts, kinds = R.expected(g)
    plain, got, got_counts, mbs = _run(name, mb)
    print("%s, minibatch %d: counts %s, %s" % (name, mb, got_counts, {k: kinds.count(k) for k in sorted(set(kinds))}))
    first = [None if r is None else dict(r, llr_detect_log="", _reserved=0) for r in g["first"]]
    _compare(plain, first, "flag off: the reference's first rows")
    assert got_counts == counts, (got_counts, counts)
    if (name, mb) == ("main", 48):
        assert got_counts == (24, 24, 21)
    if name == "extra":
        assert mbs.tolist() == [lib.MB_MAD_ZERO, lib.MB_OK] and kinds[:R.X_MB] == ["dropped"] * R.X_MB
    else:
        assert (mbs == lib.MB_OK).all()
    _compare(got, exp, "flag on")
    _unreplaced_rows_keep_their_bytes(got, plain, kinds)
    assert ((got["reserved_"] & lib.ROW_RESEGMENTED) != 0).sum() == counts[2]


def test_device_pointers_and_device_rows_give_the_same_rows():
    import torch

    from adapted_amd import lib

    sig, lens = R.batch("main")
    n, m = sig.shape
    _, want, counts, _ = _run("main", 24)
    eng = lib.Engine(R.spc_of(), n, m, device=0)
    dsig = torch.from_numpy(np.array(sig)).cuda()
    dlen = torch.from_numpy(np.array(lens)).cuda()
    torch.cuda.synchronize()
    res, _ = eng.detect_llr_rows(dsig.data_ptr(), dlen.data_ptr(), n, 24, device_ptrs=True, resegment=True)
    assert eng.debug_resegment() == counts and _canon(res) == _canon(want), "resident input"
    drows = eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
    none, _ = eng.detect_llr_rows(dsig.data_ptr(), dlen.data_ptr(), n, 24, device_ptrs=True, rows_dev=drows, resegment=True, tails_nan=True)
    back = np.zeros(n, dtype=lib.ROW_DTYPE)
    eng.d2h(back, drows)
    eng.dev_free(drows)
    assert none is None and eng.debug_resegment() == counts and _canon(eng.attach_open_pores(back)) == _canon(want), "rows on the device, ADP_TAILS_NAN"
    eng.close()


def test_start_peak_columns_are_the_first_rows():
    from adapted_amd import lib

    g = R.load("main", 24)
    _, counts, kinds = R.expected(g)
    plain, got, got_counts, _ = _run("main", 24, with_start_peak=True)
    assert got_counts == counts
    first = lib.rows_to_results(plain, "llr")
    kept = [r for r, k in enumerate(kinds) if k == "kept"]
    assert sum(first[r].start_peak_idx is not None for r in kept) >= 3, "precondition: re-segmented reads with start-peak columns to carry"
    exp, _, _ = R.expected(g, first=[dict(g["first"][r], **{k: getattr(first[r], k) for k in R.SP_FIELDS}) for r in range(len(first))])
    _compare(got, exp, "with_start_peak")
    _unreplaced_rows_keep_their_bytes(got, plain, kinds)
    sp = slice(lib.COLS.index("start_peak_idx"), lib.COLS.index("start_peak_open_pore_idx") + 1)
    mask = np.uint64(31 << sp.start)
    for r in kept:
        assert got["col"][r, sp].tobytes() == plain["col"][r, sp].tobytes() and got["start_peak_type"][r] == plain["start_peak_type"][r]
        assert got["present"][r] & mask == plain["present"][r] & mask


@pytest.mark.parametrize("env", [{"ADP_GROUPS": "2", "ADP_LANES": "2"}, {"ADP_G2_WINDOW": "0"}, {"ADP_GROUPS": "2", "ADP_LANES": "2", "ADP_G2_WINDOW": "0"}])
def test_grouping_and_the_whole_trace_pass_give_the_same_bytes(monkeypatch, env):
    """a group's workspace is recycled by the next: the phase must not depend on what the first pass left there"""
    from adapted_amd import lib

    for name, mb in (("main", 24), ("extra", R.X_MB)):
        _, want, counts, mbs0 = _run(name, mb)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sig, lens = R.batch(name)
        n, m = sig.shape
        eng = lib.Engine(R.spc_of(), n, m, device=0)
        got, mbs = eng.detect_llr_rows(sig, lens, n, mb, resegment=True)
        assert eng.debug_resegment() == counts and (mbs == mbs0).all()
        eng.close()
        for k in env:
            monkeypatch.delenv(k)
        assert _canon(got) == _canon(want), (name, env)


def test_selection_carries_its_total_past_1024_reads():
    """the 48 reads tiled 23 times in minibatches of 48: every minibatch is the stored one"""
    from adapted_amd import lib

    _, want, counts, _ = _run("main", 48)
    sig, lens = R.tiled("main", 23)
    n, m = sig.shape
    assert n == 1104
    eng = lib.Engine(R.spc_of(), n, m, device=0)
    got, mbs = eng.detect_llr_rows(sig, lens, n, 48, resegment=True)
    assert eng.debug_resegment() == tuple(23 * c for c in counts) and (mbs == lib.MB_OK).all()
    eng.close()
    kept = np.flatnonzero((got["reserved_"] & lib.ROW_RESEGMENTED) != 0)
    assert (kept < 1024).sum() >= 3 and (kept >= 1024).sum() >= 3
    tile = _canon(want)
    g = _canon(got)
    assert g[0] == tile[0] * 23 and g[1] == {r + 48 * t: v for t in range(23) for r, v in tile[1].items()}


def test_a_batch_without_eligible_reads():
    from adapted_amd import lib

    g = R.load("main", 48)
    sig, lens = R.batch("main")
    pick = [r for r in range(R.N_MAIN) if r % 6 in (0, 2, 5)]
    s, l = np.ascontiguousarray(sig[pick]), np.ascontiguousarray(lens[pick])
    assert not g["eligible"][pick].any()
    eng = lib.Engine(R.spc_of(), len(pick), R.M, device=0)
    plain, _ = eng.detect_llr_rows(s, l, len(pick), len(pick))
    got, _ = eng.detect_llr_rows(s, l, len(pick), len(pick), resegment=True)
    assert eng.debug_resegment() == (0, 0, 0)
    eng.close()
    assert (plain["success"] == 1).all(), "precondition: nothing fails in this call"
    assert _canon(got) == _canon(plain)


def test_unsupported_combinations_return_the_error_before_anything_runs():
    from adapted_amd import lib

    spc = R.spc_of()
    m = R.M
    sig, lens = R.batch("main")
    s, l = np.ascontiguousarray(sig[:4]), np.ascontiguousarray(lens[:4])
    rows = np.zeros(4, dtype=lib.ROW_DTYPE)
    mbs = np.zeros(4, dtype=np.int32)
    F = lib.ADP_LLR_RESEGMENT

    def llr(eng, flags, mb=4):
        return eng.lib.adp_detect_llr(eng._h, s, l, 4, m, mb, flags, rows, mbs)

    def refused(rc, eng, says):
        assert rc == ERR_UNSUPPORTED and says in eng.lib.adp_last_error().decode() and not rows.tobytes().strip(b"\0"), says

    overwrite = R.spc_of()
    overwrite.mvs_polya.mvs_detect_overwrite = True
    eng = lib.Engine(overwrite, 4, m, device=0)
    refused(llr(eng, F), eng, "mvs_detect_overwrite")
    assert llr(eng, 0) == 0  # (the same call without the flag runs)
    rows[:] = 0
    eng.close()
    eng = lib.Engine(spc, 4, m, device=0, single_read_layout=True)
    refused(llr(eng, F, 1), eng, "single-read")
    assert llr(eng, 0, 1) == 0
    rows[:] = 0
    eng.close()
    eng = lib.Engine(spc, 4, m, device=0)
    refused(llr(eng, F | lib.ADP_FLAG_TRUNCATED), eng, "ADP_FLAG_TRUNCATED")
    refused(eng.lib.adp_detect_start_peak(eng._h, s, l, 4, m, 4, F, rows), eng, "ADP_LLR_RESEGMENT")
    bounds = np.zeros((4, 2), dtype=np.int64)
    refused(eng.lib.adp_detect_cnn(eng._h, s, l, 4, m, 4, F, rows, bounds), eng, "ADP_LLR_RESEGMENT")
    d_raw, d_len, d_cal = eng.dev_alloc(4 * m * 2), eng.dev_alloc(16), eng.dev_alloc(32)
    refused(eng.lib.adp_detect_llr_i16(eng._h, d_raw, d_len, d_cal, d_cal + 16, 4, m, 4, lib.ADP_IN_DEVICE | F, rows, mbs), eng, "ADP_LLR_RESEGMENT")
    refused(eng.lib.adp_detect_cnn_i16(eng._h, d_raw, d_len, d_cal, d_cal + 16, 4, m, 4, lib.ADP_IN_DEVICE | F, rows, bounds), eng, "ADP_LLR_RESEGMENT")
    for p in (d_raw, d_len, d_cal):
        eng.dev_free(p)
    assert eng.debug_resegment() == (0, 0, 0)
    assert llr(eng, lib.ADP_FLAG_TRUNCATED) == 0 and llr(eng, 0) == 0 and llr(eng, F) == 0
    eng.close()


@pytest.mark.parametrize("int16", [False, True])
def test_host_pipeline_equals_the_direct_call(int16):
    from adapted_amd import lib
    from adapted_amd.pipeline import HostPipeline

    spc = R.spc_of()
    m = R.M
    sig, lens = R.batch("main")
    n, mb = R.N_MAIN, 24
    if int16:
        rng = np.random.default_rng(8)
        scale = rng.uniform(0.14, 0.2, n).astype(np.float32)
        offset = rng.uniform(-20.0, 20.0, n).astype(np.float32)
        raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
        pa = (scale[:, None] * (raw.astype(np.float32) + offset[:, None])).astype(np.float32)
        eng = lib.Engine(spc, n, m, device=0)
        direct, _ = eng.detect_llr_rows(pa, lens, n, mb, resegment=True)
        counts = eng.debug_resegment()
        eng.close()
    else:
        pa = sig
        _, direct, counts, _ = _run("main", mb)
    assert counts[2] >= 3 and ((direct["reserved_"] & lib.ROW_RESEGMENTED) != 0).sum() == counts[2]
    pipe = HostPipeline(spc, mb, m, device=0, primary="llr", int16_input=int16, group=2, resegment=True)
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


def test_adapter_front_post_pass_sees_the_final_rows():
    """the pipeline's rows with the adapter-front pass enabled are that pass applied to test 1's rows"""
    from adapted_amd import lib
    from adapted_amd.adapter_front import AdapterFrontParams, adapter_front_rows
    from adapted_amd.detect._rows import _engine
    from adapted_amd.pipeline import HostPipeline

    spc = R.spc_of()
    sig, lens = R.batch("main")
    n, mb = R.N_MAIN, 24
    _, rows1, counts, _ = _run("main", mb)
    params = AdapterFrontParams(min_adapter_len=int(spc.core.min_obs_adapter))
    want = adapter_front_rows(np.array(sig), None, np.array(rows1), params, engine=_engine(0))
    kept = (rows1["reserved_"] & lib.ROW_RESEGMENTED) != 0
    print("adapter front behind the re-segmentation: %d rows patched, %d of them re-segmented" % (want[1][:, 3].sum(), want[1][kept, 3].sum()))
    assert want[1][:, 0][kept].min() >= 0, "the pass looks at every re-segmented row (they pass)"
    pipe = HostPipeline(spc, mb, R.M, device=0, primary="llr", group=2, resegment=True)
    pipe.enable_adapter_front(params)
    out = {}

    def fill(get_buffers):
        bufs = get_buffers()
        bufs[0][:n], bufs[1][:n] = sig, lens
        yield n, 0

    pipe.run(fill, lambda k, rows, *more: out.__setitem__(k, rows.copy()))
    pipe.close()
    assert _canon(out[0]) == _canon(want[0])
    assert ((out[0]["reserved_"] & lib.ROW_RESEGMENTED) != 0).sum() == counts[2]
