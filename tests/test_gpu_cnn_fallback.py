"""The short-read LLR fallback of combined_detect_cnn (reference adapted/detect/combined.py:251-301) INSIDE adp_detect_cnn
(ADP_CNN_FALLBACK; adapted_amd/csrc/cnn_fallback.h): selection, the chain and the re-validation on the resident rows, merged
on the device.  Yardsticks: the reference's golden rows, and the host-applied fallback (``fallback="host"``: the code every
earlier version ran) byte for byte -- rows, overflow open-pore lists and the three debug counts."""

import numpy as np
import pytest

from test_gpu_cnn import _pure_tie
from util import load_case, load_stages, row_diffs

pytestmark = pytest.mark.gpu

CNN_CASES = ["rna004_cnn_default", "rna004_cnn_200k", "rna004_cnn_k3", "rna004_cnn_k1", "rna004_cnn_adapter_range", "rna004_cnn_no_mean_range",
             "rna004_cnn_200k_k3", "rna004_cnn_quantised", "rna004_cnn_flat", "rna004_cnn_nan_holes", "rna004_cnn_nan_polya",
             "rna004_cnn_nan_polya_overwrite"]
# reads whose golden row differs from the row in front of the fallback (CPU oracle on the reference's predictions, fallback on
# against off): what a flag that is passed but ignored would get wrong
CHANGED = {"rna004_cnn_default": [9, 13, 18, 23, 34, 37], "rna004_cnn_quantised": [6, 9, 11, 13, 18, 23, 27], "rna004_cnn_k1": [11, 20],
           "rna004_cnn_adapter_range": [6, 9, 23], "rna004_cnn_nan_polya": [9, 23], "rna004_cnn_nan_polya_overwrite": [4, 9, 23],
           "rna004_cnn_200k": [8, 9]}

_CASES = {}


def _case(name):
    """one golden case, loaded once and shared (nobody writes to it): (spc, sig, lens, golden rows)"""
    if name not in _CASES:
        _, spc, sig, lens, want = load_case(name)
        _CASES[name] = (spc, sig, lens, want)
    return _CASES[name]


def _engine(spc, n, m):
    from adapted_amd import lib
    from adapted_amd.detect import cnn

    eng = lib.Engine(spc, n, m, device=0)
    cnn.ensure_weights(eng, None, spc)
    return eng


def _canon(rows):
    """rows with the overflow lists resolved and the registry tokens blanked: comparable across calls"""
    from adapted_amd import lib

    lists = {int(i): lib._OPEN_PORES_MORE[int(rows[i]["open_pores_more"])].tolist() for i in np.flatnonzero(rows["n_open_pores"] > lib.MAX_OPEN_PORES)}
    r = rows.copy()
    r["open_pores_more"] = 0
    return r.tobytes(), lists


def _host_counts(eng, sig, lens, spc, minibatch=None):
    """what the host path does on this batch, from its own predicate and statuses: (selected, exception rows, re-validated)"""
    from adapted_amd.detect import cnn

    n = sig.shape[0]
    rows, bounds = eng.detect_cnn_rows(sig, lens, n, minibatch or n)
    if not spc.cnn_boundaries.fallback_to_llr_short_reads:
        return (0, 0, 0)
    idx = cnn._need_fallback(rows, bounds, lens, spc)
    if not idx.size:
        return (0, 0, 0)
    new_pe, status = eng.llr_refine_polya(sig[idx], lens[idx], idx.size, bounds[idx, :2])
    return (int(idx.size), int((status != 0).sum()), int(((status == 0) & (new_pe > 0)).sum()))


def _same(a, b, what):
    assert a[1] == b[1], (what, "overflow open-pore lists differ")
    if a[0] != b[0]:
        from adapted_amd import lib

        ra, rb = np.frombuffer(a[0], dtype=lib.ROW_DTYPE), np.frombuffer(b[0], dtype=lib.ROW_DTYPE)
        bad = [i for i in range(ra.size) if ra[i].tobytes() != rb[i].tobytes()]
        raise AssertionError((what, "rows differ at reads", bad[:20], [(int(ra[i]["success"]), int(ra[i]["fail_code"]), int(rb[i]["success"]), int(rb[i]["fail_code"])) for i in bad[:5]]))


def _device_vs_host(eng, sig, lens, spc, what):
    """detect_rows both ways on one engine -> (device canon, counts); asserts device == host and the debug counts"""
    from adapted_amd.detect import cnn

    want_counts = _host_counts(eng, sig, lens, spc)
    host = _canon(cnn.detect_rows(eng, sig, lens, None, spc, "hip", "host"))
    dev = _canon(cnn.detect_rows(eng, sig, lens, None, spc))
    counts = eng.debug_cnn_fallback()
    print("%s: selected / exception rows / re-validated: device %s, host %s" % (what, counts, want_counts))
    _same(dev, host, what)
    assert counts == want_counts, (what, counts, want_counts)
    return dev, counts


@pytest.mark.parametrize("name", CNN_CASES)
def test_one_call_gives_the_references_rows(name):
    """adp_detect_cnn with the flag and NO host fallback against the golden rows (the equal-height-tie excuse exactly as
    test_cnn_rows_vs_golden has it); the reads that the fallback changes must be among the compared ones"""
    from adapted_amd import lib
    from adapted_amd.detect import cnn

    spc, sig, lens, want = _case(name)
    n, m = sig.shape
    st = load_stages(name)
    eng = _engine(spc, n, m)
    wts = cnn.load_cnn_weights(spc.cnn_boundaries.model_name)
    preds = cnn.cnn_detect(sig, wts, spc.cnn_boundaries, spc.core, spc=spc, engine=eng)
    tied = {int(i) for i in np.flatnonzero((preds != st["preds"]).any(axis=1)) if _pure_tie(st, spc, preds, int(i))}
    assert not tied & set(CHANGED.get(name, [])), ("a read that the fallback changes is tie-excused", tied)
    rows, _ = eng.detect_cnn_rows(sig, lens, n, n, fallback=True)
    got = lib.rows_to_results(rows, "cnn")
    bad = [(i, d) for i, (g, w) in enumerate(zip(got, want)) if i not in tied for d in row_diffs(g, w, float_rel=1e-5)]
    assert not bad, bad[:10]
    eng.close()


@pytest.mark.parametrize("name", CNN_CASES)
def test_device_fallback_equals_host_fallback_bytes(name):
    import torch

    from adapted_amd import lib
    from adapted_amd.detect import cnn

    spc, sig, lens, _ = _case(name)
    n, m = sig.shape
    eng = _engine(spc, n, m)
    dev, counts = _device_vs_host(eng, sig, lens, spc, name)
    if name in CHANGED:
        assert counts[0] >= len(CHANGED[name]) > 0
    # a device-resident copy, both ways
    dsig = torch.from_numpy(np.ascontiguousarray(sig)).cuda()
    dlen = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    host_d = _canon(cnn.detect_rows_device(eng, dsig.data_ptr(), dlen.data_ptr(), n, lens, None, spc, None, "host"))
    dev_d = _canon(cnn.detect_rows_device(eng, dsig.data_ptr(), dlen.data_ptr(), n, lens, None, spc))
    assert eng.debug_cnn_fallback() == counts
    _same(dev_d, host_d, name + " (resident)")
    _same(dev_d, dev, name + " (resident against staged)")
    # rows left on the device (ADP_OUT_DEVICE) and fetched back
    drows = eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
    none, _ = eng.detect_cnn_rows(dsig.data_ptr(), dlen.data_ptr(), n, n, device_ptrs=True, rows_dev=drows, want_bounds=False, fallback=True)
    assert none is None and eng.debug_cnn_fallback() == counts
    back = np.zeros(n, dtype=lib.ROW_DTYPE)
    eng.d2h(back, drows)
    eng.dev_free(drows)
    _same(_canon(eng.attach_open_pores(back)), dev, name + " (rows on the device)")
    eng.close()


@pytest.mark.parametrize("name", ["rna004_cnn_k3", "rna004_cnn_default"])
def test_flag_without_the_configurations_consent_changes_nothing(name):
    import copy

    spc, sig, lens, _ = _case(name)
    spc = copy.deepcopy(spc)
    spc.cnn_boundaries.fallback_to_llr_short_reads = False
    n, m = sig.shape
    eng = _engine(spc, n, m)
    plain, b0 = eng.detect_cnn_rows(sig, lens, n, n)
    flagged, b1 = eng.detect_cnn_rows(sig, lens, n, n, fallback=True)
    assert eng.debug_cnn_fallback() == (0, 0, 0)
    assert np.array_equal(b0, b1)
    _same(_canon(flagged), _canon(plain), name)
    eng.close()


def test_predictions_are_those_in_front_of_the_fallback():
    """bounds_out stays what cnn_detect returned"""
    spc, sig, lens, _ = _case("rna004_cnn_default")
    n, m = sig.shape
    eng = _engine(spc, n, m)
    _, b0 = eng.detect_cnn_rows(sig, lens, n, n)
    _, b1 = eng.detect_cnn_rows(sig, lens, n, n, fallback=True)
    assert eng.debug_cnn_fallback()[0] > 0 and np.array_equal(b0, b1)
    eng.close()


# Read 13 of rna004_cnn_default is selected and re-validated; read 9 is short and has no peak of its own (predictions (1030, 0, ...)):
# it is selected only where the reference's row-compaction quirk (cnn.py:150-158: the candidates of the i-th read WITH peaks go to
# row i) hands it another read's candidates, and then raises (empty trace); read 0 is full-length: never selected.  So a batch in
# which ALL reads are selected consists of reads with peaks: copies of read 13.  In 13 / 0 / 9 / 0 x 32 + 13 / 0 the 98 reads with
# peaks fill rows 0..97, and the short reads among those rows -- the even ones, 49 -- are selected: re-validated rows, exception rows
# and untouched rows interleaved over three waves of the selection kernel.
# pattern -> (reads, selected, exception rows, re-validated; None: both kinds, more than one of each)
_PATTERNS = {
    "one_selected": ([13], 1, 0, 1),
    "64_all_selected": ([13] * 64, 64, 0, 64),
    "65_all_selected": ([13] * 65, 65, 0, 65),
    "130_alternating": ([13, 0, 9, 0] * 32 + [13, 0], 49, None, None),
    "130_last_selected": ([0] * 129 + [13], 1, 0, 1),
    "130_none_selected": ([0] * 130, 0, 0, 0),
}


@pytest.mark.parametrize("pattern", list(_PATTERNS))
def test_compaction_edges(pattern):
    """batches around the wave size assembled from three reads; the yardstick is the host path on the same batch (predictions
    inside a replicated minibatch may differ from the golden ones in their lower candidates)"""
    spc, sig, lens, _ = _case("rna004_cnn_default")
    pick, n_sel, n_exc, n_redo = _PATTERNS[pattern]
    bs, bl = np.ascontiguousarray(sig[pick]), np.ascontiguousarray(lens[pick])
    eng = _engine(spc, len(pick), sig.shape[1])
    got = _host_counts(eng, bs, bl, spc)
    assert got[0] == n_sel, ("precondition: the pattern selects %d reads" % n_sel, got)
    if n_exc is None:
        assert got[1] > 1 and got[2] > 1, ("precondition: exception rows and re-validated rows", got)
    else:
        assert got[1:] == (n_exc, n_redo), ("precondition", got)
    _device_vs_host(eng, bs, bl, spc, pattern)
    eng.close()


def _rows_device(spc, sig, lens, minibatch, fallback):
    import torch

    from adapted_amd.detect import cnn

    n, m = sig.shape
    eng = _engine(spc, n, m)
    dsig = torch.from_numpy(np.ascontiguousarray(sig)).cuda()
    dlen = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    out = _canon(cnn.detect_rows_device(eng, dsig.data_ptr(), dlen.data_ptr(), n, lens, None, spc, minibatch, fallback))
    counts = eng.debug_cnn_fallback()
    eng.close()
    return out, counts


@pytest.mark.parametrize("minibatch", [16, 20])
def test_minibatches_and_lanes(minibatch, monkeypatch):
    spc, sig, lens, _ = _case("rna004_cnn_default")
    out = {}
    for lanes in (False, True):
        monkeypatch.delenv("ADP_CNN_GROUPS", raising=False)
        monkeypatch.delenv("ADP_CNN_LANES", raising=False)
        if lanes:
            monkeypatch.setenv("ADP_CNN_GROUPS", "3")
            monkeypatch.setenv("ADP_CNN_LANES", "2")
        host, hc = _rows_device(spc, sig, lens, minibatch, "host")
        dev, dc = _rows_device(spc, sig, lens, minibatch, "device")
        assert hc == (0, 0, 0)          # (the host path's library calls do not run the fallback)
        assert dc[0] > 0 and dc[1] > 0 and dc[2] > 0, dc
        _same(dev, host, "minibatch %d, lanes %s" % (minibatch, lanes))
        out[lanes] = (dev, dc)
    _same(out[True][0], out[False][0], "lanes against one stream")
    assert out[True][1] == out[False][1]


def _open_pore_read(kind):
    """read 13 of rna004_cnn_default with 250-pA samples in its adapter: (a) 20 of them from 1200 on, 25 apart -- the first pass
    fails the MVS check, the fallback succeeds with 19 open pores; (b) 250 of them from 300 on, 10 apart -- re-validated and
    failing again ("Open pore too close to boundary") with 249 open pores"""
    spc, sig, lens, _ = _case("rna004_cnn_default")
    s = np.array(sig[13:14])
    if kind == "a":
        s[0, 1200 + 25 * np.arange(20)] = 250.0
    else:
        s[0, 300:2800:10] = 250.0
    return spc, s, np.ascontiguousarray(lens[13:14])


@pytest.mark.parametrize("kind,n_open,ok", [("a", 19, True), ("b", 249, False)])
def test_open_pore_lists_of_revalidated_rows(kind, n_open, ok, oracle_mod):
    from adapted_amd import lib

    spc, s, l = _open_pore_read(kind)
    eng = _engine(spc, 1, s.shape[1])
    first, bounds = eng.detect_cnn_rows(s, l, 1, 1)
    assert tuple(bounds[0, :2]) == (2880, 9810) and first[0]["success"] == 0
    dev, counts = _device_vs_host(eng, s, l, spc, "open pores " + kind)
    assert counts == (1, 0, 1)
    rows, bounds = eng.detect_cnn_rows(s, l, 1, 1, fallback=True)
    assert rows[0]["n_open_pores"] == n_open and bool(rows[0]["success"]) == ok
    got = lib.rows_to_results(rows, "cnn")
    want = oracle_mod.detect_cnn_from_preds(s, l, bounds, spc)
    pub = {k: v for k, v in want[0].items() if not k.startswith("_")}
    assert not row_diffs(got[0], pub), row_diffs(got[0], pub)
    assert len(got[0].open_pores) == n_open
    if ok:
        assert got[0].polya_end == 3600
    else:
        assert got[0].fail_reason == "Open pore too close to boundary"
    eng.close()


def test_arena_overflow_in_the_second_phase_repeats_the_call():
    """140 copies of input (b) on a fresh engine: the first pass wants 140 x 249 = 34 860 arena entries (the initial arena holds
    65 536), both passes 69 720 -- the overflow happens in the fallback phase, and the whole call runs again on a larger arena"""
    from adapted_amd import lib
    from adapted_amd.detect import cnn

    spc, s, l = _open_pore_read("b")
    n = 140
    bs, bl = np.ascontiguousarray(np.repeat(s, n, axis=0)), np.ascontiguousarray(np.repeat(l, n))
    eng_h = _engine(spc, n, s.shape[1])
    host = _canon(cnn.detect_rows(eng_h, bs, bl, None, spc, "hip", "host"))
    eng_h.close()
    eng = _engine(spc, n, s.shape[1])  # (fresh: its arena is the initial one)
    dev = _canon(cnn.detect_rows(eng, bs, bl, None, spc))
    assert eng.debug_cnn_fallback() == (n, 0, n)
    used = np.zeros(1, dtype=np.uint64)
    eng._check(eng.lib.adp_open_pores_arena(eng._h, None, 0, used))
    print("arena entries in use: %d" % int(used[0]))
    assert int(used[0]) > 65536, int(used[0])
    assert len(dev[1]) == n and all(len(v) == 249 for v in dev[1].values())
    _same(dev, host, "arena overflow in the second phase")
    eng.close()
