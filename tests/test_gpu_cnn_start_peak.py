"""The start-peak columns of the CNN primary inside adp_detect_cnn (ADP_WITH_START_PEAK): K1 riding the pooling pass
(k_sp_head -> k_cnn_pool<true> -> k_sp_tail) or beside the conv stack (k_start_peak), overlaid by k_sp_decorate (mode 0) on the row
the call finally delivers.

Yardsticks, never the code under test: for every byte outside the start-peak fields the same engine's call WITHOUT the flag on
the same batch, byte for byte; for the fields ``oracle.start_peak_table`` overlaid by the rule (tests/cnn_start_peak_cases.py,
checked on the CPU against the oracle's own LLR extension), compared exactly, float32 values included.  Both together are one
comparison of whole rows: the call with the flag must deliver overlay_rows(the call without it, the table)."""
import csv
import io
import os

import numpy as np
import pytest

import cnn_start_peak_cases as sc
import truncation_cases as tc
from test_gpu_cnn_fallback import _engine

pytestmark = pytest.mark.gpu

FUSED, UNFUSED = {"k_sp_head", "k_sp_tail"}, {"k_start_peak"}
_DEFAULT_FORM = {}


def _canon(rows):
    """(bytes of every row with the registry token blanked, {read: overflow open-pore list})"""
    from adapted_amd import lib

    lists = {int(i): lib._OPEN_PORES_MORE[int(rows[i]["open_pores_more"])].tolist() for i in np.flatnonzero(rows["n_open_pores"] > lib.MAX_OPEN_PORES)}
    r = rows.copy()
    r["open_pores_more"] = 0
    return [r[i].tobytes() for i in range(r.size)], lists


def _assert_rows(got, exp, what):
    g, e = _canon(got), _canon(exp)
    bad = [i for i in range(got.size) if g[0][i] != e[0][i] or g[1].get(i) != e[1].get(i)]
    if bad:
        i = bad[0]
        fields = [f for f in got.dtype.names if f != "open_pores_more" and got[i][f].tobytes() != exp[i][f].tobytes()]
        gv, ev = sc.sp_view(got[i:i + 1]), sc.sp_view(exp[i:i + 1])
        raise AssertionError((what, "rows differ from the yardstick at reads", bad[:16], "read %d: fields %s" % (i, fields),
                              "fields got %s type %s, want %s type %s" % (gv[0].tolist(), gv[1].tolist(), ev[0].tolist(), ev[1].tolist())))


def _sp_kernels(eng):
    return {n for n, _ in eng.kernel_times() if n in FUSED | UNFUSED}


def _both(eng, sig, lens, tab, mb, what, form=None, **kw):
    """the call without and with the flag on one engine, the second against the yardstick -> (plain rows, rows with the flag)"""
    n = sig.shape[0]
    eng.set_profiling(True)
    plain, b0 = eng.detect_cnn_rows(sig, lens, n, mb, **kw)
    assert not _sp_kernels(eng), "a call without the flag launches nothing of K1"
    got, b1 = eng.detect_cnn_rows(sig, lens, n, mb, with_start_peak=True, **kw)
    ran = _sp_kernels(eng)
    eng.set_profiling(False)
    assert np.array_equal(b0, b1), "bounds_out does not change"
    v, typ = sc.sp_view(plain)
    assert np.isnan(v).all() and (typ == 0).all(), "the call without the flag fills none of the fields"
    exp = sc.overlay_rows(plain, tab)
    _assert_rows(got, exp, what)
    exc = (got["fail_code"] >= 9) & (got["fail_code"] <= 14)
    v, typ = sc.sp_view(got)
    assert np.isnan(v[exc]).all() and (typ[exc] == 0).all(), "exception rows stay bare"
    if form is not None:
        assert ran == form, (what, "K1's launches", sorted(ran))
    return plain, got


def _default_form(name, oracle_mod):
    """the four inputs in the default form (one chunk, fused, host rows, the operator's fallback on), once"""
    if name not in _DEFAULT_FORM:
        spc, sig, lens = sc.inputs(name, oracle_mod)
        tab = sc.table(oracle_mod, name, sig, lens, spc)
        n, m = sig.shape
        eng = _engine(spc, n, m)
        plain, got = _both(eng, sig, lens, tab, n, name, form=FUSED, fallback=True)
        eng.close()
        _DEFAULT_FORM[name] = (plain, got)
    return _DEFAULT_FORM[name]


# ---- 1. rows
@pytest.mark.parametrize("name", ["default", "200k", "sp200k", "handmade"])
def test_rows_differ_from_the_plain_call_in_the_start_peak_fields_only(name, oracle_mod):
    """the test that fails without the feature: a flag that is accepted and ignored returns the plain rows"""
    spc, sig, lens = sc.inputs(name, oracle_mod)
    tab = sc.table(oracle_mod, name, sig, lens, spc)
    plain, got = _default_form(name, oracle_mod)
    exc = (plain["fail_code"] >= 9) & (plain["fail_code"] <= 14)
    want_filled = (tab["valid"] != 0) & ~exc & (plain["present"] != 0)
    v, typ = sc.sp_view(got)
    print("%s: %d reads, %d with the fields, %d exception rows, types %s" % (name, sig.shape[0], int(want_filled.sum()), int(exc.sum()),
                                                                             np.bincount(typ, minlength=3).tolist()))
    assert want_filled.sum() >= 10 and (~np.isnan(v[:, 0]) == want_filled).all()
    assert (np.isnan(v[:, 4]) == (typ == 0)).all(), "start_peak_open_pore_idx only when the read is flagged"
    if name in ("default", "200k"):
        assert (tab["valid"] == 0).any() and np.isnan(v[tab["valid"] == 0]).all(), "a read whose K1 result is not valid gets nothing"
    if name == "sp200k":
        assert sorted(typ.tolist()) == [0] * 19 + [2]
    if name == "handmade":
        assert all(typ[r] == 1 for r in sc.HAND_TYPE1) and all(typ[r] == 2 for r in sc.HAND_TYPE2) and all(typ[r] == 0 for r in sc.HAND_BEHIND)
    # the fail reasons do not change: the +<flag> suffix belongs to the start-peak primary alone
    from adapted_amd import lib

    a, b = lib.rows_to_results(plain, "cnn"), lib.rows_to_results(got, "cnn")
    assert [r.fail_reason for r in a] == [r.fail_reason for r in b] and [r.success for r in a] == [r.success for r in b]
    assert [r.start_peak_open_pore_type for r in b] == [sc.SP_TYPES[int(t)] for t in typ]


def test_exception_rows_with_a_start_peak_result_stay_bare(oracle_mod):
    """rna004_cnn_no_mean_range: the reference raises "pA_mean_range is not specified" for 14 of the 16 reads, 12 of them with a
    valid K1 result (the exception rows of the four inputs above all belong to reads without one)"""
    from util import load_case

    _, spc, sig, lens, want = load_case("rna004_cnn_no_mean_range")
    tab = sc.table(oracle_mod, "no_mean_range", sig, lens, spc)
    raised = np.array([w.get("fail_reason") == "pA_mean_range is not specified" for w in want])
    assert (raised & (tab["valid"] != 0)).sum() == 12 and (~raised & (tab["valid"] != 0)).sum() == 2
    n, m = sig.shape
    eng = _engine(spc, n, m)
    plain, got = _both(eng, sig, lens, tab, n, "no_mean_range", form=FUSED, fallback=True)
    eng.close()
    exc = (plain["fail_code"] >= 9) & (plain["fail_code"] <= 14)
    # (the call's own predictions may differ from the golden ones inside exact ties: the precondition is on the call's rows)
    assert (exc & (tab["valid"] != 0)).sum() >= 8 and (~exc & (tab["valid"] != 0)).any(), (exc.tolist(), raised.tolist())
    v, typ = sc.sp_view(got)
    assert np.isnan(v[exc]).all() and (typ[exc] == 0).all() and not np.isnan(v[~exc, :4]).any()
    assert _canon(got[exc])[0] == _canon(plain[exc])[0]


# ---- 2. forms
@pytest.mark.parametrize("name", ["default", "200k", "sp200k", "handmade"])
def test_side_stream_form_gives_the_same_bytes(name, oracle_mod, monkeypatch):
    spc, sig, lens = sc.inputs(name, oracle_mod)
    tab = sc.table(oracle_mod, name, sig, lens, spc)
    n, m = sig.shape
    monkeypatch.setenv("ADP_SP_FUSED", "0")
    eng = _engine(spc, n, m)
    _, got = _both(eng, sig, lens, tab, n, name + ", ADP_SP_FUSED=0", form=UNFUSED, fallback=True)
    eng.close()
    assert _canon(got) == _canon(_default_form(name, oracle_mod)[1])


def test_unequal_pooling_factors_take_the_side_stream_form(oracle_mod):
    spc0, sig, lens = sc.inputs("default")
    spc = sc.with_section(spc0, downscale_factor=7)
    tab = sc.table(oracle_mod, "default, ds 7", sig, lens, spc)
    assert tab["valid"].sum() == 42 and (tab["start_peak_idx"][tab["valid"] != 0] % 7 == 0).all()
    n, m = sig.shape
    eng = _engine(spc, n, m)
    _both(eng, sig, lens, tab, n, "rna_start_peak.downscale_factor 7", form=UNFUSED, fallback=True)
    eng.close()


def test_window_that_ends_inside_a_pooled_block(oracle_mod, monkeypatch):
    """m % ds != 0: the pooling pass's ragged last block is left to k_sp_tail (cov1 counts complete blocks only)"""
    spc, sig, lens = sc.inputs("m16003")
    tab = sc.table(oracle_mod, "m16003", sig, lens, spc)
    n, m = sig.shape
    assert m == 17503 and tab["valid"].sum() >= 40
    out = {}
    for fused in (True, False):
        monkeypatch.setenv("ADP_SP_FUSED", "1" if fused else "0")
        eng = _engine(spc, n, m)
        out[fused] = _both(eng, sig, lens, tab, n, "m 17503, fused %s" % fused, form=FUSED if fused else UNFUSED, fallback=True)[1]
        eng.close()
    assert _canon(out[True]) == _canon(out[False])


@pytest.mark.parametrize("name", ["default", "handmade"])
@pytest.mark.parametrize("fused", [True, False])
def test_groups_and_lanes_give_the_same_bytes(name, fused, oracle_mod, monkeypatch):
    """ADP_CNN_GROUPS=3 over minibatches of 16: the lanes write their slices of the owner's K1 buffer, the fallback and the second
    opinion run on the owner.  (The CNN path's own outcome depends on the minibatch: the yardstick is the one-chunk call at 16.)"""
    spc, sig, lens = sc.inputs(name, oracle_mod)
    tab = sc.table(oracle_mod, name, sig, lens, spc)
    n, m = sig.shape
    monkeypatch.setenv("ADP_SP_FUSED", "1" if fused else "0")
    out = {}
    for groups in (None, "3"):
        monkeypatch.delenv("ADP_CNN_GROUPS", raising=False)
        monkeypatch.delenv("ADP_CNN_LANES", raising=False)
        if groups:
            monkeypatch.setenv("ADP_CNN_GROUPS", groups)
            monkeypatch.setenv("ADP_CNN_LANES", "2")
        eng = _engine(spc, n, m)
        plain, got = _both(eng, sig, lens, tab, 16, "%s, groups %s" % (name, groups), form=FUSED if fused else UNFUSED, fallback=True, second_opinion=True)
        assert eng.debug_cnn_fallback()[2] > 0 and eng.debug_cnn_second_opinion()[1] > 0, "precondition: both later phases replace rows"
        out[groups] = (_canon(plain), _canon(got))
        eng.close()
    assert out[None] == out["3"]


def test_resident_input_and_device_rows_give_the_same_bytes(oracle_mod):
    import torch

    from adapted_amd import lib
    from adapted_amd.detect import cnn

    name = "handmade"
    spc, sig, lens = sc.inputs(name, oracle_mod)
    n, m = sig.shape
    want = _canon(_default_form(name, oracle_mod)[1])
    eng = _engine(spc, n, m)
    dsig = torch.from_numpy(np.ascontiguousarray(sig)).cuda()
    dlen = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    res = cnn.detect_rows_device_start_peak(eng, dsig.data_ptr(), dlen.data_ptr(), n, lens, None, spc)
    assert _canon(res) == want, "resident against staged"
    drows = eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
    none, _ = eng.detect_cnn_rows(dsig.data_ptr(), dlen.data_ptr(), n, n, device_ptrs=True, rows_dev=drows, want_bounds=False, fallback=True,
                                  with_start_peak=True)
    assert none is None
    back = np.zeros(n, dtype=lib.ROW_DTYPE)
    eng.d2h(back, drows)
    eng.dev_free(drows)
    assert _canon(eng.attach_open_pores(back)) == want, "rows on the device"
    # the operators
    assert _canon(cnn.detect_rows_start_peak(eng, sig, lens, None, spc)) == want
    out = cnn.combined_detect_cnn(sig, lens, None, spc, with_start_peak=True)
    ref = lib.rows_to_results(_default_form(name, oracle_mod)[1], "cnn")
    assert [(o.start_peak_idx, o.start_peak_pa, o.start_peak_next_max_idx, o.start_peak_next_max_pa, o.start_peak_open_pore_idx, o.start_peak_open_pore_type) for o in out] == \
           [(o.start_peak_idx, o.start_peak_pa, o.start_peak_next_max_idx, o.start_peak_next_max_pa, o.start_peak_open_pore_idx, o.start_peak_open_pore_type) for o in ref]
    assert sum(o.start_peak_open_pore_type is not None for o in out) >= len(sc.HAND_TYPE1 + sc.HAND_TYPE2)
    eng.close()


# ---- 3. phases
def test_rows_the_fallback_revalidates_carry_the_fields(oracle_mod):
    spc, sig, lens = sc.inputs("default")
    tab = sc.table(oracle_mod, "default", sig, lens, spc)
    n, m = sig.shape
    eng = _engine(spc, n, m)
    first, _ = eng.detect_cnn_rows(sig, lens, n, n)  # (in front of the fallback)
    plain, got = _default_form("default", oracle_mod)
    eng.detect_cnn_rows(sig, lens, n, n, fallback=True, with_start_peak=True)
    counts = eng.debug_cnn_fallback()
    eng.close()
    assert counts[2] > 0, counts
    fc, pc = _canon(first)[0], _canon(plain)[0]
    redone = [i for i in range(n) if fc[i] != pc[i] and not 9 <= plain[i]["fail_code"] <= 14]
    assert redone and all(tab[i]["valid"] for i in redone), ("precondition: re-validated rows with a K1 result", redone)
    v, _ = sc.sp_view(got)
    assert not np.isnan(v[redone, :4]).any()
    assert (v[redone, 0] == tab["start_peak_idx"][redone]).all() and (v[redone, 2] == tab["next_greater_idx"][redone]).all()
    made_bare = [i for i in range(n) if fc[i] != pc[i] and 9 <= plain[i]["fail_code"] <= 14]
    assert np.isnan(v[made_bare]).all()


def test_rescued_rows_carry_the_same_fields_as_in_the_plain_call(oracle_mod):
    from adapted_amd import lib

    spc, sig, lens = sc.inputs("default")
    tab = sc.table(oracle_mod, "default", sig, lens, spc)
    n, m = sig.shape
    eng = _engine(spc, n, m)
    _, got = _both(eng, sig, lens, tab, n, "second opinion", form=FUSED, fallback=True, second_opinion=True)
    counts = eng.debug_cnn_second_opinion()
    eng.close()
    rescued = np.flatnonzero(got["reserved_"] & lib.ROW_FROM_SECOND_LLR)
    assert rescued.size >= 1 and counts[1] == rescued.size, (counts, rescued)
    base = _default_form("default", oracle_mod)
    assert (base[0]["success"][rescued] == 0).all() and (got["success"][rescued] == 1).all()
    exc_before = [int(i) for i in rescued if 9 <= base[0][i]["fail_code"] <= 14]
    v, typ = sc.sp_view(got)
    keep = [int(i) for i in rescued if int(i) not in exc_before]
    vb, tb = sc.sp_view(base[1])
    assert keep and np.array_equal(v[keep], vb[keep], equal_nan=True) and np.array_equal(typ[keep], tb[keep])
    print("rescued %s (exception rows before: %s)" % (rescued.tolist(), exc_before))
    # (a read whose CNN row was an exception row had none; its LLR row has them when K1 is valid)
    assert all(not np.isnan(v[i, 0]) == bool(tab[i]["valid"]) for i in exc_before)


@pytest.mark.parametrize("second", [False, True])
def test_rows_the_truncation_look_replaces_keep_the_fields(second, oracle_mod):
    from adapted_amd import lib

    spc = tc.spc_of("cnn")
    m = spc.sig_preload_size
    sig, lens = tc.batch(m, 48, first=192 if second else 0)
    tab = sc.table(oracle_mod, ("truncation", second), sig, lens, spc)
    assert tab["valid"].sum() >= 40
    eng = _engine(spc, 48, m)
    _, got = _both(eng, sig, lens, tab, 48, "truncation look", form=FUSED, fallback=True, second_opinion=second, flag_truncated=True)
    counts = eng.debug_truncated()
    eng.close()
    replaced = np.flatnonzero(got["reserved_"] & lib.ROW_POLYA_TRUNCATED)
    assert counts[2] > 0 and replaced.size == counts[2]
    v, _ = sc.sp_view(got)
    assert tab["valid"][replaced].all() and (v[replaced, 0] == tab["start_peak_idx"][replaced]).all()
    assert (v[replaced, 1] == tab["start_peak_pa"][replaced].astype(np.float64)).all()


# ---- 4. state
def test_flag_on_off_on_leaves_nothing_behind(oracle_mod):
    name = "handmade"
    spc, sig, lens = sc.inputs(name, oracle_mod)
    n, m = sig.shape
    plain, want = _default_form(name, oracle_mod)  # (fresh engines' calls)
    eng = _engine(spc, n, m)
    a, _ = eng.detect_cnn_rows(sig, lens, n, n, fallback=True, with_start_peak=True)
    a = a.copy()
    b, _ = eng.detect_cnn_rows(sig, lens, n, n, fallback=True)
    b = b.copy()
    c, _ = eng.detect_cnn_rows(sig, lens, n, n, fallback=True, with_start_peak=True)
    fresh = _engine(spc, n, m)
    f, _ = fresh.detect_cnn_rows(sig, lens, n, n, fallback=True)
    fresh.close()
    eng.close()
    assert _canon(b) == _canon(f) == _canon(plain), "the call without the flag equals a fresh engine's"
    assert _canon(a) == _canon(c) == _canon(want)


# ---- 5. layers
@pytest.mark.parametrize("int16", [False, True])
def test_host_pipeline_equals_the_direct_call(int16, oracle_mod):
    from adapted_amd.pipeline import HostPipeline

    spc, sig, lens = sc.inputs("default")
    n, m = sig.shape
    mb = 24
    if int16:
        rng = np.random.default_rng(8)
        scale = rng.uniform(0.14, 0.2, n).astype(np.float32)
        offset = rng.uniform(-20.0, 20.0, n).astype(np.float32)
        raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
        pa = (scale[:, None] * (raw.astype(np.float32) + offset[:, None])).astype(np.float32)
        for i in range(n):  # (the on-device calibration pads with NaN from the read's end on)
            pa[i, min(int(lens[i]), m):] = np.nan
        tab = oracle_mod.start_peak_table(pa, lens, spc)
    else:
        pa = sig
        tab = sc.table(oracle_mod, "default", sig, lens, spc)
    eng = _engine(spc, n, m)
    _, direct = _both(eng, pa, lens, tab, mb, "direct, int16 %s" % int16, form=FUSED, fallback=True)
    eng.close()
    assert (~np.isnan(sc.sp_view(direct)[0][:, 0])).sum() >= 30
    pipe = HostPipeline(spc, mb, m, device=0, primary="cnn", with_start_peak=True, int16_input=int16, group=2)
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


def test_cli_writes_the_fields_with_the_cnn_preset(tmp_path, oracle_mod):
    """`adapted detect -c RNA004 --start_peak`: the CSV files equal those the shared writer makes of the direct call's results"""
    from adapted_amd import lib
    from adapted_amd import main as cli
    from adapted_amd.container_types import ReadResult

    spc, sig, lens = sc.inputs("default")
    n, m = sig.shape
    assert cli._load_spc(cli.build_parser().parse_args(["detect", "-i", "x", "-c", "RNA004"])).primary_method == "cnn"
    ids = np.array(["read_%04d" % i for i in range(n)], dtype=object)
    np.savez(tmp_path / "reads_0.npz", signals=sig, full_lengths=lens, read_ids=ids)
    out = tmp_path / "out"
    cli.main(["detect", "-i", str(tmp_path / "reads_0.npz"), "-o", str(out), "-c", "RNA004", "--start_peak", "-s", str(n), "-b", "4000"])
    run = [d for d in os.listdir(out) if d.startswith("adapted_")]
    assert len(run) == 1
    rd = out / run[0]
    res = lib.rows_to_results(_default_form("default", oracle_mod)[1], "cnn")
    assert sum(r.start_peak_idx is not None for r in res) >= 30
    w = cli._Writer(str(tmp_path / "direct"), 4000)
    w.add([ReadResult(read_id=str(rid), success=r.success, fail_reason=r.fail_reason, detect_results=r) for rid, r in zip(ids, res)])
    w.close()
    for sub, f in (("boundaries", "detected_boundaries_0.csv"), ("failed_reads", "failed_reads_0.csv")):
        text = (rd / sub / f).read_text()
        assert text == (tmp_path / "direct" / sub / f).read_text(), f
        table = list(csv.reader(io.StringIO(text)))
        header = table[0]
        assert all(c in header for c in sc.SP_COLS + ["start_peak_open_pore_type"])
        col = header.index("start_peak_idx")
        assert sum(1 for line in table[1:] if line[col] != "") >= 5, f
