"""The CNN primary over raw int16 ADC rows (adp_detect_cnn_i16, include/adapted_hip_i16.h): every kernel that touches the signal
reads the int16 samples and forms pA in registers; no float32 matrix is made.

Yardstick, never the code under test: the route the library had before -- adp_calibrate_i16 into a device float32 matrix, then
adp_detect_cnn on it with the same flags, on the same engine.  The comparison needs no tolerance: rows byte for byte (registry token
blanked, overflow open-pore lists resolved), bounds, and the counts of adp_debug_fetch(10) / (11).  Every precondition is asserted
on the yardstick route's output, so that a batch that stops exercising a branch fails loudly.

Quantisation (the recipe of the other int16 tests): rng = default_rng(8), scale ~ U(0.14, 0.2), offset ~ U(-20, 20), both float32,
raw = clip(rint(nan_to_num(sig, nan=108) / scale - offset)) as int16."""
import os

import numpy as np
import pytest

from test_gpu_cnn_fallback import _case
from test_gpu_cnn_second_opinion import _per_row
from util import row_diffs

pytestmark = pytest.mark.gpu

NONE = ()
FB = ("fallback",)
FB_SO = ("fallback", "second_opinion")
ALL = ("fallback", "second_opinion", "with_start_peak")
DEFAULT = "rna004_cnn_default"

_QUANT, _PAIRS = {}, {}


def _quantised(name):
    """one golden case quantised, once, shared and read-only -> (spc, raw int16 [n, m], scale, offset, lens)"""
    if name not in _QUANT:
        spc, sig, lens, _ = _case(name)
        n = sig.shape[0]
        rng = np.random.default_rng(8)
        scale = rng.uniform(0.14, 0.2, n).astype(np.float32)
        offset = rng.uniform(-20.0, 20.0, n).astype(np.float32)
        raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        for a in (raw, scale, offset, lens):
            a.setflags(write=False)
        _QUANT[name] = (spc, raw, scale, offset, lens)
    return _QUANT[name]


def _calibrated(raw, scale, offset, lens):
    """what adp_calibrate_i16 writes, on the host: both operations rounded to float32, NaN from the read's end on"""
    pa = (scale[:, None] * (raw.astype(np.float32) + offset[:, None])).astype(np.float32)
    m = raw.shape[1]
    for i in range(raw.shape[0]):
        pa[i, min(int(lens[i]), m):] = np.nan
    return pa


class _Dev:
    """one engine with the raw batch resident on the device, and room for the yardstick route's float32 matrix"""

    def __init__(self, spc, raw, scale, offset, lens, weights=True, profile=False):
        from adapted_amd import lib
        from adapted_amd.detect import cnn

        self.n, self.m = raw.shape
        self.eng = lib.Engine(spc, self.n, self.m, device=0)
        if weights:
            cnn.ensure_weights(self.eng, None, spc)
        if profile:
            self.eng.set_profiling(True)
        e, n, m = self.eng, self.n, self.m
        self.d_raw, self.d_len, self.d_cal, self.d_f32 = e.dev_alloc(n * m * 2 + 64), e.dev_alloc(n * 4), e.dev_alloc(2 * n * 4), e.dev_alloc(n * m * 4)
        e.h2d(self.d_raw, np.ascontiguousarray(raw))
        e.h2d(self.d_len, np.ascontiguousarray(lens, dtype=np.int32))
        e.h2d(self.d_cal, np.concatenate([scale, offset]).astype(np.float32))

    def _result(self, rows, bounds):
        e = self.eng
        return dict(rows=rows, canon=_per_row(rows), bounds=bounds.copy(), fb=e.debug_cnn_fallback(), so=e.debug_cnn_second_opinion(),
                    kernels=[k for k, _ in e.kernel_times()])

    def yardstick(self, mb, flags):
        e, n = self.eng, self.n
        e.calibrate_i16(self.d_raw, self.d_len, self.d_cal, self.d_cal + n * 4, n, self.d_f32)
        rows, bounds = e.detect_cnn_rows(self.d_f32, self.d_len, n, mb, device_ptrs=True, **{f: True for f in flags})
        return self._result(rows, bounds)

    def native(self, mb, flags, **kw):
        e, n = self.eng, self.n
        rows, bounds = e.detect_cnn_rows_i16(self.d_raw, self.d_len, self.d_cal, self.d_cal + n * 4, n, mb, **{f: True for f in flags}, **kw)
        return self._result(rows, bounds) if rows is not None else bounds

    def close(self):
        for p in (self.d_raw, self.d_len, self.d_cal, self.d_f32):
            self.eng.dev_free(p)
        self.eng.close()


def _assert_same(got, want, what):
    assert got["canon"][1] == want["canon"][1], (what, "overflow open-pore lists differ")
    bad = [i for i, (a, b) in enumerate(zip(got["canon"][0], want["canon"][0])) if a != b]
    if bad:
        g, w = got["rows"], want["rows"]
        i = bad[0]
        fields = [f for f in g.dtype.names if f != "open_pores_more" and g[i][f].tobytes() != w[i][f].tobytes()]
        raise AssertionError((what, "rows differ at reads", bad[:20], "read %d: fields %s" % (i, fields),
                              [(int(g[j]["success"]), int(g[j]["fail_code"]), int(w[j]["success"]), int(w[j]["fail_code"])) for j in bad[:5]]))
    assert np.array_equal(got["bounds"], want["bounds"]), (what, "bounds differ")
    assert got["fb"] == want["fb"] and got["so"] == want["so"], (what, "debug counts", got["fb"], want["fb"], got["so"], want["so"])


def _pair(name, flags, mb, lens=None, pick=None, profile=False):
    """both routes on one engine, compared -> (yardstick result, native result); cached for the unedited cases"""
    key = (name, flags, mb)
    if lens is None and not profile and key in _PAIRS:
        return _PAIRS[key]
    spc, raw, scale, offset, lens0 = _quantised(name)
    if pick is not None:
        raw, scale, offset, lens0 = raw[pick], scale[pick], offset[pick], lens0[pick]
    dev = _Dev(spc, raw, scale, offset, lens0 if lens is None else lens, profile=profile)
    want = dev.yardstick(mb, flags)
    got = dev.native(mb, flags)
    dev.close()
    print("%s %s minibatch %d: fallback %s, second opinion %s, pass %d of %d" % (name, flags, mb, want["fb"], want["so"],
                                                                               int(want["rows"]["success"].sum()), want["rows"].size))
    _assert_same(got, want, (name, flags, mb))
    if lens is None and not profile:
        _PAIRS[key] = (want, got)
    return want, got


def _exceptions(rows):
    return (rows["fail_code"] >= 9) & (rows["fail_code"] <= 14)


# ---- 1. every phase, default window
@pytest.mark.parametrize("mb", [48, 24])
@pytest.mark.parametrize("flags", [NONE, FB, FB_SO, ALL], ids=["plain", "fallback", "second", "start_peak"])
def test_every_phase_equals_calibrate_then_detect(flags, mb, oracle_mod):
    """(on the CPU oracle with exactly this quantisation, whole batch: 7 selected by the fallback, 11 rescued, 11 fail both ways, 26
    pass, 3 exception rows, 19 short reads.  The CNN path's candidates are grouped over the flattened minibatch, so at a minibatch of
    24 other reads may be left to the later phases: the counted preconditions hold for the whole batch, where they were checked, and
    at 24 every phase must still have work)"""
    from adapted_amd import lib

    spc, raw, scale, offset, lens = _quantised(DEFAULT)
    n, m = raw.shape
    assert (n, m) == (48, 17500)
    want, got = _pair(DEFAULT, flags, mb)
    w = want["rows"]
    sel, rep_, both, ok = (5, 8, 3, 20) if mb == 48 else (1, 1, 1, 10)
    assert (lens < m).sum() >= 10, "precondition: reads shorter than the window"
    if "fallback" in flags:
        assert _exceptions(w).sum() >= (2 if mb == 48 else 1), "precondition: exception rows (the fallback's chain makes them)"
        assert want["fb"][0] >= sel, ("precondition: reads selected by the fallback", want["fb"])
    else:
        assert want["fb"] == (0, 0, 0)
    if "second_opinion" in flags:
        assert want["so"][1] >= rep_, ("precondition: rows replaced by the second opinion", want["so"])
        assert (w["reserved_"] & lib.ROW_FROM_SECOND_LLR).sum() == want["so"][1]
        assert (w["success"] == 0).sum() >= both, "precondition: reads failing both ways"
        assert ((w["success"] == 1) & (w["reserved_"] == 0)).sum() >= ok, "precondition: reads the CNN path passes"
    else:
        assert want["so"] == (0, 0, 0, 0)
        assert (w["success"] == 1).sum() >= ok, "precondition: passing reads"
    if "with_start_peak" in flags:
        bit = np.uint64(lib.COLS.index("start_peak_idx"))
        assert ((w["present"] >> bit) & np.uint64(1)).sum() >= 30, "precondition: rows with the start-peak columns"
    if flags == FB:
        # the native rows against the CPU oracle on the calibrated signals, as the golden CNN tests compare (the device's predictions given)
        pa = _calibrated(raw, scale, offset, lens)
        ref = oracle_mod.detect_cnn_from_preds(pa, lens, got["bounds"], spc)
        res = lib.rows_to_results(got["rows"].copy(), "cnn")
        bad = [(i, d) for i, (g, r) in enumerate(zip(res, ref)) for d in row_diffs(g, {k: v for k, v in r.items() if not k.startswith("_")}, float_rel=1e-5)]
        assert not bad, bad[:10]


# ---- 2. the 200 k shapes
def test_the_200k_window(oracle_mod):
    """the wide shape of the shared sweeps (m > 32768) and the series pipeline over long slices, all three options"""
    spc, raw, _, _, _ = _quantised("rna004_cnn_200k")
    assert raw.shape == (12, 201500) and spc.cnn_boundaries.polya_cand_k > 1
    want, got = _pair("rna004_cnn_200k", ALL, 12, profile=True)
    assert want["fb"][0] >= 1, ("precondition: a read takes the fallback", want["fb"])
    for k in ("k_cnn_pool", "k_mvs_series_wave", "k_cand_stats", "k_validate", "k_partition_stats"):
        assert k in got["kernels"], (k, got["kernels"])
    assert "k_calibrate_i16" not in " ".join(got["kernels"])


# ---- 3. k
@pytest.mark.parametrize("name", ["rna004_cnn_k1", "rna004_cnn_k3"])
def test_one_and_three_candidates(name):
    spc, raw, _, _, _ = _quantised(name)
    assert spc.cnn_boundaries.polya_cand_k == (1 if name.endswith("k1") else 3)
    want, _ = _pair(name, FB, raw.shape[0])
    assert (want["rows"]["success"] == 1).sum() >= 3 and (want["rows"]["success"] == 0).sum() >= 1, "precondition: rows of both outcomes"


# ---- 4. forms
@pytest.mark.parametrize("form", ["groups", "out_device", "sp_unfused", "series_wave"])
def test_forms_equal_the_plain_native_call(form, monkeypatch):
    from adapted_amd import lib

    for v in ("ADP_CNN_GROUPS", "ADP_CNN_LANES", "ADP_SP_FUSED", "ADP_SERIES_PIPE"):
        monkeypatch.delenv(v, raising=False)
    _, plain = _pair(DEFAULT, ALL, 24)
    spc, raw, scale, offset, lens = _quantised(DEFAULT)
    n = raw.shape[0]
    env = {"groups": ("ADP_CNN_GROUPS", "2"), "sp_unfused": ("ADP_SP_FUSED", "0"), "series_wave": ("ADP_SERIES_PIPE", "0")}
    if form in env:
        monkeypatch.setenv(*env[form])
    dev = _Dev(spc, raw, scale, offset, lens, profile=True)
    if form == "out_device":
        drows = dev.eng.dev_alloc(n * lib.ROW_DTYPE.itemsize)
        bounds = dev.native(24, ALL, rows_dev=drows)
        rows = lib.empty_rows(n)
        dev.eng.d2h(rows, drows)
        dev.eng.dev_free(drows)
        got = dev._result(dev.eng.attach_open_pores(rows), bounds)
    else:
        got = dev.native(24, ALL)
    dev.close()
    _assert_same(got, plain, form)
    if form == "sp_unfused":
        assert "k_start_peak" in got["kernels"] and "k_sp_head" not in got["kernels"]
    if form == "series_wave" or form == "out_device":
        assert ("k_sp_head" in got["kernels"]) and "k_start_peak" not in got["kernels"]


# ---- 5. read ends
def test_read_ends_at_every_vector_tail():
    """full_len on both sides of the 4-sample vectors, of a pooled block's end, at the window and beyond it: the samples behind a
    read's end are there in the raw matrix and must read as NaN"""
    spc, raw, _, _, _ = _quantised(DEFAULT)
    m = raw.shape[1]
    lens = np.array([1000, 1001, 1003, 4097, 4098, 4099, m, m + 5], dtype=np.int32)
    want, _ = _pair(DEFAULT, ALL, 8, lens=lens, pick=np.arange(8))
    assert want["rows"].size == 8


# ---- 6. refusals
def test_refusals_leave_the_handle_usable():
    from adapted_amd import lib
    from adapted_amd.detect import cnn

    INVALID, UNSUPPORTED = -1, lib.ADP_ERR_UNSUPPORTED
    _, plain = _pair(DEFAULT, ALL, 24)
    spc, raw, scale, offset, lens = _quantised(DEFAULT)
    n, m = raw.shape
    dev = _Dev(spc, raw, scale, offset, lens, weights=False)
    e = dev.eng
    rows = lib.empty_rows(n)

    def call(flags, h=None, mm=m):
        return e.lib.adp_detect_cnn_i16(h or e._h, dev.d_raw, dev.d_len, dev.d_cal, dev.d_cal + n * 4, n, mm, 24, flags, rows, None)

    assert call(lib.ADP_IN_DEVICE) == INVALID and b"adp_cnn_set_weights" in e.lib.adp_last_error()
    cnn.ensure_weights(e, None, spc)
    assert call(0) == INVALID, "host pointers are refused"
    assert call(lib.ADP_IN_DEVICE | lib.ADP_FLAG_TRUNCATED) == UNSUPPORTED
    assert e.lib.adp_set_layout(e._h, 1) == 0
    assert call(lib.ADP_IN_DEVICE) == UNSUPPORTED
    assert e.lib.adp_set_layout(e._h, 0) == 0
    assert e.lib.adp_detect_cnn_i16(e._h, None, dev.d_len, dev.d_cal, dev.d_cal, n, m, 24, lib.ADP_IN_DEVICE, rows, None) == INVALID
    odd = lib.Engine(spc, 4, 17503, device=0)  # (a window that is no multiple of 4: refused before anything reads the buffers)
    cnn.ensure_weights(odd, None, spc)
    assert odd.lib.adp_detect_cnn_i16(odd._h, dev.d_raw, dev.d_len, dev.d_cal, dev.d_cal + n * 4, 4, 17503, 4, lib.ADP_IN_DEVICE, rows, None) == UNSUPPORTED
    odd.close()
    assert rows.tobytes() == lib.empty_rows(n).tobytes(), "a refused call writes no row"
    got = dev.native(24, ALL)
    dev.close()
    _assert_same(got, plain, "the good call behind the refusals")


# ---- 7. one engine, alternating calls
def test_alternating_calls_share_the_workspace():
    spc, raw, scale, offset, lens = _quantised(DEFAULT)
    n = raw.shape[0]
    want_f32, want_i16 = _pair(DEFAULT, ALL, 24)
    fresh = _Dev(spc, raw, scale, offset, lens, weights=False)
    llr_fresh, mbs_fresh = fresh.eng.detect_llr_rows_i16(fresh.d_raw, fresh.d_len, fresh.d_cal, fresh.d_cal + n * 4, n, 24, with_start_peak=True)
    fresh.close()
    dev = _Dev(spc, raw, scale, offset, lens)
    a = dev.yardstick(24, ALL)
    b = dev.native(24, ALL)
    llr, mbs = dev.eng.detect_llr_rows_i16(dev.d_raw, dev.d_len, dev.d_cal, dev.d_cal + n * 4, n, 24, with_start_peak=True)
    c = dev.native(24, ALL)
    dev.close()
    _assert_same(a, want_f32, "detect_cnn_rows first")
    _assert_same(b, want_i16, "detect_cnn_rows_i16 behind it")
    assert _per_row(llr) == _per_row(llr_fresh) and np.array_equal(mbs, mbs_fresh), "detect_llr_rows_i16 in between"
    _assert_same(c, want_i16, "detect_cnn_rows_i16 behind the LLR call")


# ---- 8. layers
@pytest.mark.parametrize("ragged", [False, True])
def test_host_pipeline_takes_the_native_route(ragged, tmp_path):
    from adapted_amd.io_utils import yield_minibatches_packed
    from adapted_amd.pipeline import HostPipeline

    spc, raw, scale, offset, lens = _quantised(DEFAULT)
    n, m = raw.shape
    _, direct = _pair(DEFAULT, ALL, 24)
    pipe = HostPipeline(spc, 24, m, device=0, primary="cnn", with_start_peak=True, int16_input="native", group=2, ragged=ragged,
                        second_opinion="llr")
    assert pipe.native_i16
    assert (pipe.dsig16 is not None) if ragged else (pipe.dsig16 is None)
    out = []
    if ragged:
        ids = np.array(["read_%04d" % i for i in range(n)], dtype=object)
        np.savez(tmp_path / "raw_0.npz", raw=raw, scale=scale, offset=offset, full_lengths=lens, read_ids=ids)

        def fill(get_buffers):
            for k, idv in yield_minibatches_packed([str(tmp_path / "raw_0.npz")], set(), set(), 48, m, get_buffers, int16=True):
                yield k, idv.copy()
    else:
        def fill(get_buffers):
            bufs = get_buffers()
            bufs[0][:n], bufs[1][:n], bufs[2][:n], bufs[3][:n] = raw, lens, scale, offset
            yield n, 0

    total = pipe.run(fill, lambda k, rows: out.append(rows.copy()))
    pipe.close()
    assert total == n and len(out) == 1
    assert _per_row(out[0]) == direct["canon"]


def test_int16_input_true_keeps_the_float32_route_for_the_cnn():
    from adapted_amd.pipeline import HostPipeline

    spc, raw, _, _, _ = _quantised(DEFAULT)
    pipe = HostPipeline(spc, 24, raw.shape[1], device=0, primary="cnn", int16_input=True, group=2)
    assert not pipe.native_i16 and pipe.dsig16 is not None
    pipe.close()


def test_cli_int16_ingest_with_the_cnn_preset(tmp_path):
    """`adapted detect -c RNA004 --int16_ingest --second_opinion llr --start_peak` on a raw bundle: the CSV files equal those the
    shared writer makes of the yardstick route's rows"""
    from adapted_amd import lib
    from adapted_amd import main as cli
    from adapted_amd.container_types import ReadResult

    spc, raw, scale, offset, lens = _quantised(DEFAULT)
    n = raw.shape[0]
    assert cli._load_spc(cli.build_parser().parse_args(["detect", "-i", "x", "-c", "RNA004"])).primary_method == "cnn"
    want, _ = _pair(DEFAULT, ALL, 24)
    ids = np.array(["read_%04d" % i for i in range(n)], dtype=object)
    np.savez(tmp_path / "raw_0.npz", raw=raw, scale=scale, offset=offset, full_lengths=lens, read_ids=ids)
    out = tmp_path / "out"
    cli.main(["detect", "-i", str(tmp_path / "raw_0.npz"), "-o", str(out), "-c", "RNA004", "--int16_ingest", "--second_opinion", "llr",
              "--start_peak", "-s", "24", "-b", "4000"])
    run = [d for d in os.listdir(out) if d.startswith("adapted_")]
    assert len(run) == 1
    res = lib.rows_to_results(want["rows"].copy(), "cnn")
    w = cli._Writer(str(tmp_path / "direct"), 4000)
    w.add([ReadResult(read_id=str(rid), success=r.success, fail_reason=r.fail_reason, detect_results=r) for rid, r in zip(ids, res)])
    w.close()
    for sub, f in (("boundaries", "detected_boundaries_0.csv"), ("failed_reads", "failed_reads_0.csv")):
        assert (out / run[0] / sub / f).read_text() == (tmp_path / "direct" / sub / f).read_text(), f
