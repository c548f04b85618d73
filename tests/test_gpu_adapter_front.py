"""The adapter-front post-pass (adp_adapter_front / adp_adapter_front_i16, include/adapted_hip_adapter_front.h; kernels:
adapted_amd/csrc/adapter_front.h) against its numpy oracle (tests/adapter_front_oracle.py): rows are compared as bytes and the side
outputs for exact equality (a NaN in `diff` equals a NaN), never with a tolerance.

The hand-made case's parameters are window 16, min_obs_adapter 64, min_shift 5, min_pA 90, min_adapter_len 32.  With them the
detector's result is below len - min_obs_adapter, so an accepted shift always leaves more than 64 > min_adapter_len samples: the
kind "an accepted shift that leaves too little adapter" cannot occur in that call.  It is driven by a second call on the same
reads with min_adapter_len 600, where the oracle holds both kinds (shifts refused for it, shifts still applied)."""
import os

import numpy as np
import pytest

import adapter_front_oracle as O

pytestmark = pytest.mark.gpu

L, W, MO = 2048, 16, 64
P = O.params(window=W, min_obs_adapter=MO, min_shift=5.0, min_pA_current=90.0, min_adapter_len=32)
SEED, N, M, LEAD_N = 11, 64, 17500, 400


def _af(p):
    from adapted_amd.adapter_front import AdapterFrontParams

    return AdapterFrontParams(p.window, p.min_obs_adapter, p.min_shift, p.min_pA_current, p.min_adapter_len)


def _read(rng, width, full_len, a0, lead_n, lead_pa):
    """a row of `width` samples: lead_pa for lead_n samples from a0 on, 80 pA elsewhere, noise of sd 2; every value a multiple of
    0.25 pA (exact through an int16 calibration of scale 0.25); NaN from full_len on"""
    x = np.full(width, 80.0)
    x[a0:a0 + lead_n] = lead_pa
    x = (np.round((x + rng.normal(0.0, 2.0, width)) * 4.0) / 4.0).astype(np.float32)
    x[full_len:] = np.nan
    return x


_HAND = {}


def _hand():
    """the 24 hand-made reads, once, shared and read-only -> (sig float32 [24, L], full lengths, rows, the kinds' read indices)"""
    if not _HAND:
        rng = np.random.default_rng(3)
        # (a0 or None, N = slice size - min_obs_adapter, samples of lead, its level)
        spec = [(0, W - 1, 0, 150.0), (0, W, 4, 150.0), (0, W + 1, 5, 150.0), (0, W + 8, 9, 150.0), (0, 2 * W, 12, 150.0),
                (0, 511, 140, 150.0), (0, 512, 100, 150.0), (0, 513, 200, 150.0), (0, 1025, 300, 150.0),
                (37, 511, 120, 150.0), (37, 512, 180, 150.0), (37, 513, 90, 150.0), (37, 1025, 610, 150.0),
                (0, 700, 150, 150.0), (0, 700, 150, 150.0), (None, 600, 130, 150.0), (0, 800, 0, 150.0), (0, 900, 250, 100.0),
                (0, 900, 250, 88.0), (0, 900, 330, 150.0), (37, 1500, 700, 150.0), (37, 1900, 60, 120.0), (0, 1300, 520, 150.0),
                (0, 700, 150, 150.0)]
        kinds = dict(value_error=0, empty=1, masked=(2, 3, 4), chunk_edges=(5, 6, 7, 8, 9, 10, 11, 12), nan=13, failing=14, no_start=15,
                     flat=16, low_current=18, ends_inside=19, no_end=23)
        sig, lens, bounds = np.zeros((len(spec), L), dtype=np.float32), [], []
        for r, (a0, n_used, lead_n, lead_pa) in enumerate(spec):
            ae = (a0 or 0) + n_used + MO
            full = L if r % 3 else min(L, ae + 40 + 7 * r)  # (some reads end inside the row: NaN behind their end)
            if r == kinds["ends_inside"]:
                full = ae - 264  # (and one inside its adapter: the slice's tail is NaN, for raw int16 rows too)
            sig[r] = _read(rng, L, full, a0 or 0, lead_n, lead_pa)
            lens.append(full)
            bounds.append((a0, ae))
        sig[kinds["nan"], 300] = np.nan
        rows = O.make_rows(bounds)
        rows["success"][kinds["failing"]] = 0
        rows["present"][kinds["no_end"]] &= ~np.uint64(1 << O.C_END)
        lens = np.asarray(lens, dtype=np.int32)
        for a in (sig, lens, rows):
            a.setflags(write=False)
        _HAND["v"] = (sig, lens, rows, kinds)
    return _HAND["v"]


def _same(got, want, what):
    """(rows, info, shift, cand, diff) twice: the rows' bytes and every side output"""
    assert got[0].tobytes() == want[0].tobytes(), (what, "rows differ at reads", [r for r in range(len(want[0])) if got[0][r].tobytes() != want[0][r].tobytes()][:10])
    for k, name in ((1, "info"), (2, "shift"), (3, "cand")):
        assert np.array_equal(got[k], want[k]), (what, name, np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[:10])
    assert got[4].dtype == want[4].dtype == np.float64 and np.array_equal(got[4], want[4], equal_nan=True), (what, "diff")


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def test_hand_made_rows_equal_the_oracle(eng):
    from adapted_amd.adapter_front import adapter_front_rows

    sig, lens, rows, kinds = _hand()
    want = O.front(sig, rows, P)
    _, info, shift, cand, diff = want
    # the preconditions, on the oracle
    assert info[:, 3].sum() >= 8, info[:, 3].sum()
    assert info[kinds["value_error"]].tolist() == [2, W, W - 1, 0]
    assert info[kinds["empty"], 0] == 0 and cand[kinds["empty"]] == -1
    assert all(info[r, 0] == 0 and cand[r] == 0 for r in kinds["masked"])
    assert all(info[r, 3] == 1 for r in kinds["chunk_edges"])
    for r in (kinds["nan"], kinds["ends_inside"]):
        assert info[r, 0] == 0 and np.isnan(diff[r]) and shift[r] == 0 and cand[r] == 0
    assert info[kinds["failing"], 0] == info[kinds["no_end"], 0] == -1
    assert info[kinds["no_start"], 3] == 1 and shift[kinds["flat"]] == 0 and info[kinds["flat"], 0] == 0
    assert shift[kinds["low_current"]] == 0 and diff[kinds["low_current"]] < -P.min_shift
    assert {int(rows["col"][r, O.C_START]) for r in np.flatnonzero(info[:, 3])} == {0, 37}
    patched = np.flatnonzero(info[:, 3])
    assert (want[0]["reserved_"][patched] == 8).all() and (np.delete(want[0]["reserved_"], patched) == 0).all()
    got = adapter_front_rows(sig, None, rows, _af(P), engine=eng)
    _same(got, want, "host rows")
    assert rows["reserved_"].max() == 0  # (the caller's rows are not written: a patched copy comes back)
    # an accepted shift that leaves too little adapter: min_adapter_len 600 on the same reads
    p2 = O.params(W, MO, 5.0, 90.0, 600)
    want2 = O.front(sig, rows, p2)
    refused = (want2[2] > 0) & (want2[1][:, 3] == 0)
    assert refused.sum() >= 2 and want2[1][:, 3].sum() >= 2 and np.array_equal(want2[2], shift)
    _same(adapter_front_rows(sig, None, rows, _af(p2), engine=eng), want2, "min_adapter_len 600")


def test_a_window_past_the_staged_history(eng):
    """window 300 > ASC_HIST: the chain's old samples come from global memory"""
    from adapted_amd.adapter_front import adapter_front_rows

    rng = np.random.default_rng(4)
    sig = np.stack([_read(rng, 4096, 4096, 0, 700, 150.0), _read(rng, 4096, 3900, 21, 1000, 150.0)])
    rows = O.make_rows([(0, 3000 + MO), (21, 3800)])
    p = O.params(300, MO, 5.0, 90.0, 32)
    want = O.front(sig, rows, p)
    assert want[1][:, 3].tolist() == [1, 1] and (np.abs(want[2] - [700, 1000]) < 150).all()
    _same(adapter_front_rows(sig, None, rows, _af(p), engine=eng), want, "window 300")


def test_host_rows_device_rows_and_raw_int16_give_the_same_bytes(eng):
    from adapted_amd import lib

    from test_gpu_cnn_i16 import _calibrated

    sig, lens, rows, kinds = _hand()
    n = rows.size
    want = O.front(sig, rows, P)
    args = _af(P).args()
    scale = np.full(n, 0.25, dtype=np.float32)
    offset = np.asarray([(-100, -60, 0, 40)[r % 4] for r in range(n)], dtype=np.float32)
    adc = np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]
    raw = adc.astype(np.int16)
    assert (raw == adc).all()
    # the float32 runs see identical samples -- but for the one NaN inside a read, which raw samples cannot carry: there that
    # read is an ordinary one, and its answer the oracle's on the calibrated matrix
    pa = _calibrated(raw, scale, offset, lens)
    differ = np.argwhere(pa.view(np.uint32) != sig.view(np.uint32))
    assert differ.tolist() == [[kinds["nan"], 300]]
    want16 = O.front(pa, rows, P)
    others = np.arange(n) != kinds["nan"]
    assert want16[0][others].tobytes() == want[0][others].tobytes() and want16[1][kinds["nan"], 3] == 1
    assert all(np.array_equal(a[others], b[others], equal_nan=True) for a, b in zip(want16[1:], want[1:]))
    d_sig, d_raw, d_len, d_cal, d_rows = (eng.dev_alloc(n * L * 4), eng.dev_alloc(n * L * 2 + 64), eng.dev_alloc(n * 4), eng.dev_alloc(2 * n * 4),
                                          eng.dev_alloc(n * lib.ROW_DTYPE.itemsize))
    try:
        eng.h2d(d_sig, sig)
        eng.h2d(d_raw, raw)
        eng.h2d(d_len, lens)
        eng.h2d(d_cal, np.concatenate([scale, offset]))
        host = np.array(rows, copy=True)
        _same((host,) + eng.adapter_front(d_sig, None, host, args, n=n, m=L), want, "device signals, host rows")
        eng.h2d(d_rows, rows)
        side = eng.adapter_front(sig, None, d_rows, args, n=n, m=L)
        back = np.zeros(n, dtype=lib.ROW_DTYPE)
        eng.d2h(back, d_rows)
        _same((back,) + side, want, "device rows in place")
        host = np.array(rows, copy=True)
        _same((host,) + eng.adapter_front_i16(d_raw, d_len, d_cal, d_cal + n * 4, host, args, n=n, m=L), want16, "raw int16, host rows")
        eng.h2d(d_rows, rows)
        side = eng.adapter_front_i16(d_raw, d_len, d_cal, d_cal + n * 4, d_rows, args, n=n, m=L)
        eng.d2h(back, d_rows)
        _same((back,) + side, want16, "raw int16, device rows in place")
    finally:
        for ptr in (d_sig, d_raw, d_len, d_cal, d_rows):
            eng.dev_free(ptr)


def test_refusals_leave_the_handle_usable(eng):
    from adapted_amd import lib

    sig, lens, rows, _ = _hand()
    host = np.array(rows[:2], copy=True)
    for kw in (dict(window=0), dict(min_obs_adapter=-1), dict(min_adapter_len=-1)):
        a = _af(P).args()
        for k, v in kw.items():
            setattr(a, k, v)
        with pytest.raises(lib.HipLibraryError, match="error -1"):
            eng.adapter_front(sig[:2].copy(), None, host, a)
    with pytest.raises(lib.HipLibraryError, match="error -4"):  # rows of a width that is no multiple of 4
        eng.adapter_front_i16(4096, 4096, 4096, 4096, host, _af(P).args(), n=2, m=L - 2)
    assert host.tobytes() == rows[:2].tobytes()
    _same((host,) + eng.adapter_front(sig[:2].copy(), None, host, _af(P).args()), O.front(sig[:2], rows[:2], P), "after the refusals")


# ---- behind real detect calls: the 64 synthetic reads of seed 11, their first 400 samples raised by 70 pA

def _llr_spc():
    from test_gpu_polya_length_cli import _spc

    spc = _spc()
    assert spc.sig_preload_size == M
    return spc


_LEAD = {}


def _lead_reads(lead=70.0):
    if lead not in _LEAD:
        from adapted_amd import synth

        sig, lens = synth.synth_batch(SEED, 0, N, M)
        sig = sig.copy()
        sig[:, :LEAD_N] += np.float32(lead)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        sig.setflags(write=False)
        lens.setflags(write=False)
        _LEAD[lead] = (sig, lens)
    return _LEAD[lead]


_LLR = {}


def _llr_rows():
    """the LLR primary's rows of the 64 reads and the oracle's answer on them, once -> (rows, want)"""
    if not _LLR:
        from adapted_amd import lib

        spc = _llr_spc()
        sig, lens = _lead_reads()
        e = lib.Engine(spc, N, M, device=0)
        try:
            rows, mbs = e.detect_llr_rows(sig, lens, N, N)
        finally:
            e.close()
        assert (mbs == 0).all()
        rows.setflags(write=False)
        _LLR["v"] = (rows, O.front(sig, rows, O.params(min_adapter_len=spc.core.min_obs_adapter)))
    return _LLR["v"]


def test_behind_the_llr_primary(eng):
    from adapted_amd.adapter_front import AdapterFrontParams, adapter_front_rows

    spc = _llr_spc()
    sig, lens = _lead_reads()
    rows, want = _llr_rows()
    info = want[1]
    print("LLR primary: passing %d, patched %d, ValueError %d, adapter_start > 0 before %d" % (
        (rows["success"] == 1).sum(), info[:, 3].sum(), (info[:, 0] == 2).sum(), ((rows["success"] == 1) & (rows["col"][:, O.C_START] > 0)).sum()))
    assert info[:, 3].sum() >= 24 and (info[:, 0] == 2).sum() >= 1
    assert ((rows["success"] == 1) & (rows["col"][:, O.C_START] > 0)).sum() >= 1
    got = adapter_front_rows(sig, None, rows, AdapterFrontParams(min_adapter_len=spc.core.min_obs_adapter), engine=eng)
    _same(got, want, "LLR primary")


def test_behind_the_cnn_primary_with_every_option(eng):
    from adapted_amd import lib
    from adapted_amd.adapter_front import AdapterFrontParams, adapter_front_rows
    from adapted_amd.config import get_chemistry_specific_config
    from adapted_amd.detect import cnn

    spc = get_chemistry_specific_config("RNA004")
    spc.update_primary_method()
    assert spc.primary_method == "cnn"
    sig, lens = _lead_reads()
    e = lib.Engine(spc, N, M, device=0)
    try:
        cnn.ensure_weights(e, None, spc)
        rows, _ = e.detect_cnn_rows(sig, lens, N, N, fallback=True, second_opinion=True, flag_truncated=True, with_start_peak=True)
    finally:
        e.close()
    p = O.params(min_adapter_len=spc.core.min_obs_adapter)
    want = O.front(sig, rows, p)
    print("CNN primary: passing %d, patched %d" % ((rows["success"] == 1).sum(), want[1][:, 3].sum()))
    assert want[1][:, 3].sum() >= 8
    got = adapter_front_rows(sig, None, rows, AdapterFrontParams(min_adapter_len=p.min_adapter_len), engine=eng)
    _same(got, want, "CNN primary")
    assert np.array_equal(got[0]["reserved_"] & 7, rows["reserved_"] & 7) and (rows["reserved_"] & 4).all()
    assert got[0]["col"][:, 22:27].tobytes() == rows["col"][:, 22:27].tobytes()  # the start-peak columns
    assert np.array_equal(got[0]["start_peak_type"], rows["start_peak_type"]) and ((rows["present"] >> np.uint64(22)) & np.uint64(1)).any()


# ---- the command line

def _files(root):
    runs = [d for d in os.listdir(root) if d.startswith("adapted_")]
    assert len(runs) == 1, runs
    out = {}
    for sub in ("boundaries", "failed_reads", "polya_length"):
        d = os.path.join(root, runs[0], sub)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            with open(os.path.join(d, f), "rb") as fh:
                out[sub + "/" + f] = fh.read()
    return out


SIX = ["adapter_start", "adapter_len", "adapter_mean", "adapter_std", "adapter_med", "adapter_mad"]


def test_cli(tmp_path):
    import pandas as pd

    from adapted_amd import lib
    from adapted_amd import main as cli
    from adapted_amd.container_types import ReadResult
    from test_gpu_cnn_i16 import _calibrated

    spc = _llr_spc()
    sig, lens = _lead_reads()
    rows, want = _llr_rows()
    ids = np.array(["read_%04d" % i for i in range(N)], dtype=object)
    cfg = str(tmp_path / "cfg.toml")
    spc.to_toml(cfg)
    np.savez(tmp_path / "reads_0.npz", signals=sig, full_lengths=lens, read_ids=ids)
    # the int16 bundle of the same reads (the recipe of tests/test_gpu_cnn_i16.py) and the float32 bundle it calibrates to
    rng = np.random.default_rng(8)
    scale, offset = rng.uniform(0.14, 0.2, N).astype(np.float32), rng.uniform(-20.0, 20.0, N).astype(np.float32)
    raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
    np.savez(tmp_path / "raw_0.npz", raw=raw, scale=scale, offset=offset, full_lengths=lens, read_ids=ids)
    np.savez(tmp_path / "cal_0.npz", signals=_calibrated(raw, scale, offset, lens), full_lengths=lens, read_ids=ids)
    out = {}
    for name, bundle, extra in (("plain", "reads_0.npz", []), ("front", "reads_0.npz", ["--adapter_front"]),
                                ("polya", "reads_0.npz", ["--adapter_front", "--polya_length", "adapter", "--adapter_nt", "60"]),
                                ("cal", "cal_0.npz", ["--adapter_front"]), ("raw", "raw_0.npz", ["--int16_ingest", "--adapter_front"])):
        cli.main(["detect", "-i", str(tmp_path / bundle), "-o", str(tmp_path / name), "--config", cfg, "-s", str(N), "-b", "4000"] + extra)
        out[name] = _files(str(tmp_path / name))
    plain, front, polya = out["plain"], out["front"], out["polya"]
    assert sorted(plain) == sorted(front) == ["boundaries/detected_boundaries_0.csv", "failed_reads/failed_reads_0.csv"]
    assert front["failed_reads/failed_reads_0.csv"] == plain["failed_reads/failed_reads_0.csv"]
    # what the shared writer makes of the oracle's rows
    for tag, rr in (("plain", rows), ("front", want[0])):
        res = lib.rows_to_results(rr.copy(), "llr")
        w = cli._Writer(str(tmp_path / ("direct_" + tag)), 4000)
        w.add([ReadResult(read_id=str(rid), success=r.success, fail_reason=r.fail_reason, detect_results=r) for rid, r in zip(ids, res)])
        w.close()
        for f in plain:
            assert out[tag][f] == (tmp_path / ("direct_" + tag) / f).read_bytes(), (tag, f)
    # line by line: unpatched reads keep their bytes, patched ones differ in the six columns only
    a, b = (v["boundaries/detected_boundaries_0.csv"].decode().splitlines() for v in (plain, front))
    assert len(a) == len(b) and a[0] == b[0]
    header = a[0].split(",")
    patched = {str(ids[r]) for r in np.flatnonzero(want[1][:, 3])}
    seen = 0
    for la, lb in zip(a[1:], b[1:]):
        rid = la.split(",")[0]
        if rid not in patched:
            assert la == lb, rid
            continue
        seen += 1
        differ = {header[k] for k, (u, v) in enumerate(zip(la.split(","), lb.split(","))) if u != v}
        assert "adapter_start" in differ and differ <= set(SIX), (rid, differ)
    assert seen == len(patched) >= 24
    # polya_length's adapter_len is the boundaries file's
    assert {f: v for f, v in polya.items() if not f.startswith("polya_length/")} == front
    bd = pd.read_csv(tmp_path / "polya" / [d for d in os.listdir(tmp_path / "polya")][0] / "boundaries" / "detected_boundaries_0.csv")
    pl = pd.read_csv(tmp_path / "polya" / [d for d in os.listdir(tmp_path / "polya")][0] / "polya_length" / "polya_length_0.csv")
    assert pl["read_id"].tolist() == bd["read_id"].tolist() and pl["adapter_len"].tolist() == bd["adapter_len"].tolist()
    assert (bd["adapter_len"] == bd["adapter_end"] - bd["adapter_start"]).all()
    # --int16_ingest on the raw bundle and the float32 route on the bundle it calibrates to
    assert out["raw"] == out["cal"]
    assert b"adapter_start" in out["raw"]["boundaries/detected_boundaries_0.csv"]
