"""Validation from a given adapter start (adp_validate_candidates_from, include/adapted_hip_revalidate.h; k_validate<SIG, true>,
adapted_amd/csrc/validate.h) against the real reference's rows (tests/golden/revalidate_*.npz, cases: tests/revalidate_cases.py),
and the re-validating adapter-front pass (adp_adapter_front_revalidate / _i16; kernels: adapted_amd/csrc/adapter_front_revalidate.h)
against its own composition: adp_adapter_front for the accepted reads and their starts, adp_validate_candidates_from for their
rows, the merge rule in numpy.  Golden rows are compared field by field without a tolerance (tests/util.py's row_diffs, as
tests/test_oracle_golden.py compares), rows of the pass as bytes."""
import os

import numpy as np
import pytest

import revalidate_cases as R
from util import load_case, row_diffs

pytestmark = pytest.mark.gpu

M, N_MAX = R.M, 64
W, MO = 16, 64  # the detector's window and min_obs_adapter in these tests
C_START, C_POLYA_END, C_SP0, C_PRIM_AE, C_PRIM_PE = 2, 10, 22, 28, 29


def _spc(chem):
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config(chem)
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


@pytest.fixture(scope="module")
def engines():
    from adapted_amd import lib

    made = {chem: lib.Engine(_spc(chem), N_MAX, M, device=0) for chem in R.CHEMS}
    yield made
    for e in made.values():
        e.close()


def _golden_diffs(rows, want, primary):
    from adapted_amd import lib

    got = lib.rows_to_results(rows.copy(), primary)
    return [(R.NAMES[i], d) for i, (g, w) in enumerate(zip(got, want)) for d in row_diffs(g, w)]


# ---- 1: adp_validate_candidates_from against the reference
@pytest.mark.parametrize("chem", R.CHEMS)
def test_validate_from_equals_the_reference(engines, chem):
    eng, spc = engines[chem], _spc(chem)
    sigs, bounds, starts, lens, want, _ = R.load(chem)
    X, n = R.padded(sigs), len(sigs)
    rows = eng.validate_rows_from(X, lens, n, bounds, starts)
    bad = _golden_diffs(rows, want, spc.primary_method)
    assert not bad, bad[:8]
    # device signals, host bounds and starts
    d_sig, d_len = eng.dev_alloc(X.nbytes), eng.dev_alloc(lens.nbytes)
    try:
        eng.h2d(d_sig, X)
        eng.h2d(d_len, lens)
        rows_d = eng.validate_rows_from(d_sig, d_len, n, bounds, starts, device_ptrs=True)
    finally:
        eng.dev_free(d_sig)
        eng.dev_free(d_len)
    bad = _golden_diffs(rows_d, want, spc.primary_method)
    assert not bad, bad[:8]
    big = rows["n_open_pores"] > 16
    assert big.sum() >= 2  # (their open_pores_more are registry tokens: one per call)
    a, b = rows.copy(), rows_d.copy()
    a["open_pores_more"][big] = b["open_pores_more"][big] = 0
    assert a.tobytes() == b.tobytes()


def test_starts_outside_the_row_give_the_defined_row(engines):
    """A start outside [0, min(adapter_end, S)) of a read with an adapter end: the row of a read without an adapter, partitions from
    start 0.  Without an adapter end a negative start counts as 0, any other only names the (empty) adapter partition's start.
    Nothing is read outside a row: the starts reach far beyond it on both sides."""
    eng = engines["RNA004"]
    sigs, bounds, _, lens, _, _ = R.load("RNA004")
    x, fl, A = sigs[0], int(lens[0]), int(bounds[0, 0])
    starts = np.array([-1, -(1 << 40), A, fl + 7, 1 << 40, -1, -(1 << 40), 0, 77, 1 << 40], dtype=np.int64)
    n = starts.size
    b = np.repeat(bounds[:1], n, axis=0)
    b[5:, 0] = 0
    X, L = R.padded([x] * n), np.full(n, fl, dtype=np.int32)
    rows = eng.validate_rows_from(X, L, n, b, starts)
    assert (rows["success"] == 0).all() and (rows["fail_code"] == 1).all() and (rows["n_open_pores"] == -1).all()
    assert rows["col"][:, C_START].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 77, float(1 << 40)]
    plain = eng.validate_rows(X, L, n, b)
    assert rows[5:8].tobytes() == plain[5:8].tobytes()  # (no adapter end, start <= 0: the validation there was)
    # a bad start and a missing adapter end differ in nothing but the adapter end the row reports and the partitions around it
    assert ((rows["present"][:5] >> np.uint64(C_START + 3)) & np.uint64(1)).all()  # (the adapter's statistics from start 0)
    assert ((rows["present"][5:] >> np.uint64(C_START + 3)) & np.uint64(1) == 0).all()


# ---- 2: no starts, and starts of 0, are adp_validate_candidates
def _no_tokens(rows):
    out = rows.copy()
    out["open_pores_more"][out["n_open_pores"] > 16] = 0
    return out.tobytes()


@pytest.mark.parametrize("name,k", [("rna004_cnn_k3", 3), ("rna004_llr_open_pores", 1)])
def test_start_0_is_the_validation_there_was(name, k):
    from adapted_amd import lib

    case, spc, sig, lens, grows = load_case(name)
    n, p = len(lens), spc.primary_method
    bounds = np.zeros((n, 1 + k), dtype=np.int64)
    for r, g in enumerate(grows):
        bounds[r, 0] = g.get(p + "_adapter_end") or 0
        c = g.get("polya_candidates") or [g.get(p + "_polya_end") or 0]
        bounds[r, 1:1 + min(k, len(c))] = c[:k]
    assert (bounds[:, 0] > 0).sum() >= n // 2
    eng = lib.Engine(spc, n, sig.shape[1], device=0)
    try:
        want = eng.validate_rows(sig, lens, n, bounds)
        none = eng.validate_rows_from(sig, lens, n, bounds, None)
        zero = eng.validate_rows_from(sig, lens, n, bounds, np.zeros(n, dtype=np.int64))
    finally:
        eng.close()
    assert (want["success"] == 1).sum() >= 4
    assert _no_tokens(none) == _no_tokens(want)
    assert _no_tokens(zero) == _no_tokens(want), [r for r in range(n) if _no_tokens(zero[r:r + 1]) != _no_tokens(want[r:r + 1])][:10]


# ---- 3: the public single-read validator
@pytest.mark.parametrize("chem", R.CHEMS)
def test_public_validate_boundaries_takes_the_start(chem):
    from adapted_amd.container_types import Boundaries
    from adapted_amd.detect.combined import validate_boundaries

    spc = _spc(chem)
    sigs, bounds, starts, lens, want, _ = R.load(chem)
    bad = []
    for i in range(len(sigs)):
        b = Boundaries(adapter_start=int(starts[i]), adapter_end=int(bounds[i, 0]), polya_end=int(bounds[i, 1]),
                       polya_end_topk=[int(t) for t in bounds[i, 1:]])
        got = validate_boundaries(sigs[i], b, spc, int(lens[i]))
        bad += [(R.NAMES[i], d) for d in row_diffs(got, want[i])]
    assert not bad, bad[:8]


# ---- 4-6: the re-validating pass against its composition
def _front_params(spc):
    from adapted_amd.adapter_front import AdapterFrontParams

    return AdapterFrontParams(W, MO, 20.0, 90.0, int(spc.core.min_obs_adapter))


def _bounds_of_rows(rows, truncated):
    """the bounds the pass reads back from rows: the primary adapter end and the candidates (the row's polya_end for a truncated row)"""
    n = rows.size
    if truncated:
        return np.stack([rows["col"][:, C_PRIM_AE], rows["col"][:, C_POLYA_END]], axis=1).astype(np.int64)
    b = np.zeros((n, 1 + rows["n_cand"].max()), dtype=np.int64)
    b[:, 0] = rows["col"][:, C_PRIM_AE]
    for r in range(n):
        assert rows["n_cand"][r] > 0
        b[r, 1:1 + rows["n_cand"][r]] = rows["cand"][r, :rows["n_cand"][r]]
    return b


def _merge(old, new):
    """the pass's merge rule for one passing re-validated row"""
    out = new.copy()
    keep = np.uint64((1 << C_PRIM_PE) | (31 << C_SP0))
    out["col"][C_PRIM_PE] = old["col"][C_PRIM_PE]
    out["col"][C_SP0:C_SP0 + 5] = old["col"][C_SP0:C_SP0 + 5]
    out["present"] = (new["present"] & ~keep) | (old["present"] & keep)
    out["start_peak_type"], out["n_cand"], out["cand"] = old["start_peak_type"], old["n_cand"], old["cand"]
    out["reserved_"] = (old["reserved_"] & 7) | 8 | 16
    return out


def _composition(eng, sig, lens, rows, params):
    """-> (expected rows, info, shift, cand, diff, reval) from adapter_front on a copy, validate_rows_from and the merge rule"""
    n = rows.size
    plain = rows.copy()
    info, shift, cand, diff = eng.adapter_front(sig, None, plain, params.args())
    info = info.copy()
    acc = np.flatnonzero(info[:, 3] == 1)
    a0 = np.where((rows["present"] >> np.uint64(C_START)) & np.uint64(1), rows["col"][:, C_START], 0).astype(np.int64)
    starts = a0 + shift
    assert np.array_equal(plain["col"][acc, C_START], starts[acc])
    want, reval = rows.copy(), np.zeros((n, 2), dtype=np.int32)
    reval[:, 0] = -1
    trunc = (rows["reserved_"] & 2) != 0
    for group in (acc[~trunc[acc]], acc[trunc[acc]]):
        if not group.size:
            continue
        t = bool(trunc[group[0]])
        v = eng.validate_rows_from(np.ascontiguousarray(sig[group]), np.ascontiguousarray(lens[group]), group.size,
                                   _bounds_of_rows(rows[group], t), starts[group], polya_truncated=t)
        for j, r in enumerate(group):
            ok = int(v["success"][j]) == 1
            reval[r] = (1, 0) if ok else (0, int(v["fail_code"][j]))
            if ok:
                want[r] = _merge(rows[r], v[j])
    info[:, 3] = reval[:, 0] == 1
    return want, info, shift, cand, diff, reval


def _same_pass(got, want, what):
    for k, name in ((1, "info"), (2, "shift"), (3, "cand"), (5, "reval")):
        assert np.array_equal(got[k], want[k]), (what, name, np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[:10])
    assert np.array_equal(got[4], want[4], equal_nan=True), (what, "diff")
    assert _no_tokens(got[0]) == _no_tokens(want[0]), (what, "rows differ at reads", [r for r in range(len(want[0])) if _no_tokens(got[0][r:r + 1]) != _no_tokens(want[0][r:r + 1])][:10])


def test_pass_equals_its_composition(engines):
    eng, spc = engines["RNA004"], _spc("RNA004")
    sig, lens, bounds, kinds = R.front_batch()
    n = lens.size
    rows = eng.validate_rows(sig, lens, n, bounds)
    rows.setflags(write=False)
    params = _front_params(spc)
    want = _composition(eng, sig, lens, rows, params)
    reval = want[5]
    # the batch holds every kind
    kept, rejected, not_accepted = (np.flatnonzero(reval[:, 0] == v) for v in (1, 0, -1))
    print("re-validated and kept %d, rejected %d (codes %s), not accepted %d" % (kept.size, rejected.size, sorted(set(reval[rejected, 1].tolist())), not_accepted.size))
    assert kept.size >= 6 and rejected.size >= 6 and not_accepted.size >= 12
    assert set(kept) <= set(kinds["kept"]) | set(kinds["rejected"]) and set(rejected) <= set(kinds["rejected"])
    assert (rows["success"][kinds["failing"]] == 0).all() and (reval[kinds["failing"], 0] == -1).all() and (reval[kinds["untouched"], 0] == -1).all()
    assert (reval[rejected, 1] == 2).all()  # "adapter MAD check failed"
    assert (want[0]["reserved_"][kept] == 24).all() and want[0][rejected].tobytes() == rows[rejected].tobytes()
    assert want[0][not_accepted].tobytes() == rows[not_accepted].tobytes()
    assert (want[0]["col"][kept, C_START] > 300).all() and (want[0]["n_cand"][kept] == 3).all()
    # the accepted reads and their starts are the detector oracle's (tests/adapter_front_oracle.py), not only the library's own
    import adapter_front_oracle as O

    _, o_info, o_shift, o_cand, o_diff = O.front(sig, rows, O.params(W, MO, 20.0, 90.0, params.min_adapter_len))
    assert np.array_equal(o_info[:, 3] == 1, reval[:, 0] >= 0) and np.array_equal(o_info[:, :3], want[1][:, :3])
    assert np.array_equal(o_shift, want[2]) and np.array_equal(o_cand, want[3]) and np.array_equal(o_diff, want[4], equal_nan=True)
    got = rows.copy()
    side = eng.adapter_front_revalidate(sig, lens, got, params.args())
    _same_pass((got,) + side, want, "host signals")
    # device signals and lengths
    d_sig, d_len = eng.dev_alloc(sig.nbytes), eng.dev_alloc(lens.nbytes)
    try:
        eng.h2d(d_sig, sig)
        eng.h2d(d_len, lens)
        got = rows.copy()
        side = eng.adapter_front_revalidate(d_sig, d_len, got, params.args(), n=n, m=M)
    finally:
        eng.dev_free(d_sig)
        eng.dev_free(d_len)
    _same_pass((got,) + side, want, "device signals")
    # through adapter_front_rows
    from adapted_amd.adapter_front import adapter_front_rows
    import dataclasses

    out = adapter_front_rows(sig, lens, rows, dataclasses.replace(params, revalidate=True), engine=eng)
    assert len(out) == 6
    _same_pass(out, want, "adapter_front_rows")


def test_int16_form_equals_the_float32_form(engines):
    eng, spc = engines["RNA004"], _spc("RNA004")
    sig, lens, bounds, _ = R.front_batch()
    n = lens.size
    scale = np.full(n, 0.25, dtype=np.float32)
    offset = np.asarray([(-100, -60, 0, 40)[r % 4] for r in range(n)], dtype=np.float32)
    adc = np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]
    raw = adc.astype(np.int16)
    assert (raw == adc).all()
    rows = eng.validate_rows(sig, lens, n, bounds)
    params = _front_params(spc)
    d_raw, d_f32, d_len, d_cal = eng.dev_alloc(raw.nbytes + 64), eng.dev_alloc(sig.nbytes), eng.dev_alloc(lens.nbytes), eng.dev_alloc(2 * n * 4)
    try:
        eng.h2d(d_raw, raw)
        eng.h2d(d_len, lens)
        eng.h2d(d_cal, np.concatenate([scale, offset]))
        eng.calibrate_i16(d_raw, d_len, d_cal, d_cal + n * 4, n, d_f32)
        back = np.zeros_like(sig)
        eng.d2h(back, d_f32)
        assert back.view(np.uint32).tobytes() == sig.view(np.uint32).tobytes()
        f = rows.copy()
        side_f = eng.adapter_front_revalidate(d_f32, d_len, f, params.args(), n=n, m=M)
        g = rows.copy()
        side_g = eng.adapter_front_revalidate_i16(d_raw, d_len, d_cal, d_cal + n * 4, g, params.args(), n=n, m=M)
    finally:
        for ptr in (d_raw, d_f32, d_len, d_cal):
            eng.dev_free(ptr)
    assert (side_f[4][:, 0] == 1).sum() >= 6 and (side_f[4][:, 0] == 0).sum() >= 6
    _same_pass((g,) + side_g, (f,) + side_f, "raw int16 rows")


def test_truncated_rows_and_long_open_pore_lists(engines):
    """Rows with ADP_ROW_POLYA_TRUNCATED take the second group (bounds: the primary adapter end and the row's polya_end, k = 1,
    Boundaries.polya_truncated).  A first validation moves adapter_start to its last open pore, so a row it made has no pore behind
    its start and a replaced row of a real call never holds one; the arena path of the pass is driven with rows of the clean
    signal over a signal that got 21 spikes behind the trimmed start afterwards."""
    from adapted_amd import lib, synth

    eng, spc = engines["RNA004"], _spc("RNA004")
    sig0, lens0, bounds0, kinds = R.front_batch()
    take = np.asarray(kinds["kept"][:6] + kinds["untouched"][:2])
    sig, lens, bounds = sig0[take].copy(), lens0[take].copy(), bounds0[take].copy()
    n = take.size
    lens[:] = M
    rng = np.random.default_rng(5)
    for r in (0, 1, 6):  # everything behind the adapter is poly(A) up to the window's end, the read goes on behind it
        a = int(bounds[r, 0])
        sig[r, a:] = (np.round((108.0 + 2.5 * rng.standard_normal(M - a)) * 4.0) / 4.0).astype(np.float32)
        lens[r] = M + 5000
    sig[np.isnan(sig)] = 95.0
    trunc = np.array([r in (0, 1, 6) for r in range(n)])
    rows = eng.validate_rows(sig, lens, n, bounds)
    tb = np.stack([bounds[trunc, 0], np.full(trunc.sum(), M)], axis=1)
    trows = eng.validate_rows(np.ascontiguousarray(sig[trunc]), np.ascontiguousarray(lens[trunc]), int(trunc.sum()), tb, polya_truncated=True)
    assert (trows["success"] == 1).all()
    # (as k_pt_merge leaves them: the first row's candidates and primary poly(A) end, bits 1 and 2)
    for j, r in enumerate(np.flatnonzero(trunc)):
        t = trows[j].copy()
        t["n_cand"], t["cand"], t["col"][C_PRIM_PE] = rows["n_cand"][r], rows["cand"][r], rows["col"][r, C_PRIM_PE]
        t["reserved_"] = 6
        rows[r] = t
    spiked = sig.copy()
    spikes = 700 + 15 * np.arange(21)
    spiked[2, spikes] = 230.0
    params = _front_params(spc)
    want = _composition(eng, spiked, lens, rows, params)
    reval = want[5]
    assert reval[:, 0].tolist() == [1, 1, 1, 1, 1, 1, -1, -1], reval.tolist()
    assert (want[0]["reserved_"][[0, 1]] == 30).all() and (want[0]["reserved_"][[2, 3]] == 24).all() and want[0]["reserved_"][6] == 6
    assert not ((want[0]["present"][[0, 1]] >> np.uint64(16)) & np.uint64(63)).any()  # (no RNA partition)
    assert want[0]["n_open_pores"][2] == 20
    tokens_before = set(lib._OPEN_PORES_MORE)
    got = rows.copy()
    side = eng.adapter_front_revalidate(spiked, lens, got, params.args())
    _same_pass((got,) + side, want, "truncated rows and a long list")
    tok = int(got["open_pores_more"][2])
    assert tok not in tokens_before and lib._OPEN_PORES_MORE[tok].tolist() == spikes[1:].tolist()
    res = lib.rows_to_results(got[2:3].copy(), spc.primary_method)[0]
    assert res.open_pores.tolist() == spikes[1:].tolist() and res.adapter_start == spikes[-1]


def test_arena_growth_repeats_the_call_and_keeps_the_rejected_reads():
    """352 copies of a read whose trimmed adapter holds 195 open pores, on a fresh engine (its arena holds 65 536 entries): the
    re-validation wants 68 640, the call repeats on a larger arena from the rows as they came.  The eight reads whose trim the
    validation rejects are selected again in the repeat and report (0, fail_code)."""
    from adapted_amd import lib

    spc = _spc("RNA004")
    sig0, lens0, bounds0, kinds = R.front_batch()
    r_keep, r_rej, copies = 8, kinds["rejected"][0], 352
    idx = np.array([r_rej] * 4 + [r_keep] * copies + [r_rej] * 4)
    n = idx.size
    clean, lens, bounds = np.ascontiguousarray(sig0[idx]), np.ascontiguousarray(lens0[idx]), np.ascontiguousarray(bounds0[idx])
    assert (lens == M).all()
    spikes = np.arange(700, int(bounds0[r_keep, 0]) - 1100, 10)
    spiked = clean.copy()
    spiked[4:4 + copies, spikes] = 230.0
    params = _front_params(spc)
    eng = lib.Engine(spc, n, M, device=0)  # (fresh: its arena is the initial one)
    try:
        rows = eng.validate_rows(clean, lens, n, bounds)  # (rows of the clean signal: see test_truncated_rows_and_long_open_pore_lists)
        assert (rows["success"] == 1).all() and (rows["n_open_pores"] == 0).all()
        got = rows.copy()
        side = eng.adapter_front_revalidate(spiked, lens, got, params.args())
        used = np.zeros(1, dtype=np.uint64)
        eng._check(eng.lib.adp_open_pores_arena(eng._h, None, 0, used))
        print("arena entries in use: %d" % int(used[0]))
        assert int(used[0]) == copies * (spikes.size - 1) > 65536, ("precondition: more than the initial arena in use", int(used[0]))
        want = _composition(eng, spiked, lens, rows, params)
    finally:
        eng.close()
    rej = np.r_[0:4, n - 4:n]
    assert (want[5][rej, 0] == 0).all() and (want[5][rej, 1] == 2).all() and (want[5][4:4 + copies, 0] == 1).all()
    _same_pass((got,) + side, want, "after a repeat on a larger arena")
    assert got[rej].tobytes() == rows[rej].tobytes()
    for r in (4, 4 + copies // 2, 3 + copies):
        assert lib._OPEN_PORES_MORE[int(got["open_pores_more"][r])].tolist() == spikes[1:].tolist()


def test_refusals_leave_the_handle_usable(engines):
    from adapted_amd import lib

    eng, spc = engines["RNA004"], _spc("RNA004")
    sig, lens, bounds, _ = R.front_batch()
    rows = eng.validate_rows(sig, lens, lens.size, bounds)
    params = _front_params(spc)
    a = params.args()
    a.min_adapter_len = 0
    host = rows.copy()
    with pytest.raises(lib.HipLibraryError, match="error -1"):
        eng.adapter_front_revalidate(sig, lens, host, a)
    import ctypes

    info, reval = np.zeros((lens.size, 4), dtype=np.int32), np.zeros((lens.size, 2), dtype=np.int32)
    z = np.zeros(lens.size, dtype=np.int64)
    with pytest.raises(lib.HipLibraryError, match="error -4"):  # ADP_OUT_DEVICE: the re-validating forms take host rows
        eng._check(eng.lib.adp_adapter_front_revalidate(eng._h, np.ascontiguousarray(sig), lens, lens.size, M, host, ctypes.byref(params.args()),
                                                        lib.ADP_OUT_DEVICE, info, z, z.copy(), np.zeros(lens.size), reval))
    assert host.tobytes() == rows.tobytes()
    side = eng.adapter_front_revalidate(sig, lens, host, params.args())
    assert (side[4][:, 0] == 1).sum() >= 6


# ---- 7: the command line
def _run_cli(tmp_path, out, extra, ranks=1, bundle="reads_0.npz"):
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, ADAPTED_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable]
    if ranks > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % ranks, "--master-addr", "127.0.0.1", "--master-port", "29747"]
    cmd += ["-m", "adapted_amd.main", "detect", "-i", str(tmp_path / bundle), "-o", str(out), "--config", str(tmp_path / "cfg.toml"), "-s", "8",
            "-b", "4000"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from test_gpu_adapter_front import _files

    return _files(str(out)), r.stdout + r.stderr


def test_cli(tmp_path):
    from adapted_amd import lib
    from adapted_amd import main as cli
    from adapted_amd.container_types import ReadResult
    from test_gpu_adapter_front import _lead_reads, _llr_spc, M as M_CLI, N as N_CLI

    spc = _llr_spc()
    sig, lens = _lead_reads()
    ids = np.array(["read_%04d" % i for i in range(N_CLI)], dtype=object)
    spc.to_toml(str(tmp_path / "cfg.toml"))
    np.savez(tmp_path / "reads_0.npz", signals=sig, full_lengths=lens, read_ids=ids)
    extra = ["--adapter_front", "--adapter_front_revalidate", "--adapter_front_params", "%d,%d,20,90" % (W, MO)]
    one, log = _run_cli(tmp_path, tmp_path / "one", extra)
    assert "Adapter front re-validated:" in log
    # the Python composition on the rows of the same detect calls (minibatches of 8, as the run's)
    e = lib.Engine(spc, N_CLI, M_CLI, device=0)
    try:
        rows, mbs = e.detect_llr_rows(sig, lens, N_CLI, 8)
        assert (mbs == 0).all()
        import dataclasses

        want = _composition(e, sig, lens, rows, dataclasses.replace(_front_params(spc)))
    finally:
        e.close()
    kept, rejected = int((want[5][:, 0] == 1).sum()), int((want[5][:, 0] == 0).sum())
    assert kept >= 16
    assert "Adapter front re-validated: %d kept, %d trims rejected by validation" % (kept, rejected) in log
    res = lib.rows_to_results(want[0].copy(), "llr")
    w = cli._Writer(str(tmp_path / "direct"), 4000)
    w.add([ReadResult(read_id=str(rid), success=r.success, fail_reason=r.fail_reason, detect_results=r) for rid, r in zip(ids, res)])
    w.close()
    assert sorted(one) == ["boundaries/detected_boundaries_0.csv", "failed_reads/failed_reads_0.csv"]
    for f in one:
        assert one[f] == (tmp_path / "direct" / f).read_bytes(), f
    two, log2 = _run_cli(tmp_path, tmp_path / "two", extra, ranks=2)
    assert two == one
    assert "Adapter front re-validated: %d kept, %d trims rejected by validation" % (kept, rejected) in log2
