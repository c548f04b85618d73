"""The packed forms of the two event calls (adp_segment_events_packed, adp_event_levels_packed: include/adapted_hip_events_packed.h)
and `adapted events` on the GPU.  The packed calls run the matrix calls' kernels on another sample source, so every comparison
with them is byte for byte, in every output; the int16 form is also held against the numpy restatements of the segmentation
and of the event tables (tests/events_oracle.py, tests/fingerprint_oracle.py) on the float32 values the calibration gives."""
import os

import numpy as np
import pytest

import events_oracle as eo
import fingerprint_oracle as fo
from adapted_amd.lib import EVENTS_TILE as TILE

pytestmark = pytest.mark.gpu
WINDOWS, WIDTHS = (4, 8), (4, 16)
LONG, MANY, BIG, NAN_SCALE = 7, 8, 19, 9  # the segments with an event of more than 128 samples, with many boundaries, the longest, a NaN scale
LEAD = 3  # samples in front of the first segment: offsets[0] > 0
THR_I16 = 6.0  # (white noise over the full int16 range: a threshold that leaves more than E - 1 boundaries in most segments)


def _sizes(w):
    """24 sizes: the small paths, the edges of the score kernel's tile and of its halo, and one that makes several batches at 1 MiB"""
    assert TILE == 1024
    return [0, 2 * w - 1, 2 * w, 1023, 1024, 1025, 2051, 700, 1500, 333, 1, 2 * w + 1, 1024 + w - 1, 1024 + w, 2047, 2048, 2049, 65, 129, 20011,
            5, 1000, 1031, 777]


def _args(w, thr=16.0):
    from adapted_amd import lib

    a = lib.AdpEventArgs()
    a.window, a.min_distance, a.threshold, a.var_floor = w, w, thr, 1e-3
    return a


class _Case:
    """the segments of one window as both calls take them: packed back to back behind LEAD samples, and one per row of a matrix
    [n, L], row g's segment from column g % 3 on.  Read-only."""

    def __init__(self, w, dtype):
        rng = np.random.default_rng(100 + w + (1000 if dtype == np.int16 else 0))
        sizes = _sizes(w)
        self.w, self.n = w, len(sizes)
        self.offsets = (LEAD + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
        self.starts = np.asarray([g % 3 for g in range(self.n)], dtype=np.int64)
        self.ends = self.starts + np.asarray(sizes)
        self.L = (max(self.ends) + 8) // 8 * 8
        self.rows = np.arange(self.n)
        self.lens = np.minimum(self.ends + 5, self.L).astype(np.int32)  # (the rows go on behind their segments)
        if dtype == np.int16:
            seg = [rng.integers(-32768, 32768, size=s).astype(np.int16) for s in sizes]
            seg[LONG][200:500] = seg[LONG][200]  # (a level without noise: no boundary inside, an event of more than 128 samples)
            fill = rng.integers(-32768, 32768, size=(self.n, self.L)).astype(np.int16)
            # calibrations that make both float32 operations round: 15 bits of ADC plus a fractional offset, times a scale of 24 bits
            self.scale = rng.uniform(0.11, 0.23, self.n).astype(np.float32)
            self.offset = rng.uniform(-250.0, 250.0, self.n).astype(np.float32)
            self.scale[NAN_SCALE] = np.nan
        else:
            seg = [eo.staircase(rng, s) for s in sizes]
            seg[LONG][200:500] = np.float32(71.5) + rng.normal(0.0, 0.05, 300).astype(np.float32)
            seg[MANY] = eo.staircase(rng, sizes[MANY], dwell=(12, 20), noise_sd=0.5)
            fill = rng.normal(85.0, 12.0, size=(self.n, self.L)).astype(np.float32)
            self.scale = self.offset = None
        self.seg = seg
        self.packed = np.concatenate([fill[0, :LEAD]] + seg)
        self.matrix = fill
        for g, x in enumerate(seg):
            self.matrix[g, self.starts[g]:self.ends[g]] = x
        assert sum(int(o) & 1 for o in self.offsets[:-1]) >= 6  # several segments start at odd elements
        for a in (self.packed, self.matrix, self.offsets):
            a.setflags(write=False)

    def values(self, g):
        """segment g as float32 pA, formed with numpy: scale * (float32(adc) + offset), rounded twice"""
        if self.scale is None:
            return self.seg[g]
        return (self.scale[g] * (self.seg[g].astype(np.float32) + self.offset[g])).astype(np.float32)

    def cal(self):
        return {} if self.scale is None else dict(scale=self.scale, offset=self.offset)


_CASES = {}


def _case(w, dtype):
    key = (w, np.dtype(dtype).name)
    if key not in _CASES:
        _CASES[key] = _Case(w, dtype)
    return _CASES[key]


@pytest.fixture(scope="module")
def eng():
    from adapted_amd.detect._rows import _engine

    return _engine(0)


def _same_bytes(got, want, what):
    if isinstance(got, dict):
        assert sorted(got) == sorted(want), what
        for k in got:
            _same_bytes(got[k], want[k], (what, k))
    elif isinstance(got, tuple):
        assert len(got) == len(want), what
        for k, (a, b) in enumerate(zip(got, want)):
            _same_bytes(a, b, (what, k))
    else:
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def _cap(info):
    return int(max(info[:, 0].max(), 1))


@pytest.mark.parametrize("w", WINDOWS)
def test_packed_float32_is_the_matrix_call(eng, w):
    c, a = _case(w, np.float32), _args(w)
    cap = _cap(eng.segment_events(c.matrix, c.lens, c.rows, c.starts, c.ends, a)[1])
    want = eng.segment_events(c.matrix, c.lens, c.rows, c.starts, c.ends, a, cap=cap)
    _same_bytes(eng.segment_events_packed(c.packed, c.offsets, a, cap=cap), want, "segment")
    assert want[1][:3, 1].tolist() == [2, 2, 0] and (want[1][3:, 1] == (np.asarray(_sizes(w)[3:]) < 2 * w) * 2).all()
    assert want[1][MANY, 0] > 16 and cap > 16
    for E in WIDTHS:
        wl = eng.event_levels(c.matrix, c.lens, c.rows, c.starts, c.ends, a, E)
        _same_bytes(eng.event_levels_packed(c.packed, c.offsets, a, E), wl, ("levels", E))
        assert wl["lengths"][LONG].max() > 128 and wl["count"][MANY] == E and (wl["status"][[3, 4, 5, 6, BIG]] == 0).all()
    # the public wrappers
    from adapted_amd import fingerprint, polya_length

    pos, count, status, stats = polya_length.segment_events_packed(c.packed, c.offsets, polya_length.EventParams(w, w, 16.0), engine=eng)
    _same_bytes((pos, count, status, stats), (want[0], want[1][:, 0].copy(), want[1][:, 1].copy(), want[2]), "wrapper")
    r = fingerprint.event_levels_packed(c.packed, c.offsets, fingerprint.FingerprintParams(16, polya_length.EventParams(w, w, 16.0)), engine=eng)
    _same_bytes((r.count, r.fingerprints, r.event_len_med), (wl["count"], wl["fingerprints"], wl["stats"][:, 0].copy()), "wrapper")


@pytest.fixture(scope="module")
def calibrated():
    """per window: an engine whose rows are the case's, with calibrate_i16's float32 matrix of the raw rows on the device"""
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config

    made = {}
    for w in WINDOWS:
        c = _case(w, np.int16)
        e = lib.Engine(get_chemistry_specific_config("RNA004"), c.n, c.L, device=0)
        d_raw, d_len, d_cal, d_f32 = e.dev_alloc(c.n * c.L * 2 + 64), e.dev_alloc(c.n * 4), e.dev_alloc(2 * c.n * 4), e.dev_alloc(c.n * c.L * 4)
        e.h2d(d_raw, c.matrix)
        e.h2d(d_len, c.lens)
        e.h2d(d_cal, np.concatenate([c.scale, c.offset]))
        e.calibrate_i16(d_raw, d_len, d_cal, d_cal + 4 * c.n, c.n, d_f32)
        made[w] = (e, d_f32, (d_raw, d_len, d_cal, d_f32))
    yield made
    for e, _, ptrs in made.values():
        for p in ptrs:
            e.dev_free(p)
        e.close()


@pytest.mark.parametrize("w", WINDOWS)
def test_packed_int16_is_calibrate_first(eng, calibrated, w):
    c, a = _case(w, np.int16), _args(w, THR_I16)
    e, d_f32, _ = calibrated[w]
    cap = _cap(e.segment_events(d_f32, c.lens, c.rows, c.starts, c.ends, a, n=c.n, L=c.L)[1])
    want = e.segment_events(d_f32, c.lens, c.rows, c.starts, c.ends, a, cap=cap, n=c.n, L=c.L)
    _same_bytes(eng.segment_events_packed(c.packed, c.offsets, a, cap=cap, **c.cal()), want, "segment")
    assert want[1][NAN_SCALE].tolist() == [0, 1] and (np.delete(want[1][:, 1], NAN_SCALE) != 1).all()  # status 1: the NaN scale alone
    assert (want[1][[3, 4, 5, 6, BIG], 0] > 16).all()
    for E in WIDTHS:
        wl = e.event_levels(d_f32, c.lens, c.rows, c.starts, c.ends, a, E, n=c.n, L=c.L)
        _same_bytes(eng.event_levels_packed(c.packed, c.offsets, a, E, **c.cal()), wl, ("levels", E))
        assert wl["lengths"][LONG].max() > 128 and wl["status"][NAN_SCALE] == 1 and (wl["count"][[3, 4, 5, 6, BIG]] == E).all()


def _bits(a):
    a = np.array(a, dtype=np.float64)
    a[a != a] = np.nan
    return a.view(np.uint64).tolist()


@pytest.mark.parametrize("w", WINDOWS)
def test_packed_int16_is_the_numpy_restatement(eng, w):
    """boundaries, statuses and gap statistics are events_oracle's on scale * (float32(adc) + offset) formed with numpy; the event
    tables -- with more than E - 1 boundaries the selection reads the scores -- are fingerprint_oracle's"""
    c, a = _case(w, np.int16), _args(w, THR_I16)
    want = [eo.segment(c.values(g), w, w, THR_I16, 1e-3) for g in range(c.n)]
    for g in range(c.n):
        assert not eo.has_close_ties(c.values(g), w, w, THR_I16, 1e-3), g
    cap = max(b.size for b, _, _, _ in want)
    pos, info, stats = eng.segment_events_packed(c.packed, c.offsets, a, cap=cap, **c.cal())
    for g, (b, status, med, mad) in enumerate(want):
        assert (int(info[g, 0]), int(info[g, 1])) == (b.size, status), g
        assert pos[g, :b.size].tolist() == b.tolist() and (pos[g, b.size:] == -1).all(), g
        assert _bits(stats[g]) == _bits([med, mad]), g
    assert want[NAN_SCALE][1] == 1 and [want[g][1] for g in (0, 1, 2)] == [2, 2, 0]
    for E in WIDTHS:
        r = eng.event_levels_packed(c.packed, c.offsets, a, E, **c.cal())
        ol = [fo.levels(c.values(g), E, w, w, THR_I16, 1e-3) for g in range(c.n)]
        assert fo.same(r["count"], np.asarray([o["count"] for o in ol], dtype=np.int32))
        assert fo.same(r["status"], np.asarray([o["status"] for o in ol], dtype=np.int32))
        assert fo.same(r["lengths"], np.stack([o["lengths"] for o in ol]))
        assert fo.same(r["levels"], np.stack([o["levels"] for o in ol]))
        assert fo.same(r["fingerprints"], np.stack([o["fp"] for o in ol]))
        assert fo.same(r["norm"], np.asarray([o["norm"] for o in ol]))
        assert sum(o["nk"] > E - 1 for o in ol) >= 12  # (the selection by score ran)


@pytest.mark.parametrize("dtype", (np.float32, np.int16))
def test_device_and_host_inputs_agree(eng, dtype):
    w, E = 8, 16
    c = _case(w, dtype)
    a = _args(w, THR_I16 if dtype == np.int16 else 16.0)
    host = eng.event_levels_packed(c.packed, c.offsets, a, E, **c.cal())
    seg = eng.segment_events_packed(c.packed, c.offsets, a, cap=20, **c.cal())
    ptrs = [eng.dev_alloc(c.packed.nbytes + 64), eng.dev_alloc(c.n * E * 8), eng.dev_alloc(c.n * 4), eng.dev_alloc(c.n * 4), eng.dev_alloc(c.n * 4)]
    try:
        d_packed, d_fp, d_count, d_scale, d_offset = ptrs
        eng.h2d(d_packed, c.packed)
        cal = {}
        if dtype == np.int16:
            eng.h2d(d_scale, c.scale)
            eng.h2d(d_offset, c.offset)
            cal = dict(scale=d_scale, offset=d_offset)
        _same_bytes(eng.segment_events_packed(d_packed, c.offsets, a, cap=20, **cal), seg, "segment")
        _same_bytes(eng.event_levels_packed(d_packed, c.offsets, a, E, **cal), host, "levels")
        dev = eng.event_levels_packed(d_packed, c.offsets, a, E, fp_ptr=d_fp, count_ptr=d_count, **cal)
        assert dev["fingerprints"] is None and dev["count"] is None
        _same_bytes({k: v for k, v in dev.items() if v is not None}, {k: v for k, v in host.items() if k not in ("fingerprints", "count")}, "kept")
        fp, count = np.zeros((c.n, E)), np.zeros(c.n, dtype=np.int32)
        eng.d2h(fp, d_fp)
        eng.d2h(count, d_count)
        _same_bytes((fp, count), (host["fingerprints"], host["count"]), "device tables")
        pick = np.flatnonzero(host["status"] == 0)[[3, 7, 11]]
        t, tc = np.where(np.isnan(host["fingerprints"][pick]), 0.0, host["fingerprints"][pick]), host["count"][pick]
        on_dev = eng.dtw_assign(d_fp, d_count, t, tc, 3, nq=c.n, Eq=E)
        _same_bytes(on_dev, eng.dtw_assign(host["fingerprints"], host["count"], t, tc, 3), "dtw")
        assert (on_dev[1][pick, 0] == [0, 1, 2]).all() and np.isnan(on_dev[0][host["status"] != 0]).all()
    finally:
        for p in ptrs:
            eng.dev_free(p)


@pytest.mark.parametrize("dtype", (np.float32, np.int16))
def test_batches_of_slots_change_nothing(eng, monkeypatch, dtype):
    from adapted_amd import lib

    w, E = 8, 16
    c = _case(w, dtype)
    a = _args(w, THR_I16 if dtype == np.int16 else 16.0)
    assert lib.EVENTS_SCRATCH_MIB * (1 << 20) // lib.events_slot_bytes(max(_sizes(w))) >= c.n  # by default one batch
    assert (1 << 20) // lib.events_slot_bytes(max(_sizes(w))) == 4  # at 1 MiB four slots: six batches
    one = (eng.segment_events_packed(c.packed, c.offsets, a, cap=40, **c.cal()), eng.event_levels_packed(c.packed, c.offsets, a, E, **c.cal()))
    monkeypatch.setenv("ADP_EVENTS_SCRATCH_MIB", "1")
    eng.set_profiling(True)
    try:
        many = (eng.segment_events_packed(c.packed, c.offsets, a, cap=40, **c.cal()), eng.event_levels_packed(c.packed, c.offsets, a, E, **c.cal()))
        launches = [name for name, _ in eng.kernel_times()]
    finally:
        eng.set_profiling(False)
    assert launches.count("k_ev_bounds") == launches.count("k_ev_levels") == 6  # (the last call ran in six batches)
    _same_bytes(many, one, "batches")


def test_one_engine_alternating_the_calls_gives_what_fresh_engines_give():
    from adapted_amd import lib
    from adapted_amd.config import get_chemistry_specific_config

    w, E = 4, 16
    f, i = _case(w, np.float32), _case(w, np.int16)
    a, ai = _args(w), _args(w, THR_I16)
    spc = get_chemistry_specific_config("RNA004")
    calls = [lambda e: e.event_levels_packed(i.packed, i.offsets, ai, E, **i.cal()),
             lambda e: e.event_levels(f.matrix, f.lens, f.rows, f.starts, f.ends, a, E),
             lambda e: e.segment_events_packed(f.packed, f.offsets, a, cap=30),
             lambda e: e.segment_events(f.matrix, f.lens, f.rows, f.starts, f.ends, a, cap=30),
             lambda e: e.segment_events_packed(i.packed, i.offsets, ai, cap=30, **i.cal()),
             lambda e: e.event_levels_packed(f.packed, f.offsets, a, E)]
    one = lib.Engine(spc, 1, 4096, device=0)
    try:
        mixed = [call(one) for call in calls + calls[::-1]]
    finally:
        one.close()
    for k, call in enumerate(calls):
        fresh = lib.Engine(spc, 1, 4096, device=0)
        try:
            want = call(fresh)
        finally:
            fresh.close()
        _same_bytes(mixed[k], want, k)
        _same_bytes(mixed[len(mixed) - 1 - k], want, k)


def test_refusals_leave_the_handle_usable(eng):
    from adapted_amd import lib

    c, a = _case(8, np.float32), _args(8)
    good = eng.segment_events_packed(c.packed, c.offsets, a, cap=4)
    L, h = eng.lib, eng._h
    info, stats = np.zeros((c.n, 2), dtype=np.int64), np.zeros((c.n, 2))
    import ctypes

    def call(packed=c.packed, offsets=c.offsets, scale=None, offset=None, n=c.n, args=a, flags=0):
        return L.adp_segment_events_packed(h, packed, offsets, scale, offset, n, ctypes.byref(args), flags, 0, None, info, stats)

    down = c.offsets.copy()
    down[5] = down[4] - 1
    huge = np.asarray([0, 1 << 30], dtype=np.int64)
    for kw, say in ((dict(n=0), b"bad argument"), (dict(offsets=c.offsets - 4), b"offsets[0]"), (dict(offsets=down), b"decrease"),
                    (dict(offsets=huge, n=1), b"2^30"), (dict(flags=lib.ADP_PACKED_I16), b"ADP_PACKED_I16"),
                    (dict(flags=lib.ADP_MVS_F64), b"float64"), (dict(args=_args(65)), b"window"), (dict(args=_args(8, float("nan"))), b"threshold")):
        assert call(**kw) == -1 and say in L.adp_last_error(), kw
    _same_bytes(eng.segment_events_packed(c.packed, c.offsets, a, cap=4), good, "after the refusals")


# ---- the command, end to end

N_READS = 48
SEED = 11


def _bundle(m):
    """48 synthetic reads with staircase adapters (the recipe of tests/test_gpu_polya_length_cli.py), quantised (the recipe of
    tests/test_gpu_cnn_i16.py) -> (signals: the calibrated raw, float32 NaN-padded; raw; scale; offset; lens)"""
    from adapted_amd import synth
    from test_gpu_cnn_i16 import _calibrated

    sig, lens = synth.synth_batch(SEED, 0, N_READS, m)
    rng = np.random.default_rng(5)
    for k in range(N_READS):
        a_len, _, flags, sp_start, op_start = synth.read_params(SEED, k)
        mean = np.full(a_len, 80.0, dtype=np.float32)
        level = np.repeat(rng.normal(80.0, 7.0, size=a_len // 20 + 2), rng.integers(20, 41, size=a_len // 20 + 2))[:a_len]
        if flags & synth.FLAG_START_PEAK:
            mean[sp_start:sp_start + synth.SP_LEN] = 150.0
            level[sp_start:sp_start + synth.SP_LEN] = 150.0
        if flags & synth.FLAG_OPEN_PORE:
            mean[op_start:op_start + synth.OP_LEN] = 230.0
            level[op_start:op_start + synth.OP_LEN] = 230.0
        noise = (sig[k, :a_len] - mean).astype(np.float64) * (1.5 / 7.0)
        sig[k, :a_len] = (level + noise).astype(np.float32)
    rng = np.random.default_rng(8)
    scale, offset = rng.uniform(0.14, 0.2, N_READS).astype(np.float32), rng.uniform(-20.0, 20.0, N_READS).astype(np.float32)
    raw = np.clip(np.rint(np.nan_to_num(sig, nan=108.0) / scale[:, None] - offset[:, None]), -32768, 32767).astype(np.int16)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    return _calibrated(raw, scale, offset, lens), raw, scale, offset, lens


def _files(root):
    out = {}
    for sub in ("boundaries", "failed_reads", "polya_length", "fingerprints"):
        d = os.path.join(root, sub)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            with open(os.path.join(d, f), "rb") as fh:
                out[sub + "/" + f] = fh.read()
    return out


def _run_dir(root):
    runs = [d for d in os.listdir(root) if d.startswith("adapted_")]
    assert len(runs) == 1, runs
    return os.path.join(root, runs[0])


OPTIONS = ["--polya_length", "events", "--fingerprints", "16"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, oracle_mod):
    """detect runs of the bundle -- with the event options, with them and --event_params 4,4,9, and one with --int16_ingest and no
    event option -- and what `adapted events` makes of them"""
    from adapted_amd import fingerprint as fpm
    from adapted_amd import main as cli
    from test_gpu_polya_length_cli import _spc

    tmp = tmp_path_factory.mktemp("events_packed_cli")
    spc = _spc()
    signals, raw, scale, offset, lens = _bundle(spc.sig_preload_size)
    # the precondition, on the CPU oracle: at least 40 of the 48 reads pass detect on the float32 bundle
    n_pass = sum(bool(r["success"]) for r in oracle_mod.detect_llr(signals, lens, spc))
    assert n_pass >= 40, n_pass
    ids = np.array(["read_%04d" % i for i in range(N_READS)], dtype=object)
    bundle = str(tmp / "reads_0.npz")
    np.savez(bundle, signals=signals, raw=raw, scale=scale, offset=offset, full_lengths=lens, read_ids=ids)
    cfg = str(tmp / "cfg.toml")
    spc.to_toml(cfg)
    rng = np.random.default_rng(3)
    lv = rng.normal(0.0, 1.5, size=(3, 16))
    lv[1, 12:], lv[2, 9:] = np.nan, np.nan
    templates = str(tmp / "templates.npz")
    fpm.save_templates(templates, fpm.Templates(["bcA", "bcB", "bcC"], lv, np.asarray([16, 12, 9], dtype=np.int32)))
    full = OPTIONS + ["--barcode_templates", templates, "--dtw_band", "3"]
    detect = ["detect", "-i", bundle, "--config", cfg, "-s", str(N_READS), "-b", "20"]
    out = {}
    for name, extra in (("detect", full), ("detect_params", full + ["--event_params", "4,4,9"]), ("detect_i16", ["--int16_ingest"])):
        cli.main(detect + ["-o", str(tmp / name)] + extra)
        out[name] = _run_dir(str(tmp / name))
    for name, run, extra in (("plain", "detect", []), ("i16", "detect", ["--int16_ingest"]), ("params", "detect", ["--event_params", "4,4,9"]),
                             ("of_i16", "detect_i16", ["--int16_ingest"])):
        cli.main(["events", out[run], "-i", bundle, "-o", str(tmp / name)] + full + extra)
        out[name] = str(tmp / name)
    return {k: (v, _files(v)) for k, v in out.items()}, n_pass


def _extension_files(files):
    return {f: v for f, v in files.items() if f.startswith(("polya_length/", "fingerprints/"))}


def _assert_same_files(got, want):
    assert sorted(got) == sorted(want) and len(got) == 9  # three files of 20, 20 and the rest: three kinds each
    for f in want:
        if f.endswith(".npz"):
            import io

            with np.load(io.BytesIO(got[f])) as a, np.load(io.BytesIO(want[f])) as b:
                assert sorted(a.files) == sorted(b.files) == ["count", "fingerprints", "lengths", "levels", "read_id", "status"]
                for k in a.files:
                    assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (f, k)
                    assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (f, k)
        else:
            assert got[f] == want[f], f  # polya_length_<k>.csv and barcodes_<k>.csv: byte for byte


def test_the_command_writes_what_detect_wrote(runs):
    out, n_pass = runs
    want = _extension_files(out["detect"][1])
    lines = sum(v.count(b"\n") - 1 for f, v in out["detect"][1].items() if f.startswith("boundaries/"))
    assert lines >= 40 and n_pass >= 40  # (the check counts: most of the 48 reads pass, on the GPU and on the CPU oracle)
    _assert_same_files(_extension_files(out["plain"][1]), want)
    assert not any(f.startswith(("boundaries/", "failed_reads/")) for f in out["plain"][1])
    assert os.path.exists(os.path.join(out["plain"][0], "events_command.json"))
    pl = b"".join(v for f, v in sorted(want.items()) if f.startswith("polya_length/")).splitlines()
    assert sum(ln.split(b",")[3] not in (b"", b"0") for ln in pl if not ln.startswith(b"read_id")) == lines  # every read has events


def test_the_command_on_raw_samples_writes_the_same(runs):
    out, _ = runs
    _assert_same_files(_extension_files(out["i16"][1]), _extension_files(out["detect"][1]))


def test_another_setting_equals_a_second_detect_run(runs):
    out, _ = runs
    want = _extension_files(out["detect_params"][1])
    _assert_same_files(_extension_files(out["params"][1]), want)
    assert any(want[f] != v for f, v in _extension_files(out["detect"][1]).items())  # (the setting matters)


def test_a_run_detect_cannot_extend_gets_the_same_files(runs):
    """a run made with --int16_ingest carries no event files and detect refuses to make them; `adapted events --int16_ingest` does"""
    out, _ = runs
    assert not _extension_files(out["detect_i16"][1])
    assert {f: v for f, v in out["detect_i16"][1].items()} == {f: v for f, v in out["detect"][1].items() if f.startswith(("boundaries/", "failed_reads/"))}
    _assert_same_files(_extension_files(out["of_i16"][1]), _extension_files(out["detect"][1]))


def test_the_command_after_the_scan(runs, tmp_path, caplog):
    """a read of the run that the input lacks: its file is not written, the others are; an input without raw samples with
    --int16_ingest; an output that exists; RUN_DIR as OUT_DIR"""
    from adapted_amd import main as cli

    out, _ = runs
    run = out["detect_i16"][0]
    with np.load(os.path.join(os.path.dirname(os.path.dirname(run)), "reads_0.npz"), allow_pickle=True) as z:
        keep = {k: z[k] for k in z.files}
    with open(os.path.join(run, "boundaries", "detected_boundaries_1.csv")) as fh:
        gone = [ln.split(",")[0] for ln in fh.read().splitlines()[1:3]]
    sel = np.asarray([str(r) not in gone for r in keep["read_ids"]])
    np.savez(tmp_path / "fewer_0.npz", **{k: v[sel] for k, v in keep.items() if k != "raw"})
    with pytest.raises(SystemExit) as e:
        cli.main(["events", run, "-i", str(tmp_path / "fewer_0.npz"), "-o", str(tmp_path / "fewer"), "--polya_length", "events"])
    assert "2 read(s) of the run are not in the input" in str(e.value) and gone[0] in str(e.value)
    assert sorted(os.listdir(tmp_path / "fewer" / "polya_length")) == ["polya_length_0.csv", "polya_length_2.csv"]
    for f in ("polya_length_0.csv", "polya_length_2.csv"):
        assert (tmp_path / "fewer" / "polya_length" / f).read_bytes() == out["detect"][1]["polya_length/" + f]
    with pytest.raises(SystemExit) as e:
        cli.main(["events", run, "-i", str(tmp_path / "fewer_0.npz"), "-o", str(tmp_path / "no_raw"), "--polya_length", "events", "--int16_ingest"])
    assert "holds no raw ADC samples" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["events", run, "-i", str(tmp_path / "fewer_0.npz"), "-o", str(tmp_path / "fewer"), "--polya_length", "events"])
    assert "exists" in str(e.value) and "--force" in str(e.value)
    # into the run directory itself: the run detect could not extend now holds the files
    bundle = os.path.join(os.path.dirname(os.path.dirname(run)), "reads_0.npz")
    import logging

    caplog.set_level(logging.INFO)
    cli.main(["events", run, "-i", bundle, "-o", run, "--int16_ingest"] + OPTIONS)
    last = caplog.records[-1].getMessage()  # the log ends with the reads, the slices' samples and the rate
    assert last.startswith("Processed %d reads, " % sum(len(v.splitlines()) - 1 for f, v in out["detect"][1].items() if f.startswith("boundaries/")))
    assert "adapter samples" in last and "reads/s" in last
    got = _extension_files(_files(run))
    want = {f: v for f, v in _extension_files(out["detect"][1]).items() if "barcodes" not in f}
    assert sorted(got) == sorted(want)
    for f in want:
        if f.endswith(".csv"):
            assert got[f] == want[f], f
