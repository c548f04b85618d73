"""The batches of tests/test_gpu_llr_stream.py as plain functions, with their truth from the CPU oracle and the coverage
conditions they were made for (tests/test_llr_stream_oracle_cpu.py asserts those without a GPU; the GPU tests repeat them).

A read's n_valid is set through its length: the row is NaN from full_len on, so the pooled blocks that reach into the padding are
NaN and n_valid = (full_len - min_obs_adapter) // ds; a row without padding gives n_valid = L = ceil((T - min_obs_adapter) / ds).
Everything returned is cached and shared: callers leave it unchanged."""
import functools
from collections import namedtuple

import numpy as np

import llr_stream_oracle as so

WAVE = 64
UNIFORM_SPAN = 8 * so.CK   # csum_uniform (llr_stream.h): max - min < 128 over the wave's 64 lanes, lanes past n_reads counting as 0

Geom = namedtuple("Geom", "T off ds L Lp m")
Batch = namedtuple("Batch", "geom name sig lens minibatch plan")   # plan: the n_valid each read was made for (None: whatever comes)

# core.max_obs_trace / min_obs_adapter / downscale_factor
GEOMS = {
    "pad": (21490, 1000, 10),      # L = 2049 = 32 * 64 + 1: two full 1024-point tiles and a ragged third
    "full": (22120, 1000, 10),     # L = 2112 = 33 * 64 = Lp: the clamped loads at a row's end
    "short": (2000, 1000, 10),     # L = 100: every wave is uniform
    "ds3": (7147, 1000, 3),        # L = 2049
    "ds7": (15343, 1000, 7),       # L = 2049
    "ds32": (21500, 1004, 32),     # L = 641
    "scalar": (21490, 1001, 10),   # L = 2049; no row of the matrix starts its segment on a 16-byte boundary (m % 4 == 2)
}
EDGE_NVALID = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 143, 144, 145, 1023, 1024, 1025)   # and L - 1, L


@functools.lru_cache(maxsize=None)
def spc_of(geom):
    from adapted_amd.config import get_chemistry_specific_config

    T, off, ds = GEOMS[geom]
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.core.max_obs_trace, spc.core.min_obs_adapter, spc.core.downscale_factor = T, off, ds
    spc.update_primary_method()
    spc.update_sig_preload_size()
    return spc


@functools.lru_cache(maxsize=None)
def geom_of(geom):
    spc = spc_of(geom)
    m = spc.sig_preload_size
    T, off, ds = min(spc.core.max_obs_trace, m), spc.core.min_obs_adapter, spc.core.downscale_factor
    L = -(-(T - off) // ds)
    return Geom(T, off, ds, L, -(-L // 64) * 64, m)


@functools.lru_cache(maxsize=None)
def pool(geom, seed=41):
    """256 full-length synth reads of the geometry's preload size (read-only)"""
    from adapted_amd import synth

    sig, _ = synth.synth_batch(seed, 0, 256, geom_of(geom).m)
    sig.setflags(write=False)
    return sig


def decoy(geom, n):
    """an unrelated batch of full-length reads, run before every stage so that nothing stale passes for a result"""
    g = geom_of(geom)
    return pool(geom, 97)[:n], np.full(n, g.m, dtype=np.int32)


def full_len_for(g, nv):
    return g.m if nv >= g.L else (g.off + nv * g.ds if nv > 0 else 0)


def make(geom, name, plan, minibatch=None, holes=(), sig=None):
    g = geom_of(geom)
    plan = [int(v) for v in plan]
    n = len(plan)
    lens = np.array([full_len_for(g, v) for v in plan], dtype=np.int32)
    sig = (pool(geom)[:n] if sig is None else sig).copy()
    for r in range(n):
        sig[r, lens[r]:] = np.nan
    for r, at, w in holes:
        sig[r, at: at + w] = np.nan
        plan[r] = None
    sig.setflags(write=False)
    return Batch(geom, name, sig, lens, minibatch or n, tuple(plan))


def _cycle(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


def edge_values(geom):
    L = geom_of(geom).L
    return tuple(v for v in EDGE_NVALID if v < L - 1) + (L - 1, L)


# ---------------------------------------------------------------- the wave layouts (one batch each)
def _edges_uniform(geom):
    """every edge length inside a wave of nearly one length (k_cumsum_gather's by default); 11 and 12: an empty and a one-point
    computed range of pass 1"""
    L = geom_of(geom).L
    groups = [(1, 2, 11, 12, 15, 16, 17, 31, 32, 33, 127), (127, 128, 129, 143, 144, 145), (1023, 1024, 1025), (L - 1, L)]
    plan = []
    for grp in groups:
        grp = [v for v in grp if v <= L]
        if grp:
            plan += _cycle(grp, WAVE)
    return make(geom, "edges_uniform", plan)


def _edges_mixed(geom):
    """every edge length in one wave of very different lengths (k_cumsum's), and a read with a NaN hole in the middle"""
    g = geom_of(geom)
    plan = _cycle(edge_values(geom) + (11, 12), WAVE)
    plan[WAVE - 1] = g.L
    return make(geom, "edges_mixed", plan, holes=((WAVE - 1, g.off + (g.L // 2) * g.ds + 3, 4),))


def _span(geom, span):
    plan = [1000 + 2 * i for i in range(WAVE)]
    plan[WAVE - 1] = 1000 + span
    return make(geom, "span%d" % span, plan)


def _full_wave(geom):
    return make(geom, "full_wave", [geom_of(geom).L] * WAVE)


def _equal_in_line(geom):
    """waves of equal lengths that end inside a gathered line of eight checkpoints: n % 128 = 1, 16, 17, 127"""
    return make(geom, "equal_in_line", [1025] * WAVE + [144] * WAVE + [145] * WAVE + [255] * WAVE)


_SHORT8 = (5, 17, 100, 127, 33, 64, 1, 90)


def _ragged_short(geom):
    L = geom_of(geom).L
    return make(geom, "ragged_short", [L] * WAVE + [min(v, L) for v in _SHORT8])


def _ragged_long(geom):
    L = geom_of(geom).L
    plan = [L] * WAVE + list(_SHORT8)
    plan[WAVE + 3] = L
    return make(geom, "ragged_long", plan)


def _half_dropped(geom):
    """two minibatches of 32 in one wave, the second all NaN with full_len = 0"""
    return make(geom, "half_dropped", [geom_of(geom).L] * 32 + [0] * 32, minibatch=32)


def _wave_dropped(geom):
    return make(geom, "wave_dropped", [geom_of(geom).L] * WAVE + [0] * WAVE, minibatch=WAVE)


_BUILDERS = {"edges_uniform": _edges_uniform, "edges_mixed": _edges_mixed, "span127": lambda g: _span(g, 127), "span128": lambda g: _span(g, 128),
             "full_wave": _full_wave, "equal_in_line": _equal_in_line, "ragged_short": _ragged_short, "ragged_long": _ragged_long,
             "half_dropped": _half_dropped, "wave_dropped": _wave_dropped}
# (geometry, batch, the kind of each wave by csum_uniform: U k_cumsum_gather's, M k_cumsum's)
LAYOUTS = (
    ("pad", "edges_uniform", "UUUU"), ("pad", "edges_mixed", "M"), ("pad", "span127", "U"), ("pad", "span128", "M"), ("pad", "full_wave", "U"),
    ("pad", "equal_in_line", "UUUU"), ("pad", "ragged_short", "UU"), ("pad", "ragged_long", "UM"), ("pad", "half_dropped", "M"),
    ("pad", "wave_dropped", "UU"),
    ("full", "edges_uniform", "UUUU"), ("full", "edges_mixed", "M"), ("full", "full_wave", "U"),
    ("short", "edges_uniform", "UU"), ("short", "ragged_short", "UU"), ("short", "half_dropped", "U"), ("short", "wave_dropped", "UU"),
)


@functools.lru_cache(maxsize=None)
def batch(geom, name):
    return _BUILDERS[name](geom)


def wave_kinds(nvalid, n_reads):
    """csum_uniform restated: per group of 64 lanes, U when max - min < 128 (lanes past n_reads hold 0)"""
    out = ""
    for w0 in range(0, n_reads, WAVE):
        v = [int(nvalid[r]) if r < n_reads else 0 for r in range(w0, w0 + WAVE)]
        out += "U" if max(v) - min(v) < UNIFORM_SPAN else "M"
    return out


# ---------------------------------------------------------------- pass 2: seam reads and plateaus (geometry "pad")
def _adapter_noise(rng, k):
    return (np.float32(80.0) + np.float32(7.0) * rng.standard_normal(k).astype(np.float32)).astype(np.float32)


SEAM_STEPS = tuple(range(1006, 1046))   # pooled index of the adapter boundary, stepped by one pooled point = ds samples


@functools.lru_cache(maxsize=None)
def seam_batch():
    """reads whose adapter runs up to pooled index ~1024 -- the seam of k_gains' first two 1024-point tiles --: adapter-like noise up
    to the boundary, behind it a synth read's poly(A) and RNA"""
    from adapted_amd import synth

    g = geom_of("pad")
    base = pool("pad")
    rng = np.random.default_rng(2024)
    n = len(SEAM_STEPS)
    sig = np.empty((n, g.m), dtype=np.float32)
    for r, k in enumerate(SEAM_STEPS):
        b = g.off + k * g.ds
        a_len = synth.read_params(41, r)[0]
        sig[r, :b] = _adapter_noise(rng, b)
        sig[r, b:] = base[r, a_len: a_len + g.m - b]
    return make("pad", "seam", [g.L] * n, sig=sig)


PLATEAU_READS = (3, 9, 14, 20)   # reads of plateau_batch with the saturated stretch
PLATEAU_LEN = 400                # samples


@functools.lru_cache(maxsize=None)
def plateau_batch():
    """reads with a stretch of samples far above the clip bound directly behind the adapter: every pooled point of the stretch is the
    same float32 (the clip bound, normalised), the head segments of pass 2 that lie inside it have zero variance, so their gains are
    +inf side by side -- a plateau of the sanitised trace, which k_gains<2> answers with npk = -1 and k_polya_peak with a recount"""
    from adapted_amd import synth

    g = geom_of("pad")
    n = 24
    sig = pool("pad")[:n].copy()
    for r in PLATEAU_READS:
        a_len = synth.read_params(41, r)[0]
        b = g.off + -(-(a_len - g.off) // g.ds) * g.ds   # the first pooled block's edge at or behind the adapter's end
        sig[r, b: b + PLATEAU_LEN] = np.float32(400.0)
    return make("pad", "plateau", [g.L] * n, sig=sig)


# ---------------------------------------------------------------- D1: reads that end around a pooled block's and a tile's edge
NP_TILE = 512


@functools.lru_cache(maxsize=None)
def d1_batch(geom):
    """full-length reads, reads ending one sample before / at / one sample after a pooled block's edge and a 512-block tile's edge,
    reads of three pooled points and of every point but the last, and a NaN hole"""
    g = geom_of(geom)
    n = 24
    lens = np.full(n, g.m, dtype=np.int32)
    k = 0
    for blk in (min(700, g.L - 30), NP_TILE, 2, g.L - 1):
        for d in (-1, 0, 1):
            lens[k] = g.off + blk * g.ds + d
            k += 1
    lens[k] = g.T; lens[k + 1] = g.T - 1; lens[k + 2] = g.off + g.ds * 3 + g.ds // 2   # noqa: E702
    sig = pool(geom)[:n].copy()
    for r in range(n):
        sig[r, lens[r]:] = np.nan
    sig[n - 1, g.off + 40 * g.ds + 1] = np.nan
    sig.setflags(write=False)
    return Batch(geom, "d1", sig, lens, n, (None,) * n)


def scalar_path_rows(geom, n):
    """the float offset of every row's pooled segment from the matrix's (16-byte aligned) start, modulo 4: k_norm_pool takes its
    float4 paths for a row only where this is 0"""
    g = geom_of(geom)
    return [(r * g.m + g.off) % 4 for r in range(n)]


# ---------------------------------------------------------------- the truth
_REF = {}


def reference(oracle, b):
    """per read: None for a read of a dropped minibatch (one without any sample), else the oracle's stages (n_valid, down, g1, g2,
    cand, polya_idx) with `ck` / `tail` from llr_stream_oracle.checkpoints.  Cached by batch."""
    key = (b.geom, b.name)
    if key in _REF:
        return _REF[key]
    spc = spc_of(b.geom)
    n = b.sig.shape[0]
    out = [None] * n
    for m0 in range(0, n, b.minibatch):
        mb = b.sig[m0: m0 + b.minibatch]
        if np.isnan(mb[:, : spc.core.max_obs_trace]).all():
            continue
        rc, np4 = oracle.norm_params(mb, spc.core.max_obs_trace, spc.core.sig_norm_outlier_thresh)
        assert rc == 0
        st = [oracle.llr_stages(row, spc, np4) for row in mb]
        assert all(s["n_valid"] > 0 for s in st), "a read without a pooled block sinks its minibatch: not made here"
        for k, s in enumerate(st):
            s["ck"], s["tail"] = so.checkpoints(s["down"], s["n_valid"])
            out[m0 + k] = s
    _REF[key] = out
    return out


def nvalid_of(ref):
    return [0 if s is None else s["n_valid"] for s in ref]


# ---------------------------------------------------------------- the coverage the batches were made for
# (asserted without a GPU by test_llr_stream_oracle_cpu.py, repeated by the GPU tests)
def check_layout(oracle, geom, name, kinds):
    """the oracle's n_valid are the planned ones, the waves are of the kinds the batch was made for (csum_uniform restated)"""
    b = batch(geom, name)
    ref = reference(oracle, b)
    nv = nvalid_of(ref)
    n = len(nv)
    assert n <= 256 and b.sig.shape == (n, geom_of(geom).m)
    assert all(p is None or p == v for p, v in zip(b.plan, nv)), (b.plan, nv)
    assert wave_kinds(nv, n) == kinds
    L = geom_of(geom).L
    if name.startswith("edges"):
        assert set(edge_values(geom)) | ({11, 12} if L > 12 else set()) <= set(nv)
    if name == "edges_mixed":                                  # the NaN hole: pooled NaN inside down[:n], whole NaN blocks in pass 1
        s = ref[WAVE - 1]
        assert s["n_valid"] == L - 1 and np.isnan(s["down"]).sum() == 1
        assert np.isinf(so.summaries(s["g1"], s["n_valid"], False)[1]).any()
    if name in ("span127", "span128"):
        assert max(nv) - min(nv) == int(name[4:])
    if name == "equal_in_line":
        assert [nv[w] % 128 for w in range(0, n, 64)] == [1, 16, 17, 127] and all(len(set(nv[w: w + 64])) == 1 for w in range(0, n, 64))
    if name.startswith("ragged"):
        assert n % 64 and (max(nv[64:]) < 128) == (name == "ragged_short")
    if name == "half_dropped":
        assert b.minibatch == 32 and all(s is not None for s in ref[:32]) and all(s is None for s in ref[32:]) and (b.lens[32:] == 0).all()
    if name == "wave_dropped":
        assert b.minibatch == 64 and all(s is None for s in ref[64:]) and (b.lens[64:] == 0).all()
    return b, ref


def check_seam(oracle):
    """candidates with cand + 1 = 1023, 1024, 1025 (pass 2's first computed point on either side of the tile seam) and strict maxima at
    1022, 1023, 1024 (the carries across the seam, lanes 62 / 63)"""
    ref = reference(oracle, seam_batch())
    assert {1023, 1024, 1025} <= {s["cand"] + 1 for s in ref}
    at = set()
    for s in ref:
        if s["cand"] >= 0:
            at |= set(so.maxima(s["g2"], s["n_valid"], s["n_valid"] - 2)[0].tolist()) & {1022, 1023, 1024}
    assert at == {1022, 1023, 1024}
    return ref


def check_plateau(oracle):
    """-> (reference, the reads whose sanitised pass-2 trace has a plateau): at least two, each with neighbouring +inf gains behind the
    candidate and a poly(A) end that the recount must reproduce"""
    ref = reference(oracle, plateau_batch())
    reads = [r for r, s in enumerate(ref) if s["cand"] >= 0 and so.maxima(s["g2"], s["n_valid"], s["n_valid"] - 2)[2]]
    assert len(reads) >= 2 and set(reads) <= set(PLATEAU_READS)
    twice = [r for r in reads if np.isposinf(ref[r]["g2"][ref[r]["cand"] + 1: ref[r]["cand"] + 3]).all()]
    assert len(twice) >= 2
    assert all(ref[r]["polya_idx"] > 0 for r in reads)
    return ref, reads
