"""The batches of tests/test_gpu_gains_tile_fast.py: reads long enough for k_gains to meet several INTERIOR tiles (llr_stream.h): the
geometries of llr_stream_cases.py have L <= 2112, where tile 0 fails `tb >= start + oh` and tile 1 fails `tb + 1024 <= E - ot` for
all but full-length reads of "full".
Geometry "tall": max_obs_trace 42000, min_obs_adapter 1000, ds 10 -> L = 4100, m = 43500; a full read has tiles 1 and 2 interior in
pass 1, and tiles 1, 2 and 3 in pass 2 for any adapter index below 1024.  The conditions the batches were made for are restated in numpy here
(tests/test_gains_tile_fast_cpu.py asserts them without a GPU).  Everything returned is cached and shared: leave it unchanged."""
import functools

import numpy as np

import llr_stream_cases as lc

GEOM = "tall"
lc.GEOMS.setdefault(GEOM, (42000, 1000, 10))
TILE = 1024
N = 64
PREFIX_END = 1500     # pooled points [0, PREFIX_END) of a "prefix" read are one value: ends inside tile 1
SUFFIX_START = 2500   # pooled points [SUFFIX_START, L) of a "suffix" read are one value: reaches back into tile 2
NAMES = ("noise", "prefix", "suffix", "constant", "mixed", "dropped")


def _shape(sig, r, kind):
    g = lc.geom_of(GEOM)
    level = np.float32(70.0 + 0.5 * r)   # inside the clip range, another value per read (a minibatch of one value has no MAD)
    if kind == "prefix":
        sig[r, : g.off + PREFIX_END * g.ds] = level
    elif kind == "suffix":
        sig[r, g.off + SUFFIX_START * g.ds:] = level
    elif kind == "constant":
        sig[r, :] = level


@functools.lru_cache(maxsize=None)
def batch(name):
    g = lc.geom_of(GEOM)
    sig = lc.pool(GEOM)[:N].copy()
    if name == "mixed":   # the four reads of one workgroup: one of each kind
        for r in range(N):
            _shape(sig, r, ("noise", "prefix", "suffix", "constant")[r % 4])
    elif name not in ("noise", "dropped"):
        for r in range(N):
            _shape(sig, r, name)
    if name == "dropped":
        return lc.make(GEOM, name, [g.L] * 32 + [0] * 32, minibatch=32, sig=sig)
    return lc.make(GEOM, name, [g.L] * N, sig=sig)


def kind_of(name, r):
    return ("noise", "prefix", "suffix", "constant")[r % 4] if name == "mixed" else ("noise" if name == "dropped" else name)


def interior_tiles(n, start, oh, ot):
    """k_gains' `interior` restated: the tiles tb with tb >= start + oh and tb + 1024 <= E - ot, E = n - 1"""
    E = n - 1
    return [tb // TILE for tb in range(0, n, TILE) if tb >= start + oh and tb + TILE <= E - ot]


def variances(down, n, start):
    """var_c of the head [start, i) and tail [i, E) segments for every split point i (NaN where a segment is empty), and of the
    whole [start, E): the float64 operations of k_gains on np.cumsum's running sums"""
    x = down[:n].astype(np.float64)
    c, c2 = np.concatenate([[0.0], np.cumsum(x)]), np.concatenate([[0.0], np.cumsum(x * x)])   # c[i]: sum of x[:i]
    E = n - 1
    i = np.arange(n)
    with np.errstate(all="ignore"):
        lh, lt = (i - start).astype(np.float64), (E - i).astype(np.float64)
        vh = (c2[i] - c2[start]) / lh - ((c[i] - c[start]) / lh) ** 2
        vt = (c2[E] - c2[i]) / lt - ((c[E] - c[i]) / lt) ** 2
        vs = (c2[E] - c2[start]) / (E - start) - ((c[E] - c[start]) / (E - start)) ** 2
    return vh, vt, vs


def log_ok(v):
    """log_cr_ok: v in [2^-1022, inf)"""
    return np.isfinite(v) & (v >= 2.0 ** -1022)


def lanes_flagged(ok, tile):
    """per lane of the tile (16 consecutive points): does the fast body flag it?"""
    return ~ok[tile * TILE: (tile + 1) * TILE].reshape(64, 16).all(axis=1)


def reads_entering(ref):
    """the live reads whose whole-window variance is in the logarithm's range: vs is finite, the fast body is entered"""
    return [r for r, s in enumerate(ref) if s is not None and bool(log_ok(variances(s["down"], s["n_valid"], 0)[2]))]
