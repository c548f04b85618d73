"""Cases of the `_c_llr` best-split segmenters (reference adapted/detect/_c_llr.pyx: `_best_split` :40-64, `c_llr_detect_adapter`
:239-287, `c_llr_detect_adapter_polya` :290-365 and the trace functions :368-433), shared by ``tools/gen_c_llr_detect_golden.py``
(runs the REAL reference's Cython module in the build container) and the parity tests.  Signals come from seeds; the fixture
tests/golden/c_llr_detect.npz holds outputs only.  Python >= 3.8 syntax only."""
import numpy as np


def levels(seed, spec, noise=0.0, quant=None, nan_at=None):
    """piecewise-constant read: spec = [(level, count), ...], Gaussian noise of sd `noise`, optionally quantised to a grid of
    `quant`, with NaNs at `nan_at`; float32 values widened to float64 (the pA signal the reference reads)"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.full(n, float(v)) for v, n in spec])
    if noise:
        x = x + rng.normal(0.0, noise, x.size)
    if quant:
        x = np.round(x / quant) * quant
    x = x.astype(np.float32).astype(np.float64)
    if nan_at is not None:
        x[np.atleast_1d(nan_at)] = np.nan
    return x


def palindrome(seed, half, quant=0.5):
    """y + y[::-1] + one last sample, values on a coarse grid: every sum is exact, so the gains of the first split over
    [0, len - 1) at i and len - 1 - i are equal bit for bit -- an exact tie, which the first index wins"""
    rng = np.random.default_rng(seed)
    y = np.concatenate([np.full(half // 3, 100.0), np.full(half - half // 3, 70.0)]) + rng.normal(0, 3.0, half)
    y = np.round(y / quant) * quant
    return np.concatenate([y, y[::-1], [85.0]])


def _case(name, sig, mo=300, bt=20, mpo=50, trace=False, **kw):
    return dict(name=name, sig=sig, mo=mo, bt=bt, mpo=mpo, trace=trace, **kw)


# pA-like levels: open pore ~210, adapter ~70, poly(A) ~105, RNA ~85 with wide events
_OPEN, _ADAPT, _POLYA, _RNA = 210.0, 70.0, 105.0, 85.0


def _rna(seed, n, sd=12.0, ev=8):
    rng = np.random.default_rng(seed + 1000)
    k = n // ev + 1
    return [(float(v), ev) for v in rng.normal(_RNA, sd, k)][: max(1, n // ev)]


CASES = [
    # full adapter: open pore / adapter / poly(A) / RNA
    _case("full_adapter", dict(kind="levels", seed=1, spec=[(180.0, 400), (_ADAPT, 3000), (125.0, 800), (115.0, 6000)], noise=6.0),
          trace=True),
    _case("full_adapter_odd", dict(kind="levels", seed=2, spec=[(200.0, 351), (_ADAPT, 3001), (125.0, 801), (120.0, 6001)], noise=6.0)),
    # the open pore's step is the largest: the first split is the adapter's start
    _case("open_pore_first", dict(kind="levels", seed=16, spec=[(_OPEN, 900), (_ADAPT, 3000), (_POLYA, 800)] + _rna(16, 6000), noise=6.0)),
    # partial adapter: the read starts inside the adapter, which steps down once (medians[0] < mean)
    _case("partial_adapter", dict(kind="levels", seed=3, spec=[(_ADAPT - 10, 700), (_ADAPT - 25, 2200), (_POLYA + 60, 900), (_POLYA, 3000)],
                                  noise=4.0), trace=True),
    # the first split is the adapter START: a long high stretch, then the adapter, then a short stretch at the adapter level
    _case("first_split_adapter_start", dict(kind="levels", seed=4, spec=[(_OPEN, 4000), (_ADAPT, 2000), (_ADAPT + 12, 1500)], noise=5.0),
          trace=True),
    # (0, 0) by decision: no drop after the first split, and the head splits better than the tail
    _case("none_by_decision", dict(kind="levels", seed=5, spec=[(100.0, 1000), (90.0, 3000), (60.0, 3000)], noise=3.0), mo=200),
    # the first split finds nothing: a constant read (every gain NaN)
    _case("constant", dict(kind="levels", seed=6, spec=[(_RNA, 5000)]), trace=True),
    # both fallbacks: a noiseless step, head and tail constant (their gains NaN) -> x_head = 1, x_tail = x_first + 1
    _case("both_fallbacks", dict(kind="levels", seed=7, spec=[(_ADAPT, 7), (_POLYA, 6)]), mo=5, bt=2, mpo=1),
    # poly(A) not found: nothing left to split after the adapter (min_obs_polya longer than the rest)
    _case("polya_not_found", dict(kind="levels", seed=8, spec=[(_OPEN, 900), (_ADAPT, 3000), (_POLYA, 300)] + _rna(8, 600), noise=6.0),
          mpo=5000),
    # a NaN in the last sample, which no split sees: the last segment's median is NaN (and so the mean of the four)
    _case("nan_last_sample", dict(kind="levels", seed=9, spec=[(180.0, 400), (_ADAPT, 3000), (125.0, 800), (115.0, 4000)], noise=6.0,
                                  nan_at=-1), trace=True),
    # a NaN inside the read: every sum from there on is NaN, and so is every gain
    _case("nan_inside", dict(kind="levels", seed=17, spec=[(150.0, 300), (_ADAPT, 3000), (_POLYA, 800)] + _rna(17, 4000), noise=6.0,
                             nan_at=2000), trace=True),
    # 0.5 pA-quantised, with exact gain ties
    _case("quantised", dict(kind="levels", seed=10, spec=[(180.0, 400), (_ADAPT, 3000), (125.0, 800), (115.0, 4000)], noise=6.0,
                            quant=0.5)),
    _case("quantised_coarse", dict(kind="levels", seed=18, spec=[(_OPEN, 900), (_ADAPT, 3000), (_POLYA, 800)] + _rna(18, 4000), noise=6.0,
                                   quant=8.0)),
    _case("exact_tie", dict(kind="palindrome", seed=11, half=1500), mo=100, bt=10),
    # tiny reads, zero offsets
    _case("n1", dict(kind="levels", seed=12, spec=[(_RNA, 1)]), mo=0, bt=0, mpo=0),
    _case("n2", dict(kind="raw", values=[80.0, 90.0]), mo=0, bt=0, mpo=0),
    _case("n3", dict(kind="raw", values=[80.0, 90.0, 85.0]), mo=0, bt=0, mpo=0, trace=True),
    _case("n3_offsets", dict(kind="raw", values=[80.0, 90.0, 85.0]), mo=1, bt=1, mpo=1),
    _case("zero_offsets", dict(kind="levels", seed=13, spec=[(_OPEN, 200), (_ADAPT, 700), (_POLYA, 150)] + _rna(13, 800), noise=6.0),
          mo=0, bt=0, mpo=0, trace=True),
    _case("shorter_than_min_obs", dict(kind="levels", seed=14, spec=[(_ADAPT, 200), (_POLYA, 200)], noise=5.0), mo=300, bt=20),
    # one long read
    _case("long_200k", dict(kind="levels", seed=15, spec=[(_OPEN, 3000), (_ADAPT, 9000), (_POLYA, 2500)] + _rna(15, 185500), noise=7.0),
          mo=1000, bt=50, mpo=100),
]

# `_best_split` on given ranges of a case's sums: (case name, start, end, offset_head, offset_tail)
SPLITS = [
    ("full_adapter", 0, 10199, 320, 20),
    ("full_adapter", 900, 10199, 0, 0),
    ("full_adapter", 0, 0, 0, 0),
    ("full_adapter", 100, 4000, 3000, 3000),
    ("constant", 0, 4999, 5, 5),
    ("exact_tie", 0, 3000, 10, 10),
    ("n3", 0, 2, 0, 0),
    ("nan_inside", 0, 8099, 5, 5),
    ("nan_inside", 0, 1990, 5, 5),
]


def signal_of(case):
    s = case["sig"]
    if s["kind"] == "levels":
        return levels(s["seed"], s["spec"], s.get("noise", 0.0), s.get("quant"), s.get("nan_at"))
    if s["kind"] == "palindrome":
        return palindrome(s["seed"], s["half"])
    return np.asarray(s["values"], dtype=np.float64)


def by_name(name):
    return next(c for c in CASES if c["name"] == name)
