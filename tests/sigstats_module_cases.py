"""Cases of the reference's signal statistics modules (adapted/partition/signal_partitions.py, adapted/detect/normalize.py,
downscale.py, real_range.py, anomalies.py), shared by ``tools/gen_sigstats_module_golden.py`` (runs the REAL reference) and the
parity tests.  Every input comes from a seed; the
fixture tests/golden/sigstats_module.npz holds outputs only, encoded by `enc` (type and exact value of every returned item, or
the exception raised).  Python >= 3.8 syntax only."""
import dataclasses
import hashlib
import inspect

import numpy as np

# the names adapted/partition/signal_partitions.py defines (the fixture records them from the reference module itself)
NAMES = ["Partition", "Partitions", "calc_partition_stats", "calc_partitions", "calc_partitions_from_vals"]

# the dtypes every case runs in.  "i32": integer input (numpy widens it to float64 in all four statistics; the parity tests feed
# int16 too and expect the int32 results)
DTYPES = ("f32", "f64", "i32")


def read(seed, n, nan_at=None, quantised=False, constant_adapter=False):
    """a calibrated read in pA (float64): adapter (level and noise drawn from a few), poly(A) (110 +- 2), RNA (events), open-pore
    spikes at 230 +- 8 pA inside the adapter; one read in ten with three NaN samples, one in ten quantised to 0.18 pA, one in
    twenty with a constant adapter -- or, with the keywords, exactly that.  Returns (signal, adapter end, poly(A) end)"""
    rng = np.random.default_rng(seed)
    a = int(rng.integers(900, 3600))
    p = int(rng.integers(100, 1500))
    lvl = float(rng.choice([45.0, 75.0, 75.0, 75.0, 88.0]))
    sd = float(rng.choice([2.5, 6.0, 6.0, 9.0, 16.0]))
    x = np.empty(n)
    a = min(a, n)
    e = min(n, a + p)
    x[:a] = rng.normal(lvl, sd, a)
    x[a:e] = rng.normal(110.0, 2.0, e - a)
    lv = np.repeat(rng.normal(100.0, 12.0, (n - e) // 8 + 1), 8)[:n - e]
    x[e:] = lv + rng.normal(0, 3.0, n - e)
    k = int(rng.choice([0, 0, 1, 3, 40]))
    for _ in range(k):
        s = int(rng.integers(0, max(a - 30, 1)))
        w = int(rng.integers(1, 25))
        x[s:s + w] = rng.normal(230.0, 8.0, len(x[s:s + w]))
    u = rng.random()
    if nan_at is not None or quantised or constant_adapter:
        u = 1.0
    if u < 0.1:
        x[rng.integers(0, n, 3)] = np.nan
    elif u < 0.2 or quantised:
        x = np.round(x / 0.18) * 0.18
    elif u < 0.25:
        x[:a] = 75.0
    if constant_adapter:
        x[:a] = 75.0
    for i in nan_at or ():
        x[i] = np.nan
    return x, a, e


def mixed_read(r):
    """read r of the mixed batches: (signal float64, adapter_end, polya_end) -- lengths 2500 - 20 000, boundaries within +-40 of
    the true ones for 80 % of the reads, otherwise anywhere up to 400 past the end"""
    rng = np.random.default_rng(10_000 + r)
    n = int(rng.integers(2500, 20000))
    x, a, e = read(r, n)
    ae = a + int(rng.integers(-40, 40)) if rng.random() < 0.8 else int(rng.integers(0, n + 400))
    pe = e + int(rng.integers(-40, 40)) if rng.random() < 0.8 else ae + int(rng.integers(-10, 400))
    return x, max(ae, 0), max(pe, 0)


def as_dtype(x, dt):
    if dt == "f32":
        return x.astype(np.float32)
    if dt == "f64":
        return x.copy()
    return np.round(np.nan_to_num(x, nan=0.0)).astype(np.int32 if dt == "i32" else np.int16)


# the sample counts every selection and summation branch is taken at: below / at / above numpy's 8-accumulator leaf, its
# 128-element leaf, its 8192-element buffer; odd and even; a whole long read
COUNTS = (1, 2, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 199999, 200000)


def C(name, seed, n, calls, **kw):
    return dict(name=name, seed=seed, n=n, calls=calls, sig=kw)


def _vals(*a):
    return ("vals",) + a


# calls: ("stats", start, end) -> calc_partition_stats; ("vals", adapter_start, adapter_end, polya_end, polya_truncated) ->
# calc_partitions_from_vals; ("parts", adapter_start, adapter_end, polya_end) -> calc_partitions of a Boundaries.
# Positions: an int; None; "a" / "e" / "n" (+k): the read's true adapter end / poly(A) end / size (+ k)
CASES = [
    C("counts", 1, 210000, [("stats", 1000, 1000 + c) for c in COUNTS] + [("stats", 0, 210000), ("parts", 0, "a", "e")]),
    C("counts_tail", 2, 9000, [("stats", 9000 - c, 9000) for c in COUNTS if c <= 8193]),
    C("clean", 3, 12000, [_vals(0, "a", "e", False), _vals(0, "a", "e"), ("parts", 0, "a", "e"), _vals(40, "a+7", "e-9", False)]),
    C("quantised", 4, 12000, [_vals(0, "a", "e", False), ("stats", 0, 12000), ("stats", 5, 4096), ("stats", 6, 4096)], quantised=True),
    C("constant", 5, 9000, [_vals(0, "a", "e", False), ("stats", 10, 11), ("stats", 10, 12), ("stats", 0, "a+1")], constant_adapter=True),
    C("nan_adapter", 6, 9000, [_vals(0, "a", "e", False), ("stats", 0, 500), ("stats", 500, 501), ("stats", 501, 900)], nan_at=(500,)),
    C("nan_polya", 7, 9000, [_vals(0, 3700, 3800, False)], nan_at=(3750,)),
    C("nan_rna", 8, 9000, [_vals(0, "a", "e", False), ("stats", 6000, 6002)], nan_at=(6001,)),
    C("nan_tail", 9, 9000, [_vals(0, "a", "e", False), ("stats", 8999, 9000), ("stats", 8990, 9400)], nan_at=(8999,)),
    C("none_positions", 10, 8000, [_vals(None, "a", "e", False), _vals(0, None, "e", False), _vals(0, "a", None, False),
                                   _vals(None, None, None, False), ("stats", None, 10), ("stats", 10, None), ("stats", None, None)]),
    C("truncated", 11, 8000, [_vals(0, "a", "e", True), _vals(0, "a", None, True), _vals(0, "a", "e", None)]),
    C("end_before_start", 12, 8000, [_vals(0, "a", "a-5", False), _vals(300, 300, "e", False), ("stats", 10, 10), ("stats", 10, 9),
                                     ("stats", 0, 0)]),
    C("beyond", 13, 6000, [_vals(0, "a", "n+300", False), _vals(0, "n+20", "n+300", False), _vals(0, "a", "n", False),
                           ("stats", "n", "n+10"), ("stats", "n-1", "n+10"), ("stats", "n+5", "n+6"), ("stats", 0, "n+1")]),
    C("empty_read", 14, 0, [("stats", 0, 5), _vals(0, 0, 0, False), _vals(0, 3, 9, False)]),
    C("tiny_read", 15, 3, [("stats", 0, 3), ("stats", 1, 3), _vals(0, 1, 2, False)]),
]


def by_name(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def inputs(case):
    """(signal float64, names: the positions "a", "e", "n" stand for)"""
    if case["n"] < 8:
        x = np.random.default_rng(case["seed"]).normal(80.0, 5.0, case["n"])
        return x, dict(a=min(1, case["n"]), e=min(2, case["n"]), n=case["n"])
    x, a, e = read(case["seed"], case["n"], **case["sig"])
    return x, dict(a=a, e=e, n=case["n"])


def position(v, names):
    if v is None or isinstance(v, int):
        return v
    for sep in ("+", "-"):
        if sep in v:
            base, k = v.split(sep)
            return names[base] + int(sep + k)
    return names[v]


def call_key(i, c):
    return "%02d.%s" % (i, c[0])


def call(mod, boundaries_cls, x, names, c):
    """one call of module `mod` (the reference's, adapted_amd.partition.signal_partitions or the restatement) -> the encoded
    result, with its to_dict"""
    pos = [position(v, names) if not isinstance(v, bool) else v for v in c[1:]]
    try:
        if c[0] == "stats":
            r = mod.calc_partition_stats(x, pos[0], pos[1])
        elif c[0] == "vals":
            r = mod.calc_partitions_from_vals(x, *pos)
        else:
            r = mod.calc_partitions(x, boundaries_cls(pos[0], pos[1], pos[2]))
    except (IndexError, ValueError, TypeError) as e:
        return "raise %s: %s" % (type(e).__name__, e)
    return enc(r) + " " + enc(r.to_dict("p")) + " " + enc(r.to_dict())


def _tname(v):
    if isinstance(v, np.generic):
        return "np." + v.dtype.name
    return type(v).__name__


def enc(v):
    """a returned value with its type, exactly (floats as hex)"""
    if dataclasses.is_dataclass(v):
        return "%s(%s)" % (type(v).__name__, ", ".join("%s=%s" % (f.name, enc(getattr(v, f.name))) for f in dataclasses.fields(v)))
    if isinstance(v, dict):
        return "{" + ", ".join("%s: %s" % (k, enc(e)) for k, e in v.items()) + "}"
    if isinstance(v, tuple):
        return "(" + ", ".join(enc(e) for e in v) + ")"
    if isinstance(v, np.ndarray):
        if v.size <= 64:
            return "ndarray[%s]%s%s" % (v.dtype.name, v.shape, [enc(e) if isinstance(e, np.floating) else e.item() for e in v.reshape(-1)])
        # a long array: dtype, shape, a digest of its bytes (every NaN made the same one) and a few probe values
        a = np.ascontiguousarray(v).copy()
        if a.dtype.kind == "f":
            a[a != a] = np.nan
        probes = [enc(a.reshape(-1)[i]) for i in np.linspace(0, a.size - 1, 7).astype(int)]
        return "ndarray[%s]%s sha256:%s %s" % (a.dtype.name, a.shape, hashlib.sha256(a.tobytes()).hexdigest(), probes)
    if isinstance(v, (float, np.floating)):
        return "%s:%s" % (_tname(v), "nan" if v != v else float(v).hex())
    if isinstance(v, np.generic):
        return "%s:%r" % (_tname(v), v.item())
    return "%s:%r" % (_tname(v), v)


def signature_rows(mod, names=None):
    """the module's functions with (parameter, kind, default), its dataclasses with their fields and methods"""
    rows = []
    for nm in names or NAMES:
        obj = getattr(mod, nm)
        if inspect.isclass(obj):
            rows.append("%s[%s]" % (nm, ", ".join(f.name for f in dataclasses.fields(obj))))
            obj, nm = obj.to_dict, nm + ".to_dict"
        ps = []
        for p in inspect.signature(obj).parameters.values():
            ps.append("%s:%s:%s" % (p.name, p.kind.name, "-" if p.default is inspect.Parameter.empty else repr(p.default)))
        rows.append(nm + "(" + ", ".join(ps) + ")")
    return rows


# ---- the detect modules: normalize, downscale, real_range, anomalies ------------------------------------------------------------
# the names each module defines (the fixture records them from the reference modules themselves)
DETECT_NAMES = {"normalize": ["med_mad", "clip_signal", "normalize_signal"],
                "downscale": ["efficient_average_pooling", "downscale_signal"],
                "real_range": ["real_range_check"],
                "anomalies": ["find_open_pores"]}
POOLS = (2, 3, 7, 10, 20, 32)


def minibatch(seed, rows, m):
    """a [rows, m] minibatch of reads with NaN behind each read's end (float64)"""
    rng = np.random.default_rng(seed)
    X = np.full((rows, m), np.nan)
    for r in range(rows):
        k = m if r % 4 == 0 else int(rng.integers(m // 3, m))
        X[r, :k] = read(seed * 100 + r, m, quantised=(r % 5 == 1))[0][:k]
    return X


def spikes(seed, n, where, level=230.0, base=80.0):
    """a flat noisy stretch with open-pore spikes: `where` lists (start, width)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(base, 5.0, n)
    for s, w in where:
        x[s:s + w] = rng.normal(level, 4.0, len(x[s:s + w]))
    return x


def two_levels(seed, n, first, last, sd=4.0, tail_sd=None, nan_at=()):
    """`first` pA at the start, `last` pA at the end, a ramp in between; noise sd (the last 40 %: tail_sd)"""
    rng = np.random.default_rng(seed)
    x = np.linspace(first, last, n) + rng.normal(0.0, sd, n)
    x[:n // 4] = first + rng.normal(0.0, sd, n // 4)
    k = n - (2 * n) // 5
    x[k:] = last + rng.normal(0.0, sd if tail_sd is None else tail_sd, n - k)
    for i in nan_at:
        x[i] = np.nan
    return x


SIGNALS = {
    "read": lambda seed, n, **kw: read(seed, n, **kw)[0],
    "minibatch": lambda seed, n, rows=8, **kw: minibatch(seed, rows, n),
    "allnan": lambda seed, n: np.full(n, np.nan),
    "const": lambda seed, n: np.full(n, 75.0),
    "normal": lambda seed, n, shape=None: np.random.default_rng(seed).normal(90.0, 11.0, n).reshape(shape or (n,)),
    "empty2d": lambda seed, n: np.zeros((0, 5)),
    "spikes": spikes,
    # samples that ARE float32(80.1) and float32(80.3): inside [80.1, 80.3] only when the bounds are rounded to float32 too
    "edge": lambda seed, n: np.array([float(np.float32(80.1)), 80.2, 50.0, float(np.float32(80.3)), 80.2, 50.0] * n),
    "two_levels": two_levels,
}


def D(module, name, signal, seed, n, calls, dtypes=("f32", "f64"), **kw):
    return dict(module=module, name=name, signal=signal, seed=seed, n=n, calls=calls, dtypes=dtypes, sig=kw)


_NORM = [("med_mad", False), ("med_mad", True), ("normalize", 5.0, False), ("normalize", 5.0, True), ("normalize", 2.0, False),
         ("clip", 3.0, 80.1, 6.3)]
_RR = [("rr", {}, False), ("rr", {}, True)]
_ALL3 = ("f32", "f64", "i32")
DETECT_CASES = [
    # normalize.py: odd / even counts, ties, MAD 0, NaN with and without with_nan, one population of any rank, both regimes
    D("normalize", "read_odd", "read", 21, 9001, _NORM + [("normalize", 0.0, False), ("normalize", -1.0, False)]),
    D("normalize", "read_even", "read", 22, 9000, _NORM),
    D("normalize", "read_200k", "read", 23, 200000, _NORM),
    D("normalize", "read_300k", "read", 24, 300001, _NORM),
    D("normalize", "quantised", "read", 25, 12000, _NORM, quantised=True),
    D("normalize", "nan_read", "read", 26, 9000, _NORM, nan_at=(5, 4000, 8999)),
    D("normalize", "constant", "const", 27, 100, _NORM),
    D("normalize", "mostly_constant", "read", 28, 4000, _NORM + [("stretch", 0, 700)], constant_adapter=True),
    D("normalize", "allnan", "allnan", 29, 50, _NORM),
    D("normalize", "empty", "normal", 30, 0, _NORM),
    D("normalize", "empty2d", "empty2d", 31, 0, _NORM),
    D("normalize", "one", "normal", 32, 1, _NORM),
    D("normalize", "two", "normal", 33, 2, _NORM),
    D("normalize", "minibatch", "minibatch", 34, 3000, _NORM, rows=8),
    D("normalize", "minibatch_big", "minibatch", 35, 6000, _NORM, rows=64),
    D("normalize", "rank3", "normal", 36, 2 * 3 * 50, _NORM, shape=(2, 3, 50)),
    # downscale.py: every pool size with and without a ragged last block, a pool larger than a leaf of numpy's sum, not 2-D
    D("downscale", "exact", "normal", 41, 5 * 6720, [("pool", p) for p in POOLS] + [("downscale", 2), ("downscale", None)], shape=(5, 6720)),
    D("downscale", "ragged", "normal", 42, 4 * 6719, [("pool", p) for p in POOLS] + [("pool", 200), ("pool", 7000), ("downscale", 10)], shape=(4, 6719)),
    D("downscale", "one_col", "normal", 43, 3, [("pool", 2), ("pool", 1)], shape=(3, 1)),
    D("downscale", "nan_tails", "minibatch", 44, 1001, [("pool", 10), ("pool", 3)], rows=6),
    D("downscale", "no_rows", "empty2d", 45, 0, [("pool", 2)]),
    D("downscale", "not_2d", "normal", 46, 64, [("pool", 2), ("downscale", 2)]),
    D("downscale", "rank3", "normal", 47, 2 * 4 * 8, [("pool", 2)], shape=(2, 4, 8)),
    # real_range.py: too short, each mean failing, the local range failing and passing, max_obs_local_range longer / shorter
    D("real_range", "pass", "two_levels", 51, 4000, _RR + [("rr", dict(max_obs_local_range=9000), True), ("rr", dict(max_obs_local_range=700), True)], _ALL3, first=75.0, last=100.0, tail_sd=7.0),
    D("real_range", "pass_long", "two_levels", 52, 12000, _RR + [("rr", dict(mean_window=1), True)], _ALL3, first=80.0, last=95.0, tail_sd=8.0),
    D("real_range", "too_short", "two_levels", 53, 599, _RR + [("rr", dict(mean_window=299), True)], _ALL3, first=75.0, last=100.0),
    D("real_range", "just_enough", "two_levels", 54, 600, _RR, _ALL3, first=75.0, last=100.0, tail_sd=7.0),
    D("real_range", "start_low", "two_levels", 55, 4000, _RR, _ALL3, first=40.0, last=100.0, tail_sd=7.0),
    D("real_range", "end_high", "two_levels", 56, 4000, _RR, _ALL3, first=75.0, last=130.0, tail_sd=7.0),
    D("real_range", "range_small", "two_levels", 57, 4000, _RR, _ALL3, first=90.0, last=92.0, sd=1.0),
    D("real_range", "range_large", "two_levels", 58, 4000, _RR, _ALL3, first=75.0, last=100.0, tail_sd=30.0),
    D("real_range", "open_ranges", "two_levels", 59, 4000, [("rr", dict(mean_start_range=(None, None), mean_end_range=(None, 500.0), local_range=(0.0, None)), True)], _ALL3, first=20.0, last=300.0),
    D("real_range", "nan_start", "two_levels", 60, 4000, _RR, ("f32", "f64"), first=75.0, last=100.0, tail_sd=7.0, nan_at=(10,)),
    D("real_range", "nan_tail", "two_levels", 61, 4000, _RR, ("f32", "f64"), first=75.0, last=100.0, tail_sd=7.0, nan_at=(3000,)),
    D("real_range", "quantised", "read", 62, 3000, _RR + [("rr", dict(mean_end_range=(None, None)), True)], _ALL3, quantised=True),
    # anomalies.py: none, one, a run closer than min_obs_diff (the last position alone), many, a range with an upper bound
    D("anomalies", "none", "spikes", 71, 3000, [("op", (200.0, None), 10)], _ALL3, where=()),
    D("anomalies", "one", "spikes", 72, 3000, [("op", (200.0, None), 10), ("op", None, None)], _ALL3, where=((1500, 1),)),
    D("anomalies", "one_run", "spikes", 73, 3000, [("op", (200.0, None), 10), ("op", (200.0, None), 1), ("op", (200.0, None), 0)], _ALL3, where=((700, 9),)),
    D("anomalies", "two_close", "spikes", 74, 3000, [("op", (200.0, None), 10), ("op", (200.0, None), 3)], _ALL3, where=((700, 1), (704, 1))),
    D("anomalies", "many", "spikes", 75, 20000, [("op", (200.0, None), 10), ("op", (200.0, None), 200), ("op", (225.0, 235.0), 10), ("op", (None, 60.0), 5)], _ALL3,
      where=tuple((300 * k + 17, 1 + k % 24) for k in range(1, 60))),
    D("anomalies", "first_and_last", "spikes", 76, 2000, [("op", (200.0, None), 10)], _ALL3, where=((0, 1), (63, 2), (64, 1), (127, 1), (128, 1), (1999, 1))),
    D("anomalies", "nan", "spikes", 77, 3000, [("op", (None, None), 500), ("op", (200.0, None), 10)], ("f32", "f64"), where=((100, 3), (900, 2))),
    D("anomalies", "bound_not_float32", "edge", 78, 4, [("op", (80.1, 80.3), 1), ("op", (80.1, 80.3), 2)], _ALL3),
    D("anomalies", "empty", "normal", 79, 0, [("op", (200.0, None), 10)], _ALL3),
    D("anomalies", "read", "read", 4, 9000, [("op", (200.0, None), 10)], _ALL3),
]


def detect_case(module, name):
    for c in DETECT_CASES:
        if c["module"] == module and c["name"] == name:
            return c
    raise KeyError((module, name))


def detect_input(case):
    x = SIGNALS[case["signal"]](case["seed"], case["n"], **case["sig"])
    if case["module"] == "anomalies" and case["name"] == "nan":
        x[[5, 101, 2999]] = np.nan
    return x


def detect_key(case, dt, i, c):
    return "%s.%s.%s.%02d.%s" % (case["module"], case["name"], dt, i, c[0])


def rr_params(cls, over):
    p = cls()
    for k, v in over.items():
        setattr(p, k, v)
    return p


def detect_call(mods, rr_cls, x, c):
    """one call of the module set `mods` (an object with the functions of DETECT_NAMES as attributes) -> the encoded result"""
    try:
        if c[0] == "med_mad":
            r = mods.med_mad(x, c[1])
        elif c[0] == "normalize":
            r = mods.normalize_signal(x, c[1], c[2])
        elif c[0] == "stretch":  # (a constant stretch of a read: MAD 0)
            r = mods.normalize_signal(x[c[1]:c[2]])
        elif c[0] == "clip":
            r = mods.clip_signal(x, c[1], c[2], c[3])
        elif c[0] == "pool":
            r = mods.efficient_average_pooling(x, c[1])
        elif c[0] == "downscale":
            r = mods.downscale_signal(x) if c[1] is None else mods.downscale_signal(x, c[1])
        elif c[0] == "rr":
            r = mods.real_range_check(x, rr_params(rr_cls, c[1]), c[2]) if c[2] else mods.real_range_check(x, rr_params(rr_cls, c[1]))
        else:
            r = mods.find_open_pores(x) if c[1] is None else mods.find_open_pores(x, c[1], c[2])
    except (IndexError, ValueError, TypeError) as e:
        return "raise %s: %s" % (type(e).__name__, e)
    return enc(r)
