"""Cases of the reference's MVS poly(A) module (adapted/detect/mvs.py), shared by ``tools/gen_mvs_module_golden.py`` (runs the
REAL reference's mvs.py with the real bottleneck 1.3.2 in the build container) and the parity tests.  Every input comes from a
seed; the fixture tests/golden/mvs_module.npz holds outputs only, encoded by `enc` (type and exact value of every returned item,
or the exception raised).  Python >= 3.8 syntax only."""
import inspect

import numpy as np

# the names adapted/detect/mvs.py defines (the fixture records them from the reference module itself)
NAMES = ["mean_var_shift_polyA_check", "mean_var_shift_polyA_detect", "mean_var_shift_polyA_detect_at_loc"]

# the dtypes every case runs in.  "i32": integer input (the reference's bottleneck 1.3.2 takes its native path for int32 / int64;
# int16 goes to its pure-Python fallback, which fails under numpy >= 1.24 -- the parity tests feed int16 too and expect the int32
# results: this module widens any integer input to float64)
DTYPES = ("f32", "f64", "i32")


def pa_read(seed, n, adapter=(2600, 3400), polya=(400, 700), decoys=0, nan_at=(), adapter_level=75.0, polya_level=110.0,
            polya_sd=2.0, rna_level=100.0):
    """a calibrated read in pA (float64): open adapter (low, noisy), poly(A) (high, quiet), RNA (events); `decoys` short quiet
    stretches at the poly(A) level inside the adapter; NaN at `nan_at`.  Returns (signal, adapter end, poly(A) end)"""
    rng = np.random.default_rng(seed)
    a = int(rng.integers(*adapter)) if adapter[1] > adapter[0] else adapter[0]
    p = int(rng.integers(*polya)) if polya[1] > polya[0] else polya[0]
    x = np.empty(n, dtype=np.float64)
    x[:min(a, n)] = rng.normal(adapter_level, 6.0, min(a, n))
    for _ in range(decoys):
        d0 = int(rng.integers(min(a // 2, 1200), max(a - 400, min(a // 2, 1200) + 1)))
        x[d0:min(d0 + 150, n)] = rng.normal(polya_level, polya_sd, max(0, min(150, n - d0)))
    e = min(n, a + p)
    if e > a:
        x[a:e] = rng.normal(polya_level, polya_sd, e - a)
    if n > e:
        lv = np.repeat(rng.normal(rna_level, 12.0, (n - e) // 8 + 1), 8)[:n - e]
        x[e:] = lv + rng.normal(0.0, 3.0, n - e)
    for i in nan_at:
        x[i] = np.nan
    return x, a, a + p


def as_dtype(x, dt):
    if dt == "f32":
        return x.astype(np.float32)
    if dt == "f64":
        return x.copy()
    return np.round(np.nan_to_num(x, nan=0.0)).astype(np.int32 if dt == "i32" else np.int16)


def C(name, seed, n, ae=None, pe=None, loc=None, mvs=None, stream=None, **kw):
    return dict(name=name, seed=seed, n=n, ae=ae, pe=pe, loc=loc, mvs=mvs or {}, stream=stream or {}, sig=kw)


# ae / pe / loc: None -> the read's true adapter end / poly(A) end / adapter end; an int -> that position; a string "+k" -> true + k
CASES = [
    C("clean", 1, 9000),
    C("clean_b", 2, 8000),
    C("clean_c", 3, 10000, polya=(900, 1200)),
    C("decoys", 4, 12000, decoys=3),
    C("decoys_b", 5, 11000, decoys=2, polya=(250, 320)),
    C("short_read", 6, 2700, adapter=(1500, 1800)),
    C("match_at_offset", 7, 7000, adapter=(2300, 2301), polya=(900, 901)),
    C("post_loc", 8, 3100, adapter=(2900, 2901), polya=(600, 601)),
    C("clipped_windows", 9, 3900, adapter=(2900, 2901), polya=(600, 601)),
    C("nan_adapter", 10, 9000, nan_at=(1200, 2000, 2001, 2750)),
    C("nan_polya", 11, 9000, adapter=(3000, 3001), nan_at=(3150, 3160)),
    C("nan_rna", 12, 9000, adapter=(3000, 3001), polya=(500, 501), nan_at=(4000, 5200)),
    C("no_polya", 13, 8000, polya=(0, 1), polya_level=75.0),
    C("low_polya", 14, 8000, polya_level=85.0),
    C("noisy_polya", 15, 8000, polya_sd=5.0),
    C("index_error", 16, 8000, polya=(0, 1), polya_level=75.0, mvs=dict(search_window=50)),
    C("loc_past_end", 17, 6000, loc=6400, ae=6400, pe=6600),
    C("loc_at_end", 18, 6000, loc=6000),
    C("loc_small", 19, 6000, loc=40, ae=40, pe=300),
    C("short_slice", 20, 8000, pe="+80"),
    C("very_short_slice", 21, 8000, pe="+15"),
    C("tiny_slice", 22, 8000, pe="+2"),
    C("pe_before_ae", 23, 8000, pe="-50"),
    C("ae_zero", 24, 8000, ae=0),
    C("less_signal", 25, 4000, adapter=(3000, 3001), polya=(400, 401)),
    C("pe_past_end", 26, 5000, adapter=(4700, 4701), ae=4950, pe=5400),
    C("ae_past_end", 27, 5000, ae=5200, pe=5400, loc=4990),
    C("long_windows", 28, 12000, polya=(1500, 1800), mvs=dict(pA_var_window=400, pA_mean_window=300),
      stream=dict(pA_var_window=400, pA_mean_window=300)),
    C("narrow_ranges", 29, 9000, mvs=dict(pA_mean_range=(100.0, 120.0), polyA_local_range=(0.0, 4.0)),
      stream=dict(polyA_local_range=(0.0, 4.0), search_increment_step=37)),
    C("small_stream", 30, 4000, adapter=(1200, 1500), stream=dict(min_obs_adapter=600, median_shift_window=500, min_obs_post_loc=150)),
    C("small_stream_b", 31, 3000, adapter=(900, 1100), decoys=2, stream=dict(min_obs_adapter=400, median_shift_window=400)),
    C("window_one", 32, 5000, mvs=dict(pA_mean_window=1, pA_var_window=1, search_window=40)),
    C("rna_like_polya", 33, 9000, rna_level=110.0),
]


def by_name(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def _pos(v, true):
    if v is None:
        return int(true)
    if isinstance(v, str):
        return int(true) + int(v)
    return int(v)


def inputs(case):
    """(signal float64, adapter_end, polya_end, loc)"""
    x, a, p = pa_read(case["seed"], case["n"], **case["sig"])
    ae = _pos(case["ae"], a)
    pe = _pos(case["pe"], p if case["pe"] is None else ae)
    loc = _pos(case["loc"], a)
    return x, ae, pe, loc


def mvs_params(cls, case):
    p = cls()
    for k, v in case["mvs"].items():
        setattr(p, k, v)
    return p


def stream_params(cls, case):
    p = cls()
    for k, v in case["stream"].items():
        setattr(p, k, v)
    return p


# every call a case makes: (key, function name, keyword flags)
CALLS = ([("check.rv%d.lso%d.ws%d" % (rv, lso, ws), "check", dict(return_values=bool(rv), less_signal_ok=bool(lso), windowed_stats=bool(ws)))
          for rv in (0, 1) for lso in (0, 1) for ws in (0, 1)]
         + [("at_loc.rv%d.lso%d" % (rv, lso), "at_loc", dict(return_values=bool(rv), less_signal_ok=bool(lso))) for rv in (0, 1) for lso in (0, 1)]
         + [("detect", "detect", {})])


def call(mod, fn, x, ae, pe, loc, mp, sp, kw):
    """one call of module `mod` (the reference's mvs, adapted_amd.detect.mvs or the restatement's wrapper) -> its encoded result"""
    try:
        if fn == "check":
            r = mod.mean_var_shift_polyA_check(x, ae, pe, mp, **kw)
        elif fn == "at_loc":
            r = mod.mean_var_shift_polyA_detect_at_loc(x, loc, mp, **kw)
        else:
            r = mod.mean_var_shift_polyA_detect(x, sp)
    except (IndexError, ValueError) as e:
        return "raise %s: %s" % ("IndexError" if isinstance(e, IndexError) else "ValueError", e)
    return enc(r)


def _tname(v):
    if isinstance(v, np.generic):
        return "np." + v.dtype.name
    return type(v).__name__


def enc(v):
    """a returned value with its type, exactly (floats as hex)"""
    if isinstance(v, tuple):
        return "(" + ", ".join(enc(e) for e in v) + ")"
    if isinstance(v, np.ndarray):
        return "ndarray[%s]%s" % (v.dtype.name, v.tolist())
    if isinstance(v, (float, np.floating)):
        return "%s:%s" % (_tname(v), float(v).hex())
    if isinstance(v, np.generic):
        return "%s:%r" % (_tname(v), v.item())
    return "%s:%r" % (_tname(v), v)


def signature_rows(mod):
    """(name, [(parameter, kind, default)]) of the module's functions; config defaults by class name"""
    rows = []
    for nm in NAMES:
        sig = inspect.signature(getattr(mod, nm))
        ps = []
        for p in sig.parameters.values():
            d = p.default
            if d is inspect.Parameter.empty:
                ds = "-"
            elif type(d).__name__.endswith("Config"):
                ds = type(d).__name__.lower() + "()"  # (the class, by name: MVSPolyAConfig here is generated as MvsPolyaConfig)
            else:
                ds = repr(d)
            ps.append("%s:%s:%s" % (p.name, p.kind.name, ds))
        rows.append(nm + "(" + ", ".join(ps) + ")")
    return rows
