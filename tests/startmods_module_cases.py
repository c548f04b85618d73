"""Cases of the reference's start-peak and adapter-start modules (adapted/detect/start_peak.py, adapter_start.py), shared by
``tools/gen_startmods_module_golden.py`` (runs the REAL reference with the real bottleneck 1.3.2 and pandas in the build
container) and the parity tests.  Every input comes from a seed; the fixture tests/golden/startmods_module.npz holds outputs
only.  Python >= 3.8 syntax only."""
import inspect

import numpy as np

NAMES = {"start_peak": ["detect_rna_start_peak"], "adapter_start": ["moving_mean_adapter_start_detect"]}

# ---------------------------------------------------------------- adapter start
AS_DTYPES = ("f32", "f64", "i32")
AS_PARAMS = [(1, 0), (2, 0), (7, 5), (100, 2500), (101, 2500), (100, 0)]  # (window, min_obs_adapter)


def as_diff_sizes(w):
    """the sizes of `difference` (L = len - min_obs_adapter - window) every parameter pair runs at"""
    return [0, 1, w - 1, w, w + 1, 2 * w + 3, 511, 512, 513, 1300]


def step_read(seed, n, split=None, hi=128.0, lo=64.0, spread=8):
    """a read on the 0.25 pA grid (float64): a high level, from `split` on (default: somewhere in the first half) a lower one,
    both with uniform grid noise of +- spread / 4 pA.  Sums on that grid are exact in float32 for these lengths: ties occur"""
    rng = np.random.default_rng(seed)
    if split is None:
        split = int(rng.integers(n // 8, n // 2 + 1)) if n >= 8 else n // 2
    x = np.empty(n, dtype=np.float64)
    x[:split] = hi
    x[split:] = lo
    if spread:
        x += rng.integers(-spread, spread + 1, n) / 4.0
    return x


def noisy_read(seed, n, split, hi=118.0, lo=76.0, sd=6.0):
    """a read off the grid: Gaussian noise, so that float32 and float64 sums round differently"""
    rng = np.random.default_rng(seed)
    x = rng.normal(lo, sd, n)
    x[:split] = rng.normal(hi, sd, split)
    return x


def as_dtype(x, dt):
    if dt == "f32":
        return x.astype(np.float32)
    if dt == "f64":
        return x.copy()
    return np.round(np.nan_to_num(x, nan=0.0, posinf=3000.0, neginf=-3000.0)).astype(np.int32 if dt == "i32" else np.int16)


def _as(name, signal, **params):
    return dict(name=name, signal=signal, params=params)


def _sweep():
    out = []
    for w, mo in AS_PARAMS:
        for k, ls in enumerate(as_diff_sizes(w)):
            n = ls + w + mo
            out.append(_as("sweep.w%d.mo%d.L%d" % (w, mo, ls), ("step", 1000 * w + 10 * k + mo % 7, n, dict(spread=8)),
                           window=w, min_obs_adapter=mo, min_shift=5.0))
    return out


def _with(kind_args, edits):
    return ("edit", kind_args, edits)


AS_CASES = _sweep() + [
    _as("constant", ("step", 1, 6000, dict(split=0, spread=0))),
    _as("two_levels", ("step", 2, 6000, dict(split=1500, spread=0))),
    _as("two_levels_noise", ("step", 3, 6000, dict(split=1500))),
    _as("low_current", ("step", 4, 6000, dict(split=1500, hi=85.0, lo=40.0, spread=4))),
    _as("nan_used", _with(("step", 5, 6000, dict(split=1500)), [(700, np.nan)])),
    _as("nan_used_late", _with(("step", 5, 6000, dict(split=1500)), [(3400, np.nan)])),
    _as("nan_trimmed", _with(("step", 3, 6000, dict(split=1500)), [(5000, np.nan), (5999, np.nan)])),
    _as("nan_window_edge", _with(("step", 3, 6000, dict(split=1500)), [(3499, np.nan)])),
    _as("pos_inf", _with(("step", 6, 6000, dict(split=1500)), [(900, np.inf)])),
    _as("neg_inf", _with(("step", 6, 6000, dict(split=1500)), [(2100, -np.inf)])),
    _as("both_inf", _with(("step", 6, 6000, dict(split=1500)), [(900, np.inf), (1000, -np.inf)])),
    _as("short", ("step", 7, 2000, {})),
    _as("just_short", ("step", 7, 2599, {})),
    _as("empty", ("step", 7, 0, {})),
    _as("empty_w1", ("step", 7, 0, {}), window=1, min_obs_adapter=0),
    _as("noisy", ("noisy", 8, 9000, 2100)),
    _as("noisy_small_shift", ("noisy", 9, 9000, 2100, dict(hi=90.0, lo=76.0))),
    _as("window_one", ("noisy", 10, 4000, 900), window=1, min_obs_adapter=100),
    _as("long_window", ("noisy", 11, 9000, 2500), window=700, min_obs_adapter=1000),
    _as("long_200k", ("noisy", 12, 200000, 40000)),
]


def as_by_name(name):
    for c in AS_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def _signal(spec):
    if spec[0] == "edit":
        x = _signal(spec[1])
        for i, v in spec[2]:
            x[i] = v
        return x
    if spec[0] == "step":
        return step_read(spec[1], spec[2], **spec[3])
    return noisy_read(spec[1], spec[2], spec[3], **(spec[4] if len(spec) > 4 else {}))


def as_input(case):
    """the case's signal (float64)"""
    return _signal(case["signal"])


def as_params(cls, case):
    p = cls()
    for k, v in case["params"].items():
        setattr(p, k, v)
    return p


def _tname(v):
    if isinstance(v, np.generic):
        return "np." + v.dtype.name
    return type(v).__name__


def as_call(fn, x, params):
    """one call of `moving_mean_adapter_start_detect` (the reference's, the drop-in's or the restatement's) -> the returned value
    with its Python type, or the exception's class and text"""
    try:
        r = fn(x, params)
    except ValueError as e:
        return "raise ValueError: %s" % e
    return "%s:%d" % (_tname(r), int(r))


# ---------------------------------------------------------------- start peak
SP_DTYPES = ("f32", "f64")
SP_COLUMNS = ["start_peak_idx", "start_peak_pa", "next_greater_idx", "next_greater_pa", "open_pore_idx", "flagged_type", "scale"]
RNA004_SECTION = dict(downscale_factor=10, start_peak_max_idx=150, offset1=10, offset2=100, open_pore_pa=195.0)


def _sp(name, seed, m, n=14, section=None, lens=None, **kw):
    return dict(name=name, seed=seed, m=m, n=n, section=section, lens=lens, kw=kw)


SP_CASES = [
    _sp("rna004_17500", 1, 17500, section=RNA004_SECTION),
    _sp("defaults_17500", 2, 17500),
    _sp("rna004_4000", 3, 4000, section=RNA004_SECTION),
    _sp("rna004_2000", 4, 2000, section=RNA004_SECTION),  # the successor's index falls off the pooled row: every row None
    _sp("ragged_ds10", 5, 4003, section=RNA004_SECTION),
    _sp("ragged_ds3", 6, 2000, section=dict(downscale_factor=3, start_peak_max_idx=120, offset1=7, offset2=60, open_pore_pa=195.0)),
    _sp("ragged_ds200", 7, 17500, section=dict(downscale_factor=200, start_peak_max_idx=20, offset1=2, offset2=10, open_pore_pa=195.0),
        lens=[17500, 17501, 40000, 17499, 9000, 12000, 16000, 17000, 300, 200]),
    _sp("empty_first_slice", 8, 4000, section=dict(downscale_factor=10, start_peak_max_idx=10, offset1=10, offset2=100, open_pore_pa=195.0)),
    _sp("all_lens_short", 9, 4000, section=RNA004_SECTION, lens=[100, 2499, 2500, 2510, 10, 3999, 4000, 100]),
    # fewer samples than one block: the open-pore scan's argmax of an empty slice is outside the reference's try block
    _sp("scan_raises", 11, 4000, section=RNA004_SECTION, lens=[4000, 9, 3000]),
    _sp("zero_len_raises", 12, 4000, section=RNA004_SECTION, lens=[0]),
    _sp("one_read", 10, 17500, n=1, section=RNA004_SECTION),
]


def sp_by_name(name):
    for c in SP_CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def sp_section(cls, case):
    """the case's [rna_start_peak] section: the class defaults, or those with the case's fields"""
    s = cls()
    for k, v in (case["section"] or {}).items():
        setattr(s, k, v)
    return s


def sp_input(case, section):
    """(signals float64 [n, m] NaN-padded behind min(len, m), full lengths int64 [n]).  The rows cycle through: a peak with no
    greater successor; a greater successor; an open pore between the two; an open pore at the successor; a NaN inside the
    first slice; an open pore in front of the peak; plain noise"""
    rng = np.random.default_rng(case["seed"])
    n, m = case["n"], case["m"]
    ds, spmax, off1, off2 = section.downscale_factor, section.start_peak_max_idx, section.offset1, section.offset2
    lens = case["lens"]
    if lens is None:
        lens = [m, m + 1, 3 * m, m - 1, 100] + [int(v) for v in rng.integers((m * 2) // 3, m + 2000, max(n - 5, 0))]
    lens = np.array(lens[:n], dtype=np.int64)
    n = lens.size
    X = np.round(rng.normal(80.0, 4.0, (n, m)) * 8.0) / 8.0
    for r in range(n):
        kind = r % 7
        a, b = off1 * ds, max(spmax * ds, off1 * ds + ds)
        pk = int(rng.integers(a, max((a + (b - a) // 4) if kind == 2 else (b - 2 * ds), a + 1)))
        if pk + 2 * ds <= m:
            X[r, pk:pk + 2 * ds] += 60.0
        s0 = (spmax + off2) * ds
        nx = s0 + int(rng.integers(3, 40)) * ds
        if kind in (1, 2, 3) and nx + ds <= m:
            X[r, nx:nx + ds] += 75.0
        if kind == 2:
            scan = min(int(lens[r]), m) // ds  # (the reference scans this many RAW samples for the open pore)
            op = int(rng.integers(pk + 3 * ds, max(min(s0, scan), pk + 3 * ds + 1)))
            if op < m:
                X[r, op] = 230.0
        if kind == 3 and nx + ds <= m:
            X[r, nx + 1] = 260.0
        if kind == 4 and a + 3 < m:
            X[r, int(rng.integers(a, min(b, m)))] = np.nan
        if kind == 5 and a > 4:
            X[r, int(rng.integers(ds, a)) if a > ds else 1] = 240.0
        X[r, min(int(lens[r]), m):] = np.nan
    return X, lens


def sp_as_dtype(X, dt):
    return X.astype(np.float32) if dt == "f32" else X.copy()


def sp_call(fn, X, lens, spc):
    """one call of `detect_rna_start_peak` -> its encoded frame, or {"raise": the exception's class and text}"""
    try:
        df = fn(X, lens, spc)
    except ValueError as e:
        return {"raise": np.array("raise ValueError: %s" % e)}
    return enc_frame(df)


def enc_frame(df):
    """a start-peak frame as arrays: per column the values as float64 (NaN where the cell is None or NaN) and a mask of the
    cells that are None; the flag strings ("" for None); the dtypes as pandas prints them"""
    out = {}
    for col in SP_COLUMNS:
        if col not in df.columns:
            out[col + ".missing"] = np.array(True)
            continue
        cells = list(df[col])
        out[col + ".none"] = np.array([c is None for c in cells], dtype=bool)
        if col == "flagged_type":
            out[col] = np.array(["" if c is None or c != c else str(c) for c in cells], dtype="U64")
            out[col + ".nan"] = np.array([c is not None and c != c for c in cells], dtype=bool)
        else:
            out[col] = np.array([np.nan if c is None else float(c) for c in cells], dtype=np.float64)
    out["dtypes"] = np.array(str(df.dtypes))
    out["columns"] = np.array([str(c) for c in df.columns])
    return out


def frame_diff(got, want, dtypes=True):
    """the keys in which two encoded frames differ (float cells by bits, every NaN as one)"""
    bad = []
    for k in sorted(set(got) | set(want)):
        if k == "dtypes" and not dtypes:
            continue
        if k not in got or k not in want:
            bad.append(k)
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape:
            bad.append(k)
        elif a.dtype.kind == "f":
            if not np.array_equal(a, b, equal_nan=True) or not np.array_equal(np.signbit(a), np.signbit(b)):
                bad.append(k)
        elif a.tolist() != b.tolist():
            bad.append(k)
    return bad


def same_pandas(gold):
    """is the installed pandas the fixture's, by major.minor?  (column dtypes are compared only then)"""
    import pandas

    return pandas.__version__.split(".")[:2] == str(gold["pandas"]).split(".")[:2]


def sp_want(gold, name, dt):
    pre = "sp.%s.%s." % (name, dt)
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}


def signature_rows(mod, names):
    """name(parameter:kind:default, ...) of the module's functions"""
    rows = []
    for nm in names:
        ps = []
        for p in inspect.signature(getattr(mod, nm)).parameters.values():
            ps.append("%s:%s:%s" % (p.name, p.kind.name, "-" if p.default is inspect.Parameter.empty else repr(p.default)))
        rows.append(nm + "(" + ", ".join(ps) + ")")
    return rows
