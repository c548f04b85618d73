"""Cases of the reference's LLR trace module (adapted/detect/llr.py), shared by ``tools/gen_llr_module_golden.py`` (runs the REAL
reference's llr.py, scipy 1.7, in the build container) and the parity tests.  Every input comes from a seed; the fixture
tests/golden/llr_module.npz holds outputs only.  Python >= 3.8 syntax only."""
import numpy as np

from trace_cases import squiggle


def bump(x, c, w):
    """a bump of height 1 at c, half width w: 1 / (1 + ((x - c) / w)^2) -- arithmetic only (a transcendental function of numpy
    may differ in the last bit between versions and machines, and the inputs must be the same everywhere)"""
    u = (x - c) / w
    return 1.0 / (1.0 + u * u)

# the names adapted/detect/llr.py defines (the fixture records them from the reference module itself)
NAMES = ["LLRBoundariesLog", "LLRTrace", "correct_for_plateau", "correct_for_split_peak", "find_peaks_in_trace", "adapter_end_from_trace",
         "calc_adapter_trace", "calc_polya_trace", "calc_full_polya_trace", "detect_full_polya_trace_peak_with_spike"]


def bumps(seed, n, k, width=(15, 120), noise=0.05, floor=0.0):
    """an LLR-trace-like array: k Gaussian bumps of random height on a small noise floor, zeros at both ends"""
    rng = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64)
    y = np.full(n, floor)
    for _ in range(k):
        c, w, h = rng.uniform(0.1 * n, 0.9 * n), rng.uniform(*width), rng.uniform(2.0, 30.0)
        y += h * bump(x, c, w)
    y += rng.normal(0.0, noise, n)
    z = max(1, n // 40)
    y[:z] = 0.0
    y[-z:] = 0.0
    return y


def plateau_after_peak(seed, n=1600):
    """a peak, a shallow dip, then a monotone rise (a plateau) above 0.9 of the peak, then a fall"""
    rng = np.random.default_rng(seed)
    y = np.zeros(n)
    a = n // 4
    y[5:a] = np.linspace(0.1, 20.0, a - 5)
    y[a:a + 30] = 20.0 - np.linspace(0.0, 1.5, 30)
    y[a + 30:a + 80] = np.linspace(18.6, 19.5, 50)
    y[a + 80:n - 5] = np.linspace(19.0, 0.5, n - 85 - a)
    return y + rng.normal(0.0, 0.002, n) * (y > 0)


def split_peak(seed, n=1200, gap=60, second=0.95):
    """two close maxima of almost equal height (the reference's split peak)"""
    x = np.arange(n, dtype=np.float64)
    c = n // 3
    y = 20.0 * bump(x, c, 40.0) + 20.0 * second * bump(x, c + gap, 25.0)
    y += np.random.default_rng(seed).normal(0.0, 0.01, n)
    y[:3] = 0.0
    y[-3:] = 0.0
    return y


def strided(seed, n, stride, k=4):
    """a trace as c_llr_trace leaves it with stride > 1: values every `stride` points, zeros between"""
    y = bumps(seed, n, k)
    m = np.zeros(n)
    m[::stride] = 1.0
    return y * m


def _holes(y, seed, frac=0.01, what=np.nan):
    y = y.copy()
    rng = np.random.default_rng(seed)
    idx = rng.choice(np.arange(5, y.size - 5), max(1, int(frac * y.size)), replace=False)
    y[idx] = what
    return y


def trace_of(case):
    k = case["kind"]
    if k == "bumps":
        y = bumps(case["seed"], case["n"], case.get("k", 5), noise=case.get("noise", 0.05))
    elif k == "plateau":
        y = plateau_after_peak(case["seed"], case["n"])
    elif k == "split":
        y = split_peak(case["seed"], case["n"], case.get("gap", 60), case.get("second", 0.95))
    elif k == "strided":
        y = strided(case["seed"], case["n"], case["stride"], case.get("k", 4))
    elif k == "negative":
        y = -np.abs(bumps(case["seed"], case["n"], 3)) - 0.5
    elif k == "zeros":
        y = np.zeros(case["n"])
    elif k == "tiny":
        y = np.asarray(case["values"], dtype=np.float64)
    elif k == "spike":
        y = spike_trace(case["seed"], case["n"], case["h1"], case.get("rise", "linear"), case.get("spacing", 300))
    elif k == "ties":
        y = ties_trace(case["n"])
    else:
        raise KeyError(k)
    if case.get("nan"):
        y = _holes(y, case["seed"] + 1, case["nan"])
    if case.get("inf"):
        y = _holes(y, case["seed"] + 2, case["inf"], np.inf)
    if case.get("ninf"):
        y = _holes(y, case["seed"] + 3, case["ninf"], -np.inf)
    return y


def spike_trace(seed, n, h1, rise, spacing):
    """the full poly(A) trace with a spike: a first peak (height 10), a dip, then a rise to a second peak of height h1"""
    rng = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64)
    p0 = n // 4
    p1 = p0 + spacing
    y = 10.0 * bump(x, p0, 12.0)
    lo = p0 + 40
    if rise == "linear":
        seg = np.linspace(0.5, h1, p1 - lo)
    else:
        u = np.linspace(0.0, 1.0, p1 - lo)
        seg = 0.5 + (h1 - 0.5) * (u * u * u)
    y[lo:p1] = np.maximum(y[lo:p1], seg + rng.normal(0.0, 0.05, p1 - lo))
    y[p1:p1 + 60] = np.maximum(y[p1:p1 + 60], np.linspace(h1, 0.0, 60))
    y += rng.normal(0.0, 0.01, n)
    y[:2] = 0.0
    return y


def ties_trace(n):
    """maxima of exactly equal height closer than the distance, where the answer does not depend on which one scipy keeps:
    both lie inside one bump whose prominence and width decide alone"""
    y = np.zeros(n)
    x = np.arange(n, dtype=np.float64)
    y += 8.0 * bump(x, n / 3, 30.0)
    y = np.round(y, 3)
    return y


def _sig(name, seed, n, stride=1, oh=5, ot=5, es=(0, 1), win=(500, 100, 50, 10), trace_params=(100, 1.0, 0.5), end_params=(1.0, 1.0, 2000),
         store=False):
    return dict(name=name, raw=dict(seed=seed, n=n), stride=stride, oh=oh, ot=ot, aes=es[0], pes=es[1], win=win, fp=trace_params,
                ae=end_params, store=store)


# calc_adapter_trace on squiggles (trace_cases.squiggle): strides, early stopping on and off, parameters
SIGNAL_CASES = [
    _sig("sq_s1_es", 1, 1600),
    _sig("sq_s1_noes", 2, 1600, es=(0, 0)),
    _sig("sq_s1_aes", 3, 1600, es=(1, 0)),
    _sig("sq_s3", 4, 1600, stride=3, win=(501, 99, 51, 9), store=True),
    _sig("sq_s10", 5, 2400, stride=10, win=(500, 100, 50, 10), store=True),
    _sig("sq_s10_noes", 6, 2400, stride=10, es=(0, 0), store=True),
    _sig("sq_long", 7, 20150, oh=5, ot=5),
    _sig("sq_params", 8, 3000, trace_params=(20, 0.5, 0.8), end_params=(0.5, 0.7, 50)),
    _sig("sq_wide", 9, 3000, end_params=(2.0, 1.0, 10)),
    _sig("sq_offsets", 10, 1600, oh=40, ot=30),
]
for _k in range(6):
    SIGNAL_CASES.append(_sig("sq_mix%d" % _k, 100 + _k, 800 + 700 * _k, stride=(1, 3, 10)[_k % 3], es=((0, 1), (0, 0), (1, 0))[_k % 3],
                             end_params=(0.5 + 0.25 * _k, 1.0, 20 + 40 * _k)))


def _tr(name, stride=1, min_obs=5, tail_trim=5, fp=(100, 1.0, 0.5), ae=(1.0, 1.0, 2000), store=False, **kind):
    if kind["kind"] == "strided":
        kind["stride"] = stride
    return dict(name=name, trace=kind, stride=stride, min_obs=min_obs, tail_trim=tail_trim, fp=fp, ae=ae, store=store)


# LLRTrace built on given arrays: multi-peak, plateaus, split peaks, NaN holes, +-inf, all <= 0, lengths 1-4, strided traces
TRACE_CASES = [
    _tr("multi", kind="bumps", seed=1, n=3000, k=8, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("multi_many", kind="bumps", seed=2, n=6000, k=30, noise=0.3, fp=(5, 0.1, 0.5), ae=(0.1, 0.5, 5)),
    _tr("multi_default", kind="bumps", seed=3, n=4000, k=6),
    _tr("plateau", kind="plateau", seed=4, n=1600, fp=(20, 0.3, 0.5), ae=(0.3, 1.0, 20)),
    _tr("split", kind="split", seed=5, n=1200, fp=(10, 0.3, 0.5), ae=(0.3, 0.5, 10)),
    _tr("split_low", kind="split", seed=6, n=1200, gap=80, second=0.7, fp=(10, 0.3, 0.5), ae=(0.3, 0.5, 10)),
    _tr("nan_holes", kind="bumps", seed=7, n=3000, k=6, nan=0.01, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("inf", kind="bumps", seed=8, n=2000, k=4, inf=0.002, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("ninf", kind="bumps", seed=9, n=2000, k=4, ninf=0.002, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("all_negative", kind="negative", seed=10, n=500),
    _tr("all_zero", kind="zeros", seed=11, n=300),
    _tr("len1", kind="tiny", seed=0, values=[1.0]),
    _tr("len2", kind="tiny", seed=0, values=[0.0, 2.0]),
    _tr("len3", kind="tiny", seed=0, values=[0.5, 2.0, 0.5], fp=(0, 0.0, 0.5), ae=(0.0, 0.5, 0)),
    _tr("len4", kind="tiny", seed=0, values=[0.0, 1.0, 3.0, 1.0], fp=(0, 0.0, 0.5), ae=(0.0, 0.5, 0), min_obs=0, tail_trim=0),
    _tr("strided3", kind="strided", seed=12, n=2000, stride=3, store=True, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("strided10", kind="strided", seed=13, n=4000, stride=10, store=True, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("strided10_nan", kind="strided", seed=14, n=3000, stride=10, nan=0.005, store=True, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("strided10_inf", kind="strided", seed=15, n=3000, stride=10, inf=0.002, store=True, fp=(20, 0.5, 0.5), ae=(0.5, 0.5, 20)),
    _tr("early_stop_range_empty", kind="bumps", seed=16, n=60, k=2, min_obs=80, tail_trim=5),
    _tr("no_peaks", kind="bumps", seed=17, n=2000, k=1, fp=(1000, 5.0, 0.5), ae=(5.0, 1.0, 5000)),
]

# correct_for_plateau / correct_for_split_peak on their own, with non-default parameters: (trace case, peak, s, t, window, prominence)
CORRECTION_CASES = [
    ("plateau", 400, 10, 0.9, 500, 1.0),
    ("plateau", 400, 1, 0.9, 500, 1.0),
    ("plateau", 400, 3, 0.95, 120, 0.5),
    ("plateau", 400, 40, 0.8, 1000, 2.0),
    ("plateau", 1590, 10, 0.9, 500, 1.0),
    ("split", 400, 10, 0.9, 500, 1.0),
    ("split", 400, 5, 0.5, 200, 0.1),
    ("split_low", 400, 10, 0.9, 500, 1.0),
    ("split_low", 400, 10, 0.6, 500, 1.0),
    ("multi", 1000, 2, 0.5, 3000, 0.2),
    ("nan_holes", 800, 10, 0.9, 500, 1.0),
]


def _sp(name, d=10, prom=1.0, width=10, ratio=0.5, r2=0.99, **kind):
    return dict(name=name, trace=kind, d=d, prom=prom, width=width, ratio=ratio, r2=r2)


# detect_full_polya_trace_peak_with_spike: distances 1 / 2 / 10 / 25 / 101, both sides of the r**2 and ratio tests, NaN / inf, ties
SPIKE_CASES = [
    _sp("second_higher", kind="spike", seed=1, n=2000, h1=12.0),
    _sp("second_low", kind="spike", seed=2, n=2000, h1=3.0),
    _sp("linear_rise", kind="spike", seed=3, n=2000, h1=8.0, r2="above"),
    _sp("linear_rise_below", kind="spike", seed=3, n=2000, h1=8.0, r2="below"),
    _sp("curved_rise", kind="spike", seed=4, n=2000, h1=8.0, rise="cubic"),
    _sp("curved_rise_above", kind="spike", seed=4, n=2000, h1=8.0, rise="cubic", r2="above"),
    _sp("curved_rise_below", kind="spike", seed=4, n=2000, h1=8.0, rise="cubic", r2="below"),
    _sp("d1", kind="bumps", seed=5, n=3000, k=8, noise=0.2, d=1),
    _sp("d2", kind="bumps", seed=5, n=3000, k=8, noise=0.2, d=2),
    _sp("d10", kind="bumps", seed=5, n=3000, k=8, noise=0.2, d=10),
    _sp("d25", kind="bumps", seed=5, n=3000, k=8, noise=0.2, d=25),
    _sp("d101", kind="bumps", seed=5, n=3000, k=8, noise=0.2, d=101),
    _sp("d2_5", kind="bumps", seed=6, n=3000, k=8, noise=0.2, d=2.5),
    _sp("params", kind="bumps", seed=7, n=3000, k=10, noise=0.1, d=25, prom=0.5, width=5, ratio=0.3),
    _sp("nan", kind="spike", seed=8, n=2000, h1=8.0, nan=0.01),
    _sp("inf", kind="bumps", seed=9, n=2000, k=5, inf=0.002, ninf=0.002),
    _sp("ties", kind="ties", n=600, d=10),
    _sp("none", kind="zeros", n=100),
    _sp("short", kind="tiny", values=[0.0, 5.0, 0.0]),
]


def r2_of(y, p0, p1):
    """linregress's r**2 on [argmin(y[p0:p1]) + p0, p1), in numpy: the generator places the thresholds of the spike cases marked
    "above" / "below" 1e-9 on either side of it and records them in the fixture"""
    i = int(np.argmin(y[p0:p1])) + p0
    x = np.arange(i, p1, dtype=np.float64)
    s = y[i:p1]
    c = np.cov(x, s, bias=True)
    return float(c[0, 1] ** 2 / (c[0, 0] * c[1, 1]))


def by_name(cases, name):
    for c in cases:
        if c["name"] == name:
            return c
    raise KeyError(name)


def raw_of(case):
    return squiggle(case["raw"]["seed"], case["raw"]["n"])
