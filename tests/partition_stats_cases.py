"""Cases that drive every branch of k_partition_stats (adapted_amd/csrc/block_stats.h), shared by the CPU and the GPU test.

The kernel guesses (a 3072-bucket key window round a median-of-three pivot, a MAD bracket predicted from the pass-A
histogram, fixed-size LDS lists for the median's bucket and the bracket) and verifies; whenever a guess misses or a list
overflows a slower branch takes over.  A case is ONE read -- adapter ~ N(75, 6), poly(A) ~ N(110, 2), RNA ~ N(100, 8), NaN
padding behind it -- with the distribution under test in one of the three partitions; the boundaries are handed to
Engine.validate_rows / oracle.detect_cnn_from_preds as they are.  Every case comes from a seed.

`trace` restates the kernel's branch arithmetic in numpy from the constants block_stats.h documents; `tags` names the branches
a segment takes.  Each case lists the tags it was built for: the CPU test holds the data to them, the GPU test holds the
device's tallies (g_bs_tally 0-4, g_dbg[20], g_dbg[21]) to the sums they imply.  numpy only."""
import numpy as np

M = 40000          # samples per row (core.max_obs_trace of `make_spc`)
BS_BINS = 3072     # pass A: 20-bit key buckets in the window; also the longest segment that is selected directly in LDS
BS_KSH = 12
BS_MEDCAP = 512    # samples of the median's bucket kept
BS_MADCAP = 2560   # samples of the MAD bracket kept
BS_BINS18 = 1536   # passes C/D: 18-bit buckets in the window, samples collected
BS_SMALLCAP = 4352 + 3072  # the longest adapter whose sums run in LDS
TALLY_MIN = 8192   # the kernel tallies segments of at least this many samples

F32 = np.float32


def make_spc():
    """RNA004, CNN primary, m = 40 000, the validator's own checks off: every case is an ordinary row"""
    from adapted_amd.config import get_chemistry_specific_config

    spc = get_chemistry_specific_config("RNA004")
    spc.core.max_obs_trace = M
    spc.mvs_polya.mvs_detect_check = False
    spc.real_range.real_signal_check = False
    spc.real_range.detect_open_pores = False
    spc.cnn_boundaries.fallback_to_llr_short_reads = False
    spc.update_primary_method()
    spc.update_sig_preload_size()
    assert spc.primary_method == "cnn" and spc.sig_preload_size == M
    return spc


# ---------------------------------------------------------------------------------------------------- the distributions
def gen(kind, n, rng):
    """n float32 samples of distribution `kind`"""
    def normal(mu, sd, k=n):
        return rng.normal(mu, sd, k)

    if kind in ("typical", "pivot_outliers", "plus_inf", "both_inf", "nan"):
        x = normal(100.0, 8.0)
        if kind == "pivot_outliers":  # the three samples the pivot is the median of
            x[[n // 4, n // 2, (3 * n) // 4]] = 1000.0
        elif kind == "plus_inf":
            x[17 % n] = np.inf
        elif kind == "both_inf":
            x[17 % n], x[n - 5] = np.inf, -np.inf
        elif kind == "nan":
            x[n // 3] = np.nan
    elif kind == "adapter":
        x = normal(75.0, 6.0)
    elif kind == "polya":
        x = normal(110.0, 2.0)
    elif kind == "zero_centred":
        x = normal(0.0, 1.0)
    elif kind in ("three_clusters", "three_clusters_huge_sd"):
        k0, k2 = (3 * n) // 10, (3 * n) // 10
        top = 1e6 if kind.endswith("huge_sd") else 400.0
        x = np.concatenate([normal(20.0, 1.0, k0), normal(100.0, 1.0, n - k0 - k2), normal(top, 1.0, k2)])
        perm = rng.permutation(n)
        x, middle = x[perm], (perm >= k0) & (perm < n - k2)
        # the pivot's three samples come from the middle cluster, so that the window holds the median and 40 % of the samples
        piv = np.array([n // 4, n // 2, (3 * n) // 4])
        middle[piv] = False
        src = np.nonzero(middle)[0][:3]
        x[piv], x[src] = x[src].copy(), x[piv].copy()
    elif kind == "wide_uniform":
        x = rng.uniform(10.0, 2000.0, n)
        x[[n // 4, n // 2, (3 * n) // 4]] = 1005.0  # the pivot in the middle: the window holds the median, not the MAD's lower samples
    elif kind == "two_values":
        x = np.concatenate([np.full(n // 2, 90.0), np.full(n - n // 2, 110.0)])
        rng.shuffle(x)
    elif kind == "two_clusters":
        x = np.concatenate([normal(90.0, 0.01, n // 2), normal(110.0, 0.01, n - n // 2)])
        rng.shuffle(x)
    elif kind.startswith("grid_"):  # grid_<step> of N(100, 8), grid_<step>_narrow of N(100, .4)
        q = float(kind.split("_")[1])
        x = np.round(normal(100.0, 0.4 if kind.endswith("_narrow") else 8.0) / q) * q
    elif kind == "constant":
        x = np.full(n, 77.25)
    elif kind == "mostly_constant":
        x = np.full(n, 77.25)
        x[::7] = 80.0
    elif kind == "negative":
        x = -normal(100.0, 8.0)
    elif kind == "tiny":
        x = normal(1e-30, 1e-31)
    else:
        raise ValueError(kind)
    return np.asarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------- the kernel's branch arithmetic, restated
def f2key(x):
    """the order-preserving uint32 key of a float32 (common.h f2key)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _find_bin(h, k, under):
    """block_find_bin: the cell of rank k among the counts h with `under` samples before them -> (cell, samples before it) or None"""
    cum = under + np.cumsum(h)
    if k < under or k >= cum[-1]:
        return None
    b = int(np.searchsorted(cum, k, side="right"))
    return b, int(cum[b] - h[b])


def _window_lo(pivot, sh):
    """bs_window_lo<sh>: half an octave below the pivot's octave, in buckets of 2^sh keys"""
    per_oct = 1 << (23 - sh)
    octv = (int(f2key(F32(pivot))) >> sh) & ~(per_oct - 1)
    return octv - per_oct // 2 if octv >= per_oct // 2 else 0


def trace(x):
    """what block_segment_stats does with the segment x when k_validate did not hand it the median (poly(A), RNA) -> dict of facts"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, k1 = x.size, x.size // 2
    f = {"n": n, "nan": bool(np.isnan(x).any()), "lds": n <= BS_BINS}
    with np.errstate(all="ignore"):
        f["nan_mean"] = bool(np.isnan(np.mean(x)))
        if f["lds"] or f["nan"]:
            return f
        med, sd = np.median(x), np.std(x)
        # pass A: the window of 3072 buckets (key >> 12) centred on the median of three samples
        a, b, c3 = x[n // 4], x[n // 2], x[(3 * n) // 4]
        pivot = max(min(a, b), min(max(a, b), c3))
        kb = int(f2key(pivot)) >> BS_KSH
        wlo = kb - BS_BINS // 2 if kb >= BS_BINS // 2 else 0
        key = f2key(x)
        d = (key >> BS_KSH).astype(np.int64) - wlo
        inwin = (d >= 0) & (d < BS_BINS)
        hist = np.bincount(d[inwin], minlength=BS_BINS)
        hit = _find_bin(hist, k1, int((d < 0).sum()))
        f["fallback_med"] = hit is None
        f["predicted"] = f["done"] = False
        f["ncollect"] = f["nmad"] = 0
        if hit is not None:
            f["bin"], f["rk"] = hit[0], k1 - hit[1]
            key_lo = np.uint32((wlo + hit[0]) << BS_KSH)
            c_lo, c_hi = key2f(key_lo), key2f(key_lo + np.uint32(1 << BS_KSH))
            c, w0 = F32(0.5) * (c_lo + c_hi), c_hi - c_lo
            if not w0 > 0 or np.isinf(c_lo) or np.isinf(c_hi):
                f["fallback_med"] = True
        if not f["fallback_med"]:
            inb = d == f["bin"]
            f["ncollect"] = int(inb.sum())
            f["one_value"] = bool(key[inb].min() == key[inb].max())
            # bs_predict_mad: the bins by the distance of their centres to the bucket's, in bucket widths
            occ = np.nonzero(hist)[0]
            xc = key2f(((wlo + occ).astype(np.uint32) << np.uint32(BS_KSH)) + np.uint32(1 << (BS_KSH - 1)))
            dd = np.abs(xc - c) / w0
            ok = dd < F32(BS_BINS)
            dh = np.bincount(dd[ok].astype(np.int64), weights=hist[occ][ok], minlength=BS_BINS).astype(np.int64)
            hit = _find_bin(dh, k1, 0)
            f["predicted"] = hit is not None
        if f["predicted"]:
            j = hit[0]
            P, Q = max(F32(j - 3) * w0, F32(0)), F32(j + 4) * w0
            dt = np.abs(x - c)
            bracket = (dt >= P) & (dt <= Q)
            f["nmad"], rel, need_prev = int(bracket.sum()), k1 - int((dt < P).sum()), int(n % 2 == 0)
            if f["nmad"] <= BS_MADCAP and need_prev <= rel < f["nmad"]:
                dv = np.sort(np.abs(x[bracket] - med))
                lo, vk = dv[rel - need_prev], dv[rel]
                dm = np.abs(med - c) + F32(0.25) * w0
                f["done"] = bool(lo >= P + dm and vk <= Q - dm and dm < F32(2) * w0)
        if not f["done"]:
            # passes C/D: 1536 buckets of key(|x - med|) >> 14 from a quarter of the octave of 0.6745 std
            pv = F32(0.6745) * sd
            if not pv > 0:
                pv = F32(1.0)
            w18 = _window_lo(pv, 14)
            w18 = w18 - 512 if w18 >= 512 else 0
            dkey = f2key(np.abs(x - med))
            d18 = (dkey >> 14).astype(np.int64) - w18
            in18 = (d18 >= 0) & (d18 < BS_BINS18)
            hit = _find_bin(np.bincount(d18[in18], minlength=BS_BINS18), k1, int((d18 < 0).sum()))
            f["cd_miss"] = hit is None
            if hit is not None:
                sel = d18 == hit[0]
                f["cd_ncollect"], f["cd_rk"] = int(sel.sum()), k1 - hit[1]
                f["cd_one_value"] = bool(dkey[sel].min() == dkey[sel].max())
    return f


# one predicate per branch, over the facts of `trace` (the first five are what g_bs_tally 1-4 and their remainder count,
# one_value_bucket and dense_bucket what g_dbg[20] and g_dbg[21] count; the others have no tally)
PREDICATES = {
    "proven": lambda f: f["done"],
    "fallback_med": lambda f: f["fallback_med"],
    "not_predicted": lambda f: not f["predicted"],
    "bracket_overflow": lambda f: f["predicted"] and not f["done"] and f["nmad"] > BS_MADCAP,
    "unproven": lambda f: f["predicted"] and not f["done"] and f["nmad"] <= BS_MADCAP,
    "one_value_bucket": lambda f: f["ncollect"] > BS_MEDCAP and f["one_value"],
    "dense_bucket": lambda f: f["ncollect"] > BS_MEDCAP and not f["one_value"],
    "rk0_even": lambda f: not f["fallback_med"] and f["n"] % 2 == 0 and f["rk"] == 0,
    "cd_hit": lambda f: not f["done"] and not f["cd_miss"] and f["cd_ncollect"] <= BS_BINS18,
    "cd_miss": lambda f: not f["done"] and f["cd_miss"],
    "cd_one_value": lambda f: not f["done"] and not f["cd_miss"] and f["cd_ncollect"] > BS_BINS18 and f["cd_one_value"],
    "cd_overflow": lambda f: not f["done"] and not f["cd_miss"] and f["cd_ncollect"] > BS_BINS18 and not f["cd_one_value"],
}


def tags(x):
    """the branches segment x takes -> frozenset of names (PREDICATES, or "lds" / "nan" / "nan_mean" where they do not apply)"""
    f = trace(x)
    if f["nan"]:
        return frozenset(["nan"])
    if f["lds"]:
        return frozenset(["lds"])
    return frozenset([k for k, p in PREDICATES.items() if p(f)] + (["nan_mean"] if f["nan_mean"] else []))


# ---------------------------------------------------------------------------------------------------------------- the cases
CONTROL = frozenset(["proven"])
_FB = frozenset(["fallback_med", "not_predicted"])
# the tags each distribution was built for at n = 20 000 (n = 20 001 for typical_odd) behind the large-segment path
DIST_TAGS = {
    "typical": CONTROL,
    "pivot_outliers": _FB | {"cd_hit"},
    "zero_centred": _FB | {"cd_hit"},
    "three_clusters": frozenset(["not_predicted", "cd_hit"]),
    "three_clusters_huge_sd": frozenset(["not_predicted", "cd_miss"]),
    "wide_uniform": frozenset(["unproven", "cd_hit"]),
    "two_values": frozenset(["bracket_overflow", "one_value_bucket", "rk0_even", "cd_one_value"]),
    "two_clusters": frozenset(["bracket_overflow", "rk0_even", "cd_overflow"]),
    "grid_4.0": frozenset(["bracket_overflow", "one_value_bucket", "cd_one_value"]),
    "grid_0.02_narrow": frozenset(["bracket_overflow", "dense_bucket", "cd_hit"]),
    "grid_0.005_narrow": frozenset(["bracket_overflow", "dense_bucket", "cd_hit"]),
    "constant": frozenset(["bracket_overflow", "one_value_bucket", "cd_miss"]),
    "mostly_constant": frozenset(["bracket_overflow", "one_value_bucket", "cd_miss"]),
    "plus_inf": CONTROL,
    "both_inf": CONTROL | {"nan_mean"},
    "nan": frozenset(["nan"]),
    "negative": CONTROL,
    "tiny": CONTROL,
}
REPEATED = ["pivot_outliers", "three_clusters", "two_values", "grid_4.0", "nan"]  # ... again in the poly(A) slice and the adapter
GROUPS = ["control", "fallback_med", "not_predicted", "unproven", "overflow", "nonfinite", "sizes", "polya", "adapter"]


def _case(name, group, seed, rna=("typical", 20000), polya=("polya", 1500), adapter=("adapter", 5000), expect=None):
    return {"name": name, "group": group, "seed": seed, "adapter": adapter, "polya": polya, "rna": rna,
            "expect": expect}  # expect: the tags of the partition under test (None: the control's)


def _cases():
    out = []
    group_of = {"typical": "control", "negative": "control", "tiny": "control", "pivot_outliers": "fallback_med",
                "zero_centred": "fallback_med", "three_clusters": "not_predicted", "three_clusters_huge_sd": "not_predicted",
                "wide_uniform": "unproven", "plus_inf": "nonfinite", "both_inf": "nonfinite", "nan": "nonfinite"}
    for kind, want in DIST_TAGS.items():
        nm = {"two_values": "two_values_even", "two_clusters": "two_clusters_even"}.get(kind, kind)
        out.append(_case(nm, group_of.get(kind, "overflow"), 0, rna=(kind, 20000), expect=want))
    out.append(_case("typical_odd", "control", 0, rna=("typical", 20001), expect=CONTROL))
    # sizes and edges: N(100, 8) everywhere
    for n in (3073, 8191, 8192, 8193, 16384, 16385, 3 * 8192 + 127, 3 * 8192 + 129):
        out.append(_case("rna_len_%d" % n, "sizes", 0, rna=("typical", n), expect=CONTROL))
    for n in (1, 2, 7, 8, 9, 127, 128, 129, 3071, 3072, 3073):
        out.append(_case("polya_len_%d" % n, "sizes", 0, polya=("polya", n), expect=CONTROL if n > BS_BINS else frozenset(["lds"])))
    for n in (BS_SMALLCAP - 1, BS_SMALLCAP, BS_SMALLCAP + 1, 8193):
        out.append(_case("adapter_len_%d" % n, "sizes", 0, adapter=("adapter", n)))
    for i in range(4):      # every residue of both segment starts mod 4: the 16-byte loads start from 4-byte aligned addresses
        for j in range(4):  # (a poly(A) slice of the large path: ragged-chunk loads from a_e, whole-chunk loads from p_e)
            out.append(_case("start_mod4_%d_%d" % (i, j), "sizes", 0, adapter=("adapter", 5000 + i), polya=("polya", 3200 + j - i),
                             expect=CONTROL))
    for kind in REPEATED:
        for n in (3073, 3000):  # the large path, and the one read into LDS
            # (below 8192 samples the bracket of N(100, 8)-like data need not prove itself: the tags are pinned per case)
            out.append(_case("polya_%s_%d" % (kind, n), "polya", 0, polya=(kind, n), expect=POLYA_TAGS[(kind, n)]))
        out.append(_case("adapter_%s" % kind, "adapter", 0, adapter=(kind, 9000)))  # median and MAD from k_validate, the sums from here
    for i, c in enumerate(out):
        c["seed"] = 7000 + i
    assert len(set(c["name"] for c in out)) == len(out)
    return out


POLYA_TAGS = {(k, 3000): frozenset(["nan" if k == "nan" else "lds"]) for k in REPEATED}
POLYA_TAGS.update({
    ("pivot_outliers", 3073): _FB | {"cd_miss"},  # (three outliers in 3073 samples: 0.6745 std is four times the MAD)
    ("three_clusters", 3073): frozenset(["not_predicted", "cd_hit"]),
    ("two_values", 3073): frozenset(["unproven", "one_value_bucket", "cd_miss"]),  # (an odd count: 1537 x 110.0, the MAD is 0)
    ("grid_4.0", 3073): frozenset(["proven", "one_value_bucket"]),
    ("nan", 3073): frozenset(["nan"]),
})
CASES = _cases()


def by_group(group):
    return [c for c in CASES if c["group"] == group]


def under_test(case):
    """the partition a case is about: "adapter", "polya" or "rna" """
    if case["adapter"][0] != "adapter" or case["name"].startswith("adapter_len"):
        return "adapter"
    return "polya" if case["polya"][0] != "polya" or case["name"].startswith("polya_len") else "rna"


def build(case):
    """-> (row float32[M] with NaN behind the read, read length, adapter end, poly(A) end)"""
    rng = np.random.default_rng(case["seed"])
    parts = [gen(kind, n, rng) for kind, n in (case["adapter"], case["polya"], case["rna"])]
    a_e = parts[0].size
    p_e = a_e + parts[1].size
    S = p_e + parts[2].size
    assert S <= M
    row = np.full(M, np.nan, dtype=np.float32)
    row[:S] = np.concatenate(parts)
    return row, S, a_e, p_e


def segments(case):
    """the three slices as the kernel sees them: {"adapter" | "polya" | "rna": float32 array}"""
    row, S, a_e, p_e = build(case)
    return {"adapter": row[:a_e], "polya": row[a_e:p_e], "rna": row[p_e:S]}


def batch(cases):
    """-> (signals float32[n, M], lens int32[n], bounds int64[n, 2]: adapter end and ONE poly(A) candidate per read)"""
    sig = np.empty((len(cases), M), dtype=np.float32)
    lens = np.empty(len(cases), dtype=np.int32)
    bounds = np.empty((len(cases), 2), dtype=np.int64)
    for i, c in enumerate(cases):
        sig[i], lens[i], bounds[i, 0], bounds[i, 1] = build(c)
    return sig, lens, bounds


FIELDS = [p + "_" + s for p in ("adapter", "polya", "rna_preloaded") for s in ("mean", "std", "med", "mad")]


def numpy_stats(case):
    """the twelve statistics as plain numpy gives them on the float32 slices (signal_partitions.py:81-96) -> {field: float}"""
    out = {}
    with np.errstate(all="ignore"):
        for part, x in segments(case).items():
            p = "rna_preloaded" if part == "rna" else part
            med = np.median(x)
            for s, v in (("mean", np.mean(x)), ("std", np.std(x)), ("med", med), ("mad", np.median(np.abs(x - med)))):
                assert v.dtype == np.float32
                out[p + "_" + s] = float(v)
    return out


def expected_tallies(cases):
    """what the cases' tags imply for the device's tallies: every poly(A) / RNA segment of at least 8192 samples without a NaN
    counts in slot 0; the tags under test give the least the other slots rise by -> dict"""
    t = {"segments": 0, "proven": 0, "fallback_med": 0, "not_predicted": 0, "bracket_overflow": 0, "unproven": 0,
         "one_value_bucket": 0, "dense_bucket": 0}
    for c in cases:
        which = under_test(c)
        for part, x in segments(c).items():
            if part == "adapter" or x.size < TALLY_MIN or np.isnan(x).any():
                continue
            t["segments"] += 1
            want = c["expect"] if part == which else CONTROL
            for k in t:
                if k in want:
                    t[k] += 1
    return t
