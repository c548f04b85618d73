"""Cases of the validation from a given adapter start (adp_validate_candidates_from, detect.combined.validate_boundaries with
Boundaries.adapter_start): one synthetic read (adapted_amd.synth, seed 7, read 4, undecorated: adapter N(80, 7^2) up to A = 4242,
poly(A) N(108, 2.5^2) up to A + P = 4952, RNA behind), edited per case, validated with bounds (adapter_end, three poly(A)
candidates, 0 = none) from ``start``.  Both presets run every case.  tools/gen_revalidate_golden.py hands the cases to the real
reference and stores signals, bounds, starts and the reference's DetectResults in tests/golden/revalidate_*.npz; ``coverage``
names what the case list must reach, from the stored arrays alone.  TEST INFRASTRUCTURE: nothing here runs code under test."""
import os

import numpy as np

from adapted_amd import synth

M = 12288
SEED, READ = 7, 4
A, P = synth.read_params(SEED, READ, False)[:2]
assert (A, P) == (4242, 710)
PE = A + P
KEEP = PE + 2500  # samples of the read that exist (full_len) unless the case says otherwise
K = 3
CHEMS = ("RNA002", "RNA004")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RNG_SEED = 20240607

# edits: ("set", lo, hi, value) | ("noise", lo, hi, mean, sd) | ("add", lo, hi, delta) | ("spikes", [positions], value) |
#        ("bimodal", lo, hi, delta): +delta on every 5th sample, -delta on the next
CASES = [
    dict(name="pass.s501", start=501),
    dict(name="pass.s502", start=502),
    dict(name="pass.s503", start=503),
    dict(name="pass.s2", start=2),
    dict(name="mad_fail.flat", start=501, edits=[("noise", 501, A, 80.0, 1.0)]),
    dict(name="mad_fail.wide", start=777, edits=[("noise", 777, A, 80.0, 25.0)]),
    dict(name="mad_zero.const", start=1001, edits=[("set", 1001, A, 80.0)]),
    dict(name="mad_zero.one", start=A - 1),
    dict(name="pore.close", start=501, edits=[("spikes", [A - 500], 230.0)]),
    dict(name="pore.at_start", start=601, edits=[("spikes", [601], 230.0)]),
    dict(name="pore.front_only", start=601, edits=[("spikes", [551, 580], 230.0)]),
    dict(name="pore.straddle7", start=603, edits=[("spikes", [599, 606, 623, 628], 230.0)]),
    dict(name="pore.straddle11", start=603, edits=[("spikes", [599, 610, 615], 230.0)]),
    dict(name="pore.straddle_pair", start=603, edits=[("spikes", [598, 605], 230.0)]),
    dict(name="pore.many", start=502, edits=[("spikes", list(range(600, 600 + 15 * 21, 15)), 230.0)]),
    dict(name="pore.many_front", start=1003, edits=[("spikes", list(range(600, 600 + 15 * 21, 15)) + list(range(1100, 1100 + 12 * 19, 12)), 230.0)]),
    dict(name="real.short", start=A - 400),
    dict(name="real.long_fail", start=501, edits=[("bimodal", 501, A, 40.0)]),
    dict(name="real.n63", start=A - 63),
    dict(name="real.n64", start=A - 64),
    dict(name="real.n65", start=A - 65),
    dict(name="real.n2560", start=A - 2560),
    dict(name="real.n640", start=A - 640),
    dict(name="long_adapter", start=503, adapter_end=A + 2500, cands=[A + 3500, 0, 0], keep=A + 6000,
         edits=[("noise", A, A + 2500, 80.0, 7.0), ("noise", A + 2500, A + 3500, 108.0, 2.5)]),
    dict(name="mvs_flip", start=2601, edits=[("add", 0, 2601, -12.0), ("add", 2601, A, 6.0)]),
    dict(name="second_cand", start=501, cands=[PE + 1500, PE, PE - 50]),
    dict(name="second_cand.pore", start=502, cands=[PE + 1500, PE, 0], edits=[("spikes", [900, 930], 230.0)]),
    dict(name="short_read", start=503, keep=A - 300),
    dict(name="short_read.tiny", start=A - 401, keep=A - 300),
]
NAMES = [c["name"] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def build(case):
    """-> (signal float32 [full_len], bounds int64 [1 + K], start, full_len)"""
    x = synth.synth_read(SEED, READ, M, None, decorate=False).copy()
    rng = np.random.default_rng(RNG_SEED + NAMES.index(case["name"]))
    for e in case.get("edits", ()):
        if e[0] == "set":
            x[e[1]:e[2]] = np.float32(e[3])
        elif e[0] == "noise":
            x[e[1]:e[2]] = (e[3] + e[4] * rng.standard_normal(e[2] - e[1])).astype(np.float32)
        elif e[0] == "add":
            x[e[1]:e[2]] += np.float32(e[3])
        elif e[0] == "spikes":
            x[np.asarray(e[1], dtype=np.int64)] = np.float32(e[2])
        elif e[0] == "bimodal":
            i = np.arange(e[1], e[2])
            x[i[(i - e[1]) % 5 == 0]] += np.float32(e[3])
            x[i[(i - e[1]) % 5 == 1]] -= np.float32(e[3])
        else:
            raise ValueError(e[0])
    keep = int(case.get("keep", KEEP))
    assert keep <= M
    b = np.zeros(1 + K, dtype=np.int64)
    b[0] = case.get("adapter_end", A)
    b[1:] = case.get("cands", [PE, 0, 0])
    return x[:keep].copy(), b, int(case["start"]), keep


# ---- the reference's DetectResults as arrays, and back --------------------------------------------------------------------
LIST_FIELDS = ("open_pores", "polya_candidates")
STR_FIELDS = ("fail_reason", "start_peak_open_pore_type", "llr_detect_log")


def encode(results):
    """DetectResults.__dict__ of every case -> arrays: per field its kind, the values and a mask of its None cells"""
    out = {}
    keys = sorted(results[0])
    out["fields"] = np.array(keys)
    kinds = []
    for k in keys:
        vals = [r[k] for r in results]
        none = np.array([v is None for v in vals])
        out["none." + k] = none
        if k in LIST_FIELDS:
            kinds.append("l")
            lists = [np.zeros(0, dtype=np.int64) if v is None else np.asarray(v, dtype=np.int64).ravel() for v in vals]
            out["len." + k] = np.array([a.size for a in lists], dtype=np.int64)
            out["val." + k] = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
        elif k in STR_FIELDS or any(isinstance(v, str) for v in vals):
            kinds.append("s")
            out["val." + k] = np.array(["" if v is None else str(v) for v in vals])
        else:
            have = [v for v in vals if v is not None]
            if all(isinstance(v, (bool, np.bool_)) for v in have):
                kinds.append("b")
            elif all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in have):
                kinds.append("i")
            elif all(isinstance(v, np.float32) for v in have) and have:
                kinds.append("g")  # numpy float32 scalars
            else:
                kinds.append("f")
            out["val." + k] = np.array([np.nan if v is None else float(v) for v in vals], dtype=np.float64)
    out["kinds"] = np.array(kinds)
    return out


def decode(z, prefix=""):
    """-> one dict per case, as tests/util.py's row_diffs takes them"""
    keys, kinds = [str(k) for k in z[prefix + "fields"]], [str(k) for k in z[prefix + "kinds"]]
    n = z[prefix + "none." + keys[0]].size
    rows = [dict() for _ in range(n)]
    for k, kind in zip(keys, kinds):
        none, val = z[prefix + "none." + k], z[prefix + "val." + k]
        off = np.concatenate([[0], np.cumsum(z[prefix + "len." + k])]) if kind == "l" else None
        for i in range(n):
            if none[i]:
                v = None
            elif kind == "l":
                v = [int(t) for t in val[off[i]:off[i + 1]]]
            elif kind == "s":
                v = str(val[i])
            elif kind == "b":
                v = bool(val[i])
            elif kind == "i":
                v = int(val[i])
            else:
                v = float(val[i])
            rows[i][k] = v
    return rows


def load(chem):
    """-> (signals list of float32 arrays, bounds int64 [n, 1 + K], starts int64 [n], full_lens int32 [n], the reference's rows,
    what the reference said from start 0: success bool [n], fail_reason str [n], adapter_med float64 [n])"""
    s = np.load(os.path.join(GOLD, "revalidate_signals.npz"))
    z = np.load(os.path.join(GOLD, "revalidate_%s.npz" % chem))
    assert [str(x) for x in s["names"]] == NAMES and [str(x) for x in z["names"]] == NAMES, "regenerate the fixtures: the case list changed"
    off = np.concatenate([[0], np.cumsum(s["full_lens"])])
    sigs = [s["samples"][off[i]:off[i + 1]] for i in range(len(NAMES))]
    return sigs, s["bounds"], s["starts"], s["full_lens"].astype(np.int32), decode(z), (z["ref0.success"], z["ref0.fail_reason"], z["ref0.adapter_med"])


def padded(sigs, m=M):
    """the signals as a detect call's NaN padded float32 [n, m] minibatch"""
    X = np.full((len(sigs), m), np.nan, dtype=np.float32)
    for i, x in enumerate(sigs):
        X[i, :x.size] = x
    return X


def coverage(sigs, bounds, starts, full_lens, rows, ref0, mean_window=300, max_obs_local_range=5000, var_hi=20.0, mean_scale_lo=1.3):
    """what the case list reaches (all with start > 0) -> {condition: the cases that reach it}.
    The reference never resets ``success`` once a candidate failed (combined.py:490-566), so no later candidate can make a row pass:
    what the list reaches instead is a row whose first candidate fails the MVS mean and variance gates and whose reported MVS values
    -- the last evaluated candidate's -- pass them."""
    cov = {}

    def hit(name, i):
        cov.setdefault(name, []).append(NAMES[i])

    for i, (x, b, s, fl, r) in enumerate(zip(sigs, bounds, starts, full_lens, rows)):
        s, ae, fl = int(s), int(b[0]), int(fl)
        assert s > 0
        end = min(ae, fl)
        n = end - s
        fr = r["fail_reason"]
        pores = r["open_pores"]
        hits = np.flatnonzero(x[:end] >= 200.0)
        if r["success"]:
            hit("passes", i)
        if fr == "adapter MAD check failed":
            hit("adapter MAD check failed", i)
        if r["adapter_mad"] == 0.0 and pores is not None and len(pores) == 0 and r["adapter_start"] == s:
            hit("MAD 0, one sample" if n == 1 else "MAD 0, constant slice", i)
        if fr == "Open pore too close to boundary":
            hit("Open pore too close to boundary", i)
        if pores is not None and s in pores:
            hit("pore exactly at start", i)
        if pores is not None and len(pores) == 0 and (hits < s).any():
            hit("pores only in front of start", i)
        if any(h2 - h1 < 10 for h1 in hits[hits < s] for h2 in hits[hits >= s]):
            hit("hits closer than 10 apart on either side of start", i)
        if pores is not None and len(pores) > 16:
            hit("more than 16 pores behind start", i)
        if fr == "Real signal check failed":
            hit("Real signal check failed, values None" if r["real_adapter_mean_start"] is None else "Real signal check failed, values given", i)
            if r["real_adapter_mean_start"] is None:
                assert end - int(r["adapter_start"]) < 2 * mean_window
        if r["real_adapter_local_range"] is not None:
            hit("slice shorter than max_obs_local_range" if end - int(r["adapter_start"]) < max_obs_local_range else "slice longer than max_obs_local_range", i)
        s0, f0, med0 = bool(ref0[0][i]), str(ref0[1][i]), float(ref0[2][i])
        reasons = [t for ok, t in ((s0, f0), (r["success"], fr or "")) if not ok]
        if s0 != bool(r["success"]) and reasons[0].startswith("MVS polya check failed:") and "mean" in reasons[0] and med0 != r["adapter_med"]:
            hit("MVS mean gate flips with the start", i)
        if (b[2] != 0 and fr == "MVS polya check failed: mean var" and r["mvs_detect_var_at_loc"] <= var_hi
                and r["mvs_detect_mean_at_loc"] >= mean_scale_lo * r["adapter_med"]):
            hit("a later candidate passes the gates the first failed", i)
        if fl < ae:
            hit("full_len < adapter_end", i)
        hit("start = %d (mod 4)" % (s % 4), i)
        if s % 2:
            hit("odd start", i)
        if n in (63, 64, 65):
            hit("slice of %d samples" % n, i)
        elif n >= 128 and n % 64 == 0:
            hit("slice of 64 k samples", i)
    return cov


REQUIRED = ["passes", "adapter MAD check failed", "MAD 0, one sample", "MAD 0, constant slice", "Open pore too close to boundary",
            "pore exactly at start", "pores only in front of start", "hits closer than 10 apart on either side of start",
            "more than 16 pores behind start", "Real signal check failed, values None", "Real signal check failed, values given",
            "slice shorter than max_obs_local_range", "slice longer than max_obs_local_range", "MVS mean gate flips with the start",
            "a later candidate passes the gates the first failed", "full_len < adapter_end", "start = 1 (mod 4)", "start = 2 (mod 4)",
            "start = 3 (mod 4)", "odd start", "slice of 63 samples", "slice of 64 samples", "slice of 65 samples", "slice of 64 k samples"]


# ---- reads for the re-validating front pass (adp_adapter_front_revalidate): the detector runs with window 16, min_obs_adapter 64
FRONT_SEED, FRONT_N = 11, 32
_FRONT = {}


def front_batch(n=FRONT_N, m=M):
    """-> (signals float32 [n, m], every sample a multiple of 0.25 pA, NaN behind each read's end; full lengths int32 [n]; bounds
    int64 [n, 1 + K] of the first validation: the synthetic adapter end and poly(A) end, a second candidate 40 samples in front;
    kinds {name: read indices}).  Read r by r % 4:
      0  the first 400 samples raised by 70 pA: the detector trims them and the trimmed read passes again
      1  adapter noise of sd 4.1 and the first 12 % of the adapter raised by 70 pA: from start 0 the raised samples lift the adapter
         MAD over 3, from the trimmed start it is below (0.6745 x 4.1 = 2.8): the trim is rejected
      2  untouched: the detector accepts nothing
      3  as 0 with an open pore 300 samples in front of the adapter end: the first row fails, the pass does not look at it
    Shared, nobody writes to them."""
    key = (n, m)
    if key not in _FRONT:
        sig, _ = synth.synth_batch(FRONT_SEED, 0, n, m, decorate=False)
        sig = sig.copy()
        rng = np.random.default_rng(RNG_SEED)
        lens = np.full(n, m, dtype=np.int32)
        bounds = np.zeros((n, 1 + K), dtype=np.int64)
        kinds = {"kept": [], "rejected": [], "untouched": [], "failing": []}
        for r in range(n):
            a, p = synth.read_params(FRONT_SEED, r, False)[:2]
            bounds[r] = (a, a + p, a + p - 40, 0)
            g = r % 4
            if g == 1:
                sig[r, :a] = (80.0 + 4.1 * rng.standard_normal(a)).astype(np.float32)
                sig[r, :int(0.12 * a)] += np.float32(70.0)
            elif g in (0, 3):
                sig[r, :400] += np.float32(70.0)
                if g == 3:
                    sig[r, a - 300] = np.float32(230.0)
            if r % 5 == 4:
                lens[r] = a + p + 1500 + r
            kinds[("kept", "rejected", "untouched", "failing")[g]].append(r)
        sig = (np.round(sig * 4.0) / 4.0).astype(np.float32)
        for r in range(n):
            sig[r, lens[r]:] = np.nan
        for arr in (sig, lens, bounds):
            arr.setflags(write=False)
        _FRONT[key] = (sig, lens, bounds, kinds)
    return _FRONT[key]
