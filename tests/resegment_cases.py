"""Inputs and stored reference results of the re-segmentation tests (ADP_LLR_RESEGMENT, include/adapted_hip_resegment.h).

``main``: 48 synthetic RNA004 reads (adapted_amd.synth, seed 11, reads 0..47, window m = 17 500 -- the preset's: a shorter one breaks
min_obs_adapter and the peak width -- every read 40 000 samples longer than the window), read r edited by r % 6:
  1  a low stall, 55 + 2 N(0, 1), on [0, 1800 + 100 (r % 7))
  3  +20 pA on [0, 1000 + (a_len - 1000) // 2): a level step inside the adapter
  4  a high stall, 120 + 3 N(0, 1), on [0, 2200)
  2  -18 pA on the adapter's second half [a_len // 2, a_len)
  0, 5  unchanged
The noise comes from numpy.random.default_rng(5), drawn in read order.  Every read of kinds 1, 3 and 4 fails its first validation,
nearly all of them behind a first change point: (adapter end, poly(A) end) = (end of the front stretch, true adapter end).
``extra``: 16 hand-made reads (seed 13, undecorated) in two minibatches of 8 for the outcomes ``main`` does not reach: the first
minibatch is constant (MAD 0: the primary drops it), the second holds eligible reads beside reads without an adapter or a poly(A)
end, a read whose second segmentation finds nothing, and an eligible read that ends inside the window.
tools/gen_resegment_golden.py hands the batches to the real reference, one minibatch at a time, and stores what it said in
tests/golden/resegment_*.npz -- no signals: a sha256 per read shows a drift of these generators.  TEST INFRASTRUCTURE: nothing here
runs code under test."""
import hashlib
import os

import numpy as np

import revalidate_cases as rc
from adapted_amd import synth
from adapted_amd.config import get_chemistry_specific_config

M = 17500
SEED, RNG_SEED, BEYOND, N_MAIN = 11, 5, 40000, 48
X_SEED, X_RNG_SEED, X_MB = 13, 77, 8
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (batch, minibatch size) of every stored file
RUNS = (("main", 24), ("main", 48), ("extra", X_MB))
ROW_RESEGMENTED, ROW_FIRST_FAIL_SHIFT = 32, 6
SP_FIELDS = ("start_peak_idx", "start_peak_pa", "start_peak_next_max_idx", "start_peak_next_max_pa", "start_peak_open_pore_idx",
             "start_peak_open_pore_type")
_BATCHES = {}


def spc_of():
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect, spc.cnn_boundaries.cnn_detect = True, False
    spc.rna_start_peak.detect_rna_start_peak = False
    spc.update_primary_method()
    spc.update_sig_preload_size()
    assert spc.primary_method == "llr" and spc.sig_preload_size == M
    return spc


def _main():
    sig, lens = synth.synth_batch(SEED, 0, N_MAIN, M, np.full(N_MAIN, M + BEYOND, dtype=np.int32))
    rng = np.random.default_rng(RNG_SEED)
    for r in range(N_MAIN):
        a_len = synth.read_params(SEED, r)[0]
        k = r % 6
        if k == 1:
            e = 1800 + 100 * (r % 7)
            sig[r, :e] = (55.0 + 2.0 * rng.standard_normal(e)).astype(np.float32)
        elif k == 3:
            sig[r, :1000 + (a_len - 1000) // 2] += np.float32(20.0)
        elif k == 4:
            sig[r, :2200] = (120.0 + 3.0 * rng.standard_normal(2200)).astype(np.float32)
        elif k == 2:
            sig[r, a_len // 2:a_len] -= np.float32(18.0)
    return sig, lens


# the second minibatch of ``extra``: (name, read of seed 13, edits, full_len as a function of (a_len, p_len))
_LONG = M + BEYOND
X_READS = (
    ("stall", 0, ("stall",), lambda a, p: _LONG),
    ("stall.ends_in_window", 2, ("stall",), lambda a, p: a + p + 3000),
    ("stall.cut_behind_adapter", 3, ("stall",), lambda a, p: a + 250),
    ("flat", 5, ("flat",), lambda a, p: _LONG),
    ("tiny", 8, (), lambda a, p: 1500),
    ("plain", 8, (), lambda a, p: _LONG),
    ("adapter_only", 6, ("adapter_only",), lambda a, p: _LONG),
    ("stall.adapter_only", 7, ("stall", "adapter_only"), lambda a, p: _LONG),
)
X_NAMES = ["constant.%d" % i for i in range(X_MB)] + [x[0] for x in X_READS]


def _extra():
    rng = np.random.default_rng(X_RNG_SEED)
    n = 2 * X_MB
    sig = np.full((n, M), np.float32(90.0), dtype=np.float32)
    lens = np.full(n, _LONG, dtype=np.int32)
    for i, (_, read, edits, fl) in enumerate(X_READS):
        a, p = synth.read_params(X_SEED, read, False)[:2]
        x = synth.synth_read(X_SEED, read, M, None, decorate=False).copy()
        if "flat" in edits:
            x[:] = (90.0 + 3.0 * rng.standard_normal(M)).astype(np.float32)
        if "adapter_only" in edits:
            x[a:] = (80.0 + 7.0 * rng.standard_normal(M - a)).astype(np.float32)
        if "stall" in edits:
            x[:1900] = (55.0 + 2.0 * rng.standard_normal(1900)).astype(np.float32)
        lens[X_MB + i] = fl(a, p)
        x[min(int(lens[X_MB + i]), M):] = np.nan
        sig[X_MB + i] = x
    return sig, lens


def batch(name):
    """-> (signals float32 [n, M] NaN padded, full lengths int32 [n]); shared, nobody writes to them"""
    if name not in _BATCHES:
        sig, lens = {"main": _main, "extra": _extra}[name]()
        sig.setflags(write=False)
        lens.setflags(write=False)
        _BATCHES[name] = (sig, lens)
    return _BATCHES[name]


def digests(sig):
    return np.array([hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in sig])


def tiled(name, times):
    sig, lens = batch(name)
    return np.tile(sig, (times, 1)), np.tile(lens, times)


# ---- the stored results ---------------------------------------------------------------------------------------------------------
def golden_path(name, mb):
    return os.path.join(GOLD, "resegment_%s_mb%d.npz" % (name, mb))


def pack(first, eligible, c, p2, second, sig, blank):
    """first / second: one dict (DetectResults.__dict__) or None per read; blank: the dict of DetectResults(success=False), which
    stands where a read has no row (the ``given`` masks say where)"""
    out = {}
    for prefix, rows in (("first.", first), ("second.", second)):
        for k, v in rc.encode([blank if r is None else r for r in rows]).items():
            out[prefix + k] = v
        out[prefix + "given"] = np.array([r is not None for r in rows])
    out["eligible"] = np.asarray(eligible, dtype=bool)
    out["c"] = np.asarray(c, dtype=np.int64)
    out["p2"] = np.asarray(p2, dtype=np.int64)
    out["sha256"] = digests(sig)
    return out


def load(name, mb):
    """-> dict(first, second: one dict or None per read (first None: a read of a minibatch the reference drops; second None: the
    read was not validated again), eligible bool [n], c, p2 int64 [n] (0 where not eligible))"""
    z = np.load(golden_path(name, mb))
    sig, _ = batch(name)
    assert z["sha256"].tolist() == digests(sig).tolist(), "tests/resegment_cases.py no longer makes the reads the fixture was made from"
    out = {}
    for key in ("first", "second"):
        rows = rc.decode(z, key + ".")
        out[key] = [r if g else None for r, g in zip(rows, z[key + ".given"])]
    out.update(eligible=z["eligible"], c=z["c"], p2=z["p2"])
    return out


def eligible(row):
    """the rule's eligibility of a first row (a dict, or None for a read of a dropped minibatch)"""
    if row is None or row["success"] or row.get("signal_len") is None:  # (signal_len None: a row that only carries an exception)
        return False
    a1, p1 = row.get("llr_adapter_end"), row.get("llr_polya_end")
    return a1 is not None and a1 > 0 and p1 is not None and p1 > a1


_FAIL_CODES = (("No adapter detected (primary)", 1), ("adapter MAD check failed", 2), ("Open pore too close to boundary", 3),
               ("Real signal check failed", 4), ("No polya detected (primary)", 5), ("MVS polya check failed: not enough signal", 6),
               ("MVS polya check failed: ", 7), ("Median shift check failed", 8), ("No adapter detected in range (mvs_detect)", 15))


def fail_code(reason):
    for text, code in _FAIL_CODES:
        if reason == text or (code == 7 and reason.startswith(text)):
            return code
    raise ValueError(reason)


def fail_text(code):
    return dict((c, t) for t, c in _FAIL_CODES)[code].rstrip(": ")


def expected(g, first=None):
    """what a flagged call delivers, from the stored results: (one dict or None per read with ``llr_detect_log`` and ``_reserved``
    added, (eligible, p2 > 0, replaced), outcome per read: "dropped" / "ineligible" / "no_p2" / "second_failed" / "kept").
    first: the call's own first rows where they carry more than the reference's (the start-peak columns)"""
    first = g["first"] if first is None else first
    out, kinds = [], []
    for r, row in enumerate(first):
        second = g["second"][r]
        if row is None:
            out.append(None)
            kinds.append("dropped")
            continue
        new = dict(row, llr_detect_log="", _reserved=0)
        kind = "ineligible"
        if g["eligible"][r]:
            kind = "no_p2" if g["p2"][r] == 0 else "second_failed"
            if second is not None and second["success"]:
                kind = "kept"
                code = fail_code(g["first"][r]["fail_reason"])
                new = dict(second, _reserved=ROW_RESEGMENTED | code << ROW_FIRST_FAIL_SHIFT,
                           llr_detect_log="resegmented: first pass failed (%s)" % fail_text(code))
                for k in SP_FIELDS:
                    new[k] = row.get(k)
        out.append(new)
        kinds.append(kind)
    counts = (int(g["eligible"].sum()), int((g["p2"] > 0).sum()), kinds.count("kept"))
    return out, counts, kinds


def coverage(name, g):
    """what a stored run reaches -> {condition: reads}"""
    _, lens = batch(name)
    _, _, kinds = expected(g)
    cov = {}

    def hit(what, r):
        cov.setdefault(what, []).append(r)

    for r, (kind, row) in enumerate(zip(kinds, g["first"])):
        if kind == "ineligible" and row["success"]:
            hit("ineligible, passes", r)
        if kind == "ineligible" and not row["success"] and not (row.get("llr_adapter_end") or 0) > 0:
            hit("ineligible: no adapter", r)
        if kind == "ineligible" and not row["success"] and (row.get("llr_adapter_end") or 0) > 0:
            hit("ineligible: no poly(A) end behind the adapter end", r)
        if kind == "kept":
            hit("kept", r)
        if kind == "second_failed":
            hit("second validation fails", r)
        if kind == "no_p2":
            hit("p2 == 0", r)
        if g["eligible"][r] and lens[r] < M:
            hit("eligible read shorter than the window", r)
        if kind == "dropped":
            hit("a minibatch the primary drops", r)
    if "a minibatch the primary drops" in cov and g["eligible"].any():
        cov["a dropped minibatch beside one with eligible reads"] = cov["a minibatch the primary drops"]
    return cov


REQUIRED = {"main": ["ineligible, passes", "kept", "second validation fails"],
            "extra": ["ineligible: no adapter", "ineligible: no poly(A) end behind the adapter end", "p2 == 0", "kept",
                      "eligible read shorter than the window", "a dropped minibatch beside one with eligible reads"]}
