"""Inputs and the overlay rule of the start-peak tests of the CNN primary (ADP_WITH_START_PEAK on adp_detect_cnn).

The rule is the one k_sp_decorate(mode = 0) applies on the LLR path, restated here over K1's table
(``oracle.start_peak_table``): a row made for an exception the reference raises stays bare, a read whose K1 result is not valid
gets nothing, every other read gets start_peak_idx / _pa / _next_max_idx / _next_max_pa, start_peak_open_pore_idx only when it is
flagged, and the type.  Two forms: over the oracle's dict rows (checked on the CPU against the oracle's own LLR extension) and
over adp_row arrays (what the GPU tests expect of a call with the flag, given the same engine's call without it).

Inputs, each the smallest that covers its branch (counts asserted by the tests as preconditions):
  default   rna004_cnn_default's 48 x 17 500 signals with the preset: 42 valid / 6 invalid K1 results, 19 reads shorter than the window
  200k      rna004_cnn_200k's 12 x 201 500: 11 valid, 1 invalid
  sp200k    the signals of rna004_start_peak_200k under the CNN preset at max_obs_trace = 200000: 20 valid, one flagged type 2
  handmade  default's signals with rna_start_peak.offset1 = 5, start_peak_max_idx = 60, offset2 = 20 (all 48 valid) and open pores
            written in: reads 3, 5, 8 type 1; reads 2, 10, 12, 14 type 2; reads 4 and 6 (8000 and 3000 samples) the same edit behind
            min(len, m) // ds raw samples, unflagged
TEST INFRASTRUCTURE: nothing here runs code under test."""
import copy

import numpy as np

from adapted_amd import synth
from golden_cases import CASES, resolve_lens
from util import load_case, make_spc

SP_COLS = ["start_peak_idx", "start_peak_pa", "start_peak_next_max_idx", "start_peak_next_max_pa", "start_peak_open_pore_idx"]
SP_TYPES = {0: None, 1: "open pore in adapter", 2: "potential concatemer adapter-only read"}
HAND_TYPE1, HAND_TYPE2, HAND_BEHIND = [3, 5, 8], [2, 10, 12, 14], [4, 6]

_INPUTS, _TABLES = {}, {}


def _frozen(spc, sig, lens):
    sig = np.ascontiguousarray(sig, dtype=np.float32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    sig.setflags(write=False)
    lens.setflags(write=False)
    return spc, sig, lens


def with_section(spc, **fields):
    """a copy of the configuration with rna_start_peak fields (or ``core__x`` for core.x) changed"""
    s = copy.deepcopy(spc)
    for k, v in fields.items():
        if k.startswith("core__"):
            assert hasattr(s.core, k[6:])
            setattr(s.core, k[6:], v)
        else:
            assert hasattr(s.rna_start_peak, k), k
            setattr(s.rna_start_peak, k, v)
    s.update_primary_method()
    s.update_sig_preload_size()
    assert s.primary_method == "cnn"
    return s


def inputs(name, oracle_mod=None):
    """-> (spc, signals float32 [n, m], full lengths int32 [n]); loaded once, shared, read-only.  ``handmade`` and ``m16003`` need
    the oracle (the edits sit on the unedited table's indices)"""
    if name in _INPUTS:
        return _INPUTS[name]
    if name == "default":
        _, spc, sig, lens, _ = load_case("rna004_cnn_default")
    elif name == "200k":
        _, spc, sig, lens, _ = load_case("rna004_cnn_200k")
    elif name == "sp200k":
        spc = make_spc(CASES["rna004_cnn_200k"])
        c = CASES["rna004_start_peak_200k"]
        m = spc.sig_preload_size
        assert (c["seed"], c["first"], c["n"], m) == (29, 3000, 20, 201500)
        lens = np.asarray(resolve_lens("long200", 20, m), dtype=np.int32)
        sig, _ = synth.synth_batch(29, 3000, 20, m, lens)
    elif name == "m16003":  # a window with m % ds != 0: the ragged last pooled block at m
        spc0, _, _ = inputs("default")
        spc = with_section(spc0, core__max_obs_trace=16003)
        m = spc.sig_preload_size
        assert m % spc.core.downscale_factor != 0
        c = CASES["rna004_cnn_default"]
        lens = np.asarray(resolve_lens(c["lens"], c["n"], m), dtype=np.int32)
        sig, _ = synth.synth_batch(c["seed"], c["first"], c["n"], m, lens)
    elif name == "handmade":
        spc0, sig0, lens = inputs("default")
        spc = with_section(spc0, offset1=5, start_peak_max_idx=60, offset2=20)
        ds = int(spc.rna_start_peak.downscale_factor)
        assert ds == 10
        t = oracle_mod.start_peak_table(sig0, lens, spc)
        assert t["valid"].all(), "precondition: with this section every read has a K1 result"
        sig = np.array(sig0)
        for r in HAND_TYPE1 + HAND_TYPE2 + HAND_BEHIND:
            mx, nxt = int(t[r]["start_peak_idx"]) // ds, int(t[r]["next_greater_idx"]) // ds
            if r in HAND_TYPE1:
                sig[r, nxt * 10 + 4] = 250.0
            else:
                p = mx + (nxt - mx) // 2
                assert mx < p < nxt
                sig[r, p * 10: p * 10 + 10] = 60.0
                sig[r, p * 10 + 4] = 196.0
                if r in HAND_BEHIND:
                    assert p * 10 + 4 >= min(int(lens[r]), sig.shape[1]) // ds, "precondition: the edit lies behind the open-pore scan"
    else:
        raise KeyError(name)
    _INPUTS[name] = _frozen(spc, sig, lens)
    return _INPUTS[name]


def table(oracle_mod, key, sig, lens, spc):
    """oracle.start_peak_table, computed once per key (the inputs of one key never change)"""
    if key not in _TABLES:
        _TABLES[key] = oracle_mod.start_peak_table(sig, lens, spc)
    return _TABLES[key]


def _fields(t):
    """one valid table row -> {column: value}, the type"""
    f = {"start_peak_idx": int(t["start_peak_idx"]), "start_peak_pa": float(t["start_peak_pa"]),
         "start_peak_next_max_idx": int(t["next_greater_idx"]), "start_peak_next_max_pa": float(t["next_greater_pa"])}
    if t["has_open_pore"]:
        f["start_peak_open_pore_idx"] = int(t["open_pore_idx"])
    return f, int(t["flagged_type"])


def overlay_dicts(rows, tab):
    """the oracle's dict rows of a call without the extension -> with it"""
    out = []
    for d, t in zip(rows, tab):
        d = dict(d)
        if not d.get("_exception") and t["valid"]:
            f, typ = _fields(t)
            d.update(f)
            d["start_peak_open_pore_type"] = SP_TYPES[typ]
        out.append(d)
    return out


def overlay_rows(rows, tab):
    """adp_row[] of a call without the flag -> what the call with it must deliver, byte for byte"""
    from adapted_amd import lib

    out = rows.copy()
    for r, t in zip(out, tab):
        if 9 <= int(r["fail_code"]) <= 14 or not t["valid"] or int(r["present"]) == 0:
            continue
        f, typ = _fields(t)
        pres = int(r["present"])
        for name, v in f.items():
            c = lib.COLS.index(name)
            r["col"][c] = float(v)
            pres |= 1 << c
        r["present"] = pres
        r["start_peak_type"] = typ
    return out


def sp_view(rows):
    """the start-peak fields of adp_row[]: (values [n, 5] with NaN where absent, type [n])"""
    from adapted_amd import lib

    idx = [lib.COLS.index(c) for c in SP_COLS]
    v = np.array(rows["col"][:, idx], dtype=np.float64)
    for j, c in enumerate(idx):
        v[(rows["present"] >> np.uint64(c)) & np.uint64(1) == 0, j] = np.nan
    return v, np.array(rows["start_peak_type"])
