"""The truncation look of ADP_FLAG_TRUNCATED (include/adapted_hip.h) restated on the CPU from the checkers alone: first rows as
the CPU oracle returns them (dicts), T1 through tests/mvs_module_restated.check, T2 through oracle.detect_cnn_from_preds on the
one read with the boundaries (adapter end, obs_end).  TEST INFRASTRUCTURE: nothing here runs code under test."""
import types
import warnings

import numpy as np

import mvs_module_restated as mvs

SP_FIELDS = ("start_peak_idx", "start_peak_pa", "start_peak_next_max_idx", "start_peak_next_max_pa", "start_peak_open_pore_idx",
             "start_peak_open_pore_type")
RNA_FIELDS = ("rna_preloaded_start", "rna_preloaded_len", "rna_preloaded_mean", "rna_preloaded_std", "rna_preloaded_med", "rna_preloaded_mad")


def _empty(r):
    return r is None or (r[0] is None and r[1] is None)


def primary_of(row, call_primary):
    """how a first row names its primary columns: a row the LLR second opinion made carries llr_* whatever the call"""
    return "llr" if row.get("_second_llr") else call_primary


def t1_params(spc, adapter_med):
    M = spc.mvs_polya
    rng = M.pA_mean_range
    if _empty(rng):
        s = M.pA_mean_adapter_med_scale_range
        if _empty(s):
            return None
        rng = (None if s[0] is None else s[0] * adapter_med, None if s[1] is None else s[1] * adapter_med)
    return types.SimpleNamespace(median_shift_window=M.median_shift_window, pA_var_window=M.pA_var_window, pA_mean_window=M.pA_mean_window,
                                 pA_mean_range=rng, pA_var_range=M.pA_var_range, polyA_med_range=M.polyA_med_range,
                                 polyA_local_range=M.polyA_local_range, median_shift_range=M.median_shift_range)


def eligible(row, full_len, m, spc, call_primary):
    """-> (adapter end, obs_end, T1 parameters) or None"""
    if row is None or row.get("_exception") or full_len <= m:  # (None: a read of a dropped minibatch)
        return None
    ae = row.get(primary_of(row, call_primary) + "_adapter_end")
    if ae is None or ae <= 0 or row.get("adapter_med") is None:
        return None
    obs_end = min(int(full_len), m)
    if ae + spc.mvs_polya.median_shift_window > obs_end:
        return None
    params = t1_params(spc, row["adapter_med"])
    if params is None:
        return None
    return int(ae), obs_end, params


def t1(signal, obs_end, params):
    W = params.median_shift_window
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        res = mvs.check(np.asarray(signal[:obs_end]), obs_end - W, obs_end, params, return_values=True, less_signal_ok=True, windowed_stats=True)
    return bool(np.asarray(res[1])[:4].all())


def look(oracle_mod, sig, lens, first, spc, call_primary):
    """first: the call's rows in front of the look (oracle dicts; None for a read of a dropped minibatch) ->
    (expected dicts with ``polya_truncated`` and ``_reserved`` added, (eligible, T1 passed, rows replaced), outcome per read:
    "ineligible" / "t1_failed" / "t2_failed" / "flagged")"""
    n, m = sig.shape
    out, kinds = [], []
    n_el = n_t1 = n_rep = 0
    for r in range(n):
        row = first[r]
        el = eligible(row, int(lens[r]), m, spc, call_primary)
        kind, new = "ineligible", None
        if el is not None:
            ae, obs_end, params = el
            n_el += 1
            kind = "t1_failed"
            if t1(sig[r], obs_end, params):
                n_t1 += 1
                kind = "t2_failed"
                t2 = oracle_mod.detect_cnn_from_preds(sig[r:r + 1], lens[r:r + 1], np.array([[ae, obs_end]], dtype=np.int64), spc)[0]
                if t2["success"]:
                    n_rep += 1
                    kind = "flagged"
                    p = primary_of(row, call_primary)
                    new = {k: v for k, v in t2.items() if k not in ("cnn_adapter_end", "cnn_polya_end")}
                    new[p + "_adapter_end"] = t2["cnn_adapter_end"]
                    new[p + "_polya_end"] = row[p + "_polya_end"]
                    new["polya_candidates"] = row["polya_candidates"]
                    for k in SP_FIELDS:
                        new[k] = row[k]
                    assert all(new[k] is None for k in RNA_FIELDS[1:])
                    new["rna_preloaded_start"] = None
                    new["polya_truncated"] = True
                    new["_reserved"] = 2 | 4 | (1 if row.get("_second_llr") else 0)
        if new is None:
            if row is None:
                new = None
            else:
                new = dict(row)
                new["polya_truncated"] = False if (row["success"] and not row.get("_exception")) else None
                new["_reserved"] = 4 | (1 if row.get("_second_llr") else 0)
        out.append(new)
        kinds.append(kind)
    return out, (n_el, n_t1, n_rep), kinds


def second_llr(first_cnn, llr_rows):
    """the rows behind ADP_CNN_SECOND_LLR: a read whose CNN row fails (exception rows included) gets its minibatch's LLR row where
    that one passes (llr_rows: oracle.detect_llr dicts, None for a minibatch the LLR primary drops)"""
    out = []
    for c, l in zip(first_cnn, llr_rows):
        if not c["success"] and l is not None and l["success"]:
            l = dict(l)
            l["_second_llr"] = True
            out.append(l)
        else:
            out.append(c)
    return out


_LLR = {}


def llr_first_rows(oracle_mod, sig, lens, spc, mb, with_start_peak=False, key=None):
    """oracle.detect_llr minibatch by minibatch (None for the reads of a minibatch it drops); cached under key"""
    k = (key, mb, with_start_peak)
    if key is not None and k in _LLR:
        return _LLR[k]
    out = []
    for a in range(0, sig.shape[0], mb):
        try:
            out += oracle_mod.detect_llr(sig[a:a + mb], lens[a:a + mb], spc, with_start_peak=with_start_peak)
        except ValueError:
            out += [None] * min(mb, sig.shape[0] - a)
    if key is not None:
        _LLR[k] = out
    return out


def public(d):
    return {k: v for k, v in d.items() if not k.startswith("_")}
