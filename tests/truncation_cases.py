"""Inputs of the truncation tests (ADP_FLAG_TRUNCATED): synthetic RNA004 reads that go on far past the preloaded window, some of
them with a poly(A) that runs into the window's end.  Read r of a batch is changed by r % 4:
  0  unchanged (adapter, a short poly(A), RNA up to the window's end)
  1  the last 1200 observed samples replaced by poly(A)-like noise 108 + 2.5 N(0, 1): the tail window looks like poly(A), the
     stretch behind the adapter as a whole does not
  2  everything behind the synthetic adapter replaced by such noise, and five NaN at m - 300
  3  as 2 without the NaN: the poly(A) is cut off by the preload
The noise comes from numpy.random.default_rng(7), drawn in read order.  TEST INFRASTRUCTURE: nothing here runs code under test."""
import copy

import numpy as np

from adapted_amd import synth
from adapted_amd.config import get_chemistry_specific_config

SEED, RNG_SEED, BEYOND = 11, 7, 40000
_BATCHES = {}


def spc_of(primary="llr", max_obs_trace=None):
    spc = get_chemistry_specific_config("RNA004")
    spc.llr_boundaries.llr_detect = primary == "llr"
    spc.cnn_boundaries.cnn_detect = primary == "cnn"
    spc.rna_start_peak.detect_rna_start_peak = False
    if max_obs_trace:
        spc.core.max_obs_trace = int(max_obs_trace)
    spc.update_primary_method()
    spc.update_sig_preload_size()
    assert spc.primary_method == primary
    return spc


def llr_copy(spc):
    s = copy.deepcopy(spc)
    s.llr_boundaries.llr_detect, s.cnn_boundaries.cnn_detect = True, False
    s.update_primary_method()
    s.update_sig_preload_size()
    assert s.primary_method == "llr" and s.sig_preload_size == spc.sig_preload_size
    return s


def batch(m, n=48, first=0, full_len=None, rng_seed=RNG_SEED):
    """-> (signals float32 [n, m], full lengths int32 [n]; shared, nobody writes to them)"""
    key = (m, n, first, full_len, rng_seed)
    if key not in _BATCHES:
        fl = m + BEYOND if full_len is None else full_len
        sig, lens = synth.synth_batch(SEED, first, n, m, np.full(n, fl, dtype=np.int32))
        obs = min(fl, m)
        rng = np.random.default_rng(rng_seed)
        for r in range(n):
            g = r % 4
            if g == 1:
                sig[r, obs - 1200:obs] = (108.0 + 2.5 * rng.standard_normal(1200)).astype(np.float32)
            elif g in (2, 3):
                a_len = synth.read_params(SEED, first + r)[0]
                sig[r, a_len:obs] = (108.0 + 2.5 * rng.standard_normal(obs - a_len)).astype(np.float32)
                if g == 2:
                    sig[r, obs - 300:obs - 295] = np.nan
        sig.setflags(write=False)
        lens.setflags(write=False)
        _BATCHES[key] = (sig, lens)
    return _BATCHES[key]
