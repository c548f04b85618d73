"""The second segmentation of ADP_LLR_RESEGMENT (include/adapted_hip_resegment.h) restated on the CPU from the checkers alone: the
minibatch's normalisation and the read's pooled signal from ``oracle.llr_stages``, the trace from ``oracle.c_llr_trace`` (start c,
offsets 1 / 1, its own sequential float64 cumulative sums) and the poly(A) index from ``llr_module_restated.spike``.
TEST INFRASTRUCTURE: nothing here runs code under test."""
import numpy as np

import llr_module_restated as lm
import resegment_cases as R


def second_segmentation(orc, sig, lens, spc, mb, first=None):
    """-> (eligible bool [n], c int64 [n], p2 int64 [n]) over minibatches of mb reads; first: the first rows to take eligibility and
    (adapter end, poly(A) end) from (dicts, None for a dropped minibatch's reads) -- the CPU oracle's own when not given"""
    n = sig.shape[0]
    ds, off = int(spc.core.downscale_factor), int(spc.core.min_obs_adapter)
    elig, cs, p2s = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for a in range(0, n, mb):
        try:
            rows, np4 = orc.detect_llr(sig[a:a + mb], lens[a:a + mb], spc, return_params=True)
        except ValueError:  # the primary drops the minibatch
            continue
        for i, row in enumerate(rows):
            r = a + i
            row = row if first is None else first[r]
            if not R.eligible(row):
                continue
            p1 = int(row["llr_polya_end"])
            assert (p1 - off) % ds == 0
            c = (p1 - off) // ds
            down = orc.llr_stages(sig[r], spc, np4)["down"]
            g = orc.c_llr_trace(down, c, down.size - 1, 1, 1)
            p = lm.spike(orc, g)
            elig[r], cs[r], p2s[r] = True, c, p * ds + off if p > 0 else 0
    return elig, cs, p2s
