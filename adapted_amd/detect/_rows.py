"""The [n, L] input of the module drop-ins' batch forms (_c_llr, llr, mvs): a host array, or a device pointer (int) with n and L,
and one length per read.  Each caller passes its own dtype rule and keeps its own exceptions beyond these."""
from __future__ import annotations

import numpy as np


def as_rows(x, lens, n, L, work_dtype, what, min_len=0, lens_msg=None):
    """-> (x as a C-contiguous [n, L] array of work_dtype(x.dtype) -- a device pointer passes through --, lens int64 [n]).
    ValueError: a device pointer without n and L, a host array that is not 2-D, lens not one per read in [min_len, L]"""
    if isinstance(x, int):
        if n is None or L is None:
            raise ValueError("a device pointer needs n and L")
        return x, np.asarray(lens, dtype=np.int64).reshape(-1)
    x = np.asarray(x)
    x = np.ascontiguousarray(x, dtype=work_dtype(x.dtype))
    if x.ndim != 2:
        raise ValueError("%s must be [n, L]" % what)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if lens.size != x.shape[0] or (lens.size and (lens.min() < min_len or lens.max() > x.shape[1])):
        raise ValueError(lens_msg or "need one length per read, %d <= lens <= L" % min_len)
    return x, lens
